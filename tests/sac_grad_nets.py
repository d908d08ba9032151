"""Inputs and NumPy models for the tests of pd_sac_critic_grad and pd_adam_step (plain NumPy; no
GPU, no torch at import).  Builds on sac_nets.py and sac_td_nets.py.

`backward` is the backward pass of one Q net -- q, the loss gradient given as dq, every delta and
every parameter gradient -- in int64 (the integer fixture: the reference the kernel must EQUAL) or
binary64 (the real-valued cases), with the largest sum of absolute terms of any partial sum it forms.
The integer fixture: sac_td_nets' integer twin critic, integer state | action and an integer dq_in
in [-2, 2]; every partial sum of the forward pass, of every delta and of every gradient entry is an
integer below 2**24, so any float32 evaluation in any order gives the integer's bits.

`loss_model` is the four losses of sac_pytorch.py:457-468 in binary64 on given float32 q, target and
weights, with the a-priori float32 bounds of dq, td_abs and the loss; `adam_model` is
clip_grad_norm_, Adam.step and the Polyak update in binary64 with the a-priori bound of every
result (tests/test_gpu_sac_update.py derives both)."""
import numpy as np

import sac_nets as sn
import sac_td_nets as td

SHAPES_N = td.SHAPES_N                   # one per hidden width
BATCHES = [1, 15, 16, 17, 37]            # the row-tile edges; 37 = 9 * 4 + 1
SHAPES_DEEP = [(5, 4, 256, 3), (1, 1, 128, 8)]   # at n = 37: two and seven chained hidden-layer steps
EPS32 = 2.0 ** -24
SECOND_ORDER = 1.01
L2, L1 = 0, 1                            # PD_SAC_LOSS_*


def int_dq(n, seed=0):
    """[n][2] integer upstream gradients in [-2, 2] (zeros among them), float32."""
    return np.random.default_rng([seed, n, 5]).integers(-2, 3, (n, 2)).astype(np.float32)


def backward(params, sa, dq, dtype=np.int64):
    """One Q net (params: W1 [H][D], b1, (W [H][H], b) x (L - 1), W [1][H], b [1]) on sa [n][D] with
    the upstream gradient dq [n]: dict of
      q [n], grads (the parameters' order), h (post-ReLU activations per layer), deltas (per layer),
      abs_sum: the largest, over the forward pass, every delta and every gradient entry, of the sum
               of the absolute values of the terms of one sum,
      terms:   per gradient tensor, the largest such sum over its entries,
      zero_pre: how many pre-activations are exactly 0 (ReLU's derivative there is 0),
      live:    the share of positive units after the last hidden layer."""
    ps = [np.asarray(p).astype(dtype) for p in params]
    L = len(ps) // 2 - 1
    x = np.asarray(sa).astype(dtype)
    dq = np.asarray(dq).astype(dtype)
    ab = np.abs
    hs, abs_sum, zero_pre = [], 0, 0
    h = x
    for l in range(L):
        W, b = ps[2 * l], ps[2 * l + 1]
        abs_sum = max(abs_sum, (ab(h) @ ab(W).T + ab(b)).max())
        z = h @ W.T + b
        zero_pre += int((z == 0).sum())
        h = np.maximum(z, 0)
        hs.append(h)
    wm, bm = ps[2 * L], ps[2 * L + 1]
    abs_sum = max(abs_sum, (ab(h) @ ab(wm).T + ab(bm)).max())
    q = (h @ wm.T + bm)[:, 0]
    grads = [None] * (2 * (L + 1))
    terms = [None] * (2 * (L + 1))

    def put(k, value, t):
        grads[k], terms[k] = value, t.max() if t.size else 0

    put(2 * L, (dq[None, :] @ hs[-1]), ab(dq)[None, :] @ ab(hs[-1]))
    put(2 * L + 1, dq.sum(keepdims=True), ab(dq).sum(keepdims=True))
    delta = dq[:, None] * wm[0][None, :] * (hs[-1] > 0)
    deltas = [None] * L
    for l in range(L - 1, -1, -1):
        deltas[l] = delta
        below = hs[l - 1] if l > 0 else x
        put(2 * l, delta.T @ below, ab(delta).T @ ab(below))
        put(2 * l + 1, delta.sum(axis=0), ab(delta).sum(axis=0))
        if l > 0:
            abs_sum = max(abs_sum, (ab(delta) @ ab(ps[2 * l])).max())
            delta = (delta @ ps[2 * l]) * (hs[l - 1] > 0)
    abs_sum = max([abs_sum] + terms)
    return dict(q=q, grads=grads, h=hs, deltas=deltas, abs_sum=abs_sum, terms=terms, zero_pre=zero_pre,
                live=float((hs[-1] > 0).mean()))


_int = {}


def int_grad_case(S, A, H, L, n=sn.N_EXACT):
    """The integer fixture of a shape over the first n of its 37 rows (computed once per (shape, n)):
    dict of params (q1, q2), sa [n][S + A], dq [n][2], q [n][2] and grads (q1's, q2's) as float32, with
    the conditions asserted on the int64 model: every sum of absolute terms below 2**24 (forward, deltas,
    gradients), every value a float32 integer, and -- at n = 37 -- pre-activations that are exactly 0,
    a live share in [0.2, 0.8] and gradient tensors that are not all zero."""
    key = (S, A, H, L, n)
    if key in _int:
        return _int[key]
    p1, p2, states, actions, _ = td.int_critic_case(S, A, H, L)
    sa = np.concatenate([states, actions], axis=1)[:n]
    dq = int_dq(sn.N_EXACT)[:n]
    out = dict(params=(p1, p2), sa=np.ascontiguousarray(sa), dq=np.ascontiguousarray(dq), q=[], grads=[], zero_pre=0)
    for w, p in enumerate((p1, p2)):
        m = backward(p, sa, dq[:, w])
        assert m["abs_sum"] < sn.EXACT_LIMIT, (m["abs_sum"], sn.EXACT_LIMIT)
        for g in m["grads"] + m["deltas"]:
            assert np.array_equal(g.astype(np.float32).astype(np.int64), g)
        if n == sn.N_EXACT:
            assert m["zero_pre"] > 0
            assert 0.2 <= m["live"] <= 0.8, m["live"]
            assert all((g != 0).any() for g in m["grads"])
        out["zero_pre"] += m["zero_pre"]
        out["q"].append(m["q"])
        out["grads"].append([g.reshape(np.asarray(pp).shape).astype(np.float32) for g, pp in zip(m["grads"], p)])
    out["q"] = np.stack(out["q"], axis=1).astype(np.float32)
    _int[key] = out
    return out


# ------------------------------------------------------------------ the loss
def loss_model(q, target, weights, kind):
    """The loss of sac_pytorch.py:457-468 in binary64 on float32 q [n][2], target [n], weights [n] or
    None: dict of dq [n][2], td_abs [n], loss and their a-priori float32 bounds E_dq, E_td, E_loss
    (absolute).  With e = 2**-24, d = q - t rounded once (E_d = e |d|):
      L2: dq = ((2 w) d) / B: 2 w exact, a product, a division (taken at 2 e: one ulp), B exact:
          E_dq = |2 w| E_d / B + 3 e |dq|;  L1: dq = (w sign(d)) / B: E_dq = 2 e |dq| (sign(d) is
          exact: d rounds to 0 only when it is 0);
      td_abs = max |t - q|: one rounding each, E_td = e td_abs;
      the loss: per (row, net) term w d d (L2: E = 2 |w d| E_d + 2 e |term|) or w |d| (L1: E = |w| E_d +
          e |term|); a sum of N = 2 B non-negative terms in some fixed order: at most (N - 1) e times the
          sum; one or two divisions by B and an addition: 5 e |loss|."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(target, dtype=np.float64)[:, None]
    n = q.shape[0]
    w = np.ones((n, 1)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(n, 1)
    e, ab = EPS32, np.abs
    d = q - t
    E_d = e * ab(d)
    if kind == L2:
        dq = 2 * w * d / n
        E_dq = ab(2 * w) * E_d / n + 3 * e * ab(dq)
        term = w * d * d
        E_term = 2 * ab(w * d) * E_d + 2 * e * ab(term)
    else:
        dq = w * np.sign(d) / n
        E_dq = 2 * e * ab(dq)
        term = w * ab(d)
        E_term = ab(w) * E_d + e * ab(term)
    td_abs = ab(d).max(axis=1)
    total = term.sum()
    loss = total / n
    E_loss = (E_term.sum() + (2 * n - 1) * e * ab(term).sum()) / n + 5 * e * ab(loss)
    s = SECOND_ORDER
    return dict(dq=dq, td_abs=td_abs, loss=loss, E_dq=s * E_dq, E_td=s * e * td_abs, E_loss=s * E_loss)


# ------------------------------------------------------------------ clip, Adam, Polyak
ULP_DIV = ULP_SQRT = 1        # the device's float32 division and square root, taken at one ulp = 2 e


def adam_model(p, g, m, v, step, lr, beta1, beta2, eps, max_norm=0.0, partials=None, E_g=None, sum_terms=None,
               E_total_extra=0.0):
    """clip_grad_norm_, Adam.step (step: the count AFTER its increment) in binary64 on float32 tensors
    (lists of arrays) and constants rounded as the kernel receives them; partials: the float32 sums of
    squares the kernel is given; E_g: per tensor, an absolute error bound the gradients come with
    (default 0: exact inputs); sum_terms: the number of float32 additions behind the sum of the
    partials (default: their count) and E_total_extra an absolute error the norm comes with, for
    partials that are not exact inputs.  Returns dict of lists p, g (the scaled gradients), m, v with E_p, E_g,
    E_m, E_v, and norm, E_norm, coef.  First-order propagation with e = 2**-24 a rounding, a division
    and a square root 2 e:
      total = sqrt(sum of n partials)     E_total = (n - 1) e total / 2 + 2 e total
      s = total + 1e-6                    E_s = E_total + e s
      c = max_norm / s                    E_c = c E_s / s + 2 e c     (coef = min(1, c): exact when 1)
      g' = g c                            E_g' = c E_g + |g| E_c + e |g'|
      d = g' - m, pr = w1 d, m' = m + pr  E_m = w1 (E_g' + e |d|) + e |pr| + e |m'|
      v1 = v beta2, t1 = w2 g', t2 = t1 g', v' = v1 + t2
                                          E_v = e |v1| + (|g'| (w2 E_g' + e |t1|) + |t1| E_g' + e |t2|) + e |v'|
      r = sqrt(v')                        E_r = E_v / (2 r) + 2 e r   (r = 0 with E_v = 0: 0; else sqrt(E_v))
      dn = r / bc2s, den = dn + eps       E_den = E_r / bc2s + 2 e dn + e den
      u = m' / den                        E_u = E_m / den + |m'| E_den / den^2 + 2 e |u|
      s = step_size u, p' = p - s         E_p = step_size E_u + e |s| + e |p'|"""
    f32 = lambda x: float(np.float32(x))
    e, ab = EPS32, np.abs
    w1, w2, b2, epsf = f32(1.0 - beta1), f32(1.0 - beta2), f32(beta2), f32(eps)
    step_size, bc2s = f32(lr / (1 - beta1 ** step)), f32((1 - beta2 ** step) ** 0.5)
    out = dict(p=[], g=[], m=[], v=[], E_p=[], E_g=[], E_m=[], E_v=[], norm=None, E_norm=None, coef=1.0)
    c, E_c = 1.0, 0.0
    if max_norm > 0:
        parts = np.asarray(partials, dtype=np.float64)
        total = float(np.sqrt(parts.sum()))
        E_total = ((sum_terms or len(parts)) - 1) * e * total / 2 + 2 * e * total + E_total_extra
        s = total + f32(1e-6)
        E_s = E_total + e * s
        c = f32(max_norm) / s
        E_c = c * E_s / s + 2 * e * c
        if c >= 1.0 + E_c:
            c, E_c = 1.0, 0.0
        elif c > 1.0 - E_c:          # (too close to tell which side the float32 evaluation lands on)
            c, E_c = min(c, 1.0), 2 * E_c
        out.update(norm=total, E_norm=SECOND_ORDER * E_total, coef=c)
    for k in range(len(p)):
        pk, gk, mk, vk = (np.asarray(x[k], dtype=np.float64) for x in (p, g, m, v))
        Eg0 = 0.0 if E_g is None else E_g[k]
        g1 = gk * c
        Eg = c * Eg0 + ab(gk) * E_c + (e * ab(g1) if max_norm > 0 else 0.0)
        d = g1 - mk
        pr = w1 * d
        m1 = mk + pr
        E_m = w1 * (Eg + e * ab(d)) + e * ab(pr) + e * ab(m1)
        v1, t1 = vk * b2, w2 * g1
        t2 = t1 * g1
        vn = v1 + t2
        E_v = e * ab(v1) + (ab(g1) * (w2 * Eg + e * ab(t1)) + ab(t1) * Eg + e * ab(t2)) + e * ab(vn)
        r = np.sqrt(vn)
        with np.errstate(divide="ignore", invalid="ignore"):
            E_r = np.where(r > 0, np.minimum(E_v / (2 * r), np.sqrt(E_v)) + 2 * e * r, np.sqrt(E_v))
        dn = r / bc2s
        den = dn + epsf
        E_den = E_r / bc2s + 2 * e * dn + e * den
        u = m1 / den
        E_u = E_m / den + ab(m1) * E_den / den ** 2 + 2 * e * ab(u)
        s = step_size * u
        p1 = pk - s
        E_p = step_size * E_u + e * ab(s) + e * ab(p1)
        so = SECOND_ORDER
        for name, val in (("p", p1), ("g", g1), ("m", m1), ("v", vn), ("E_p", so * E_p), ("E_g", so * Eg),
                          ("E_m", so * E_m), ("E_v", so * E_v)):
            out[name].append(val)
    return out


def polyak_f32(t, p, tau):
    """torch's (1 - tau) * t + tau * p on float32 arrays: two rounded products and their rounded sum."""
    t, p = np.asarray(t, dtype=np.float32), np.asarray(p, dtype=np.float32)
    return np.float32(1.0 - tau) * t + np.float32(tau) * p


# ------------------------------------------------------------------ the real-valued case
def grad_case(S, A, H, L, n=sn.N_REAL):
    """The real-valued case of a shape: the critic of sac_td_nets.real_critic, rows [n][2S + A + 2]
    float32 (state | action first), target_q [n] and PER weights [n] in (0.2, 1]."""
    rng = np.random.default_rng([S, A, H, L, 23])
    W = 2 * S + A + 2
    rows = rng.uniform(-2, 2, (n, W)).astype(np.float32)
    rows[:, S:S + A] = rng.uniform(-1, 1, (n, A))
    target = rng.uniform(-2, 2, n).astype(np.float32)
    weights = rng.uniform(0.2, 1.0, n).astype(np.float32)
    return dict(S=S, A=A, H=H, L=L, n=n, critic=td.real_critic(S, A, H, L), rows=rows, target=target, weights=weights)


def full_backward(params_pair, sa, target, weights, kind):
    """The binary64 model of the whole gradient: q from the model's own forward pass, dq from the loss;
    (grads of q1 and q2 as one list in the parameters' order, terms: the largest sum of absolute terms
    of the batch reduction per tensor, q [n][2])."""
    n = sa.shape[0]
    qs = np.stack([td.q_forward(p, sa, dtype=np.float64)[0] for p in params_pair], axis=1)
    dq = loss_model(qs, target, weights, kind)["dq"]
    grads, terms = [], []
    for w, p in enumerate(params_pair):
        m = backward(p, sa, dq[:, w], dtype=np.float64)
        grads += [g.reshape(np.asarray(pp).shape) for g, pp in zip(m["grads"], p)]
        terms += [float(t) for t in m["terms"]]
    return grads, terms, qs
