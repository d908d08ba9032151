"""Inputs and NumPy models for the tests of pd_sac_critic_dinput, pd_sac_actor_grad and
pdenv.sac.ActorUpdate (plain NumPy; no GPU, no torch at import).  Builds on sac_nets.py,
sac_td_nets.py and sac_grad_nets.py.

`actor_backward` is the actor's backward pass from a given dLoss / d(mean | raw log_std) and
`q_dinput` the gradient of one Q net with respect to its input under unit upstream gradient, in int64
(the integer fixtures: the reference the kernels must EQUAL) or binary64.  `elem` is the elementwise
chain of the actor step in binary64 -- the sample, the log-probability, the loss coefficients, the
sample's backward and the three losses -- from given heads, eps, q and dq/da, `elem_bound` its
a-priori float32 error bound, `full` the whole block (sac_pytorch.py:486-497, 512-520) in binary64,
and `np_eps` the kernel's eps draws (Philox tag 72).

The bound of `elem` (e = 2**-24 one float32 rounding, a division 2 e, expf / logf / tanhf at
sac_td_nets' ulp counts; heads m | raw, eps, q, dq/da, w, log_alpha and target_entropy are float32
inputs, exact in the model; everything evaluated on the model's own values, times 1.01 for the
products of errors; nothing comes from the kernel's output).  The forward part, up to a, log_prob
and alpha, is sac_td_nets.chain_bound's.  Then, per row and component, Bf exact:
    wb = w / Bf                       E_wb = 2 e |wb|
    c_j = -(wb sel_j)                 E_cj = sel_j E_wb            (sel_j in {0, 1/2, 1}: exact products;
                                                                    sel_j is decided by float32 inputs)
    wa = w alpha, cl = wa / Bf        E_cl = (|w| E_alpha + e |wa|) / Bf + 2 e |cl|
    p_j = c_j dq_j, G = p_1 + p_2     E_G = sum_j (|dq_j| E_cj + e |p_j|) + e |G|
    a2 = a a, t = 1 - a2              E_t = 2 |a| E_a + e a2 + e |t|
    u1 = G max_action, u2 = u1 t      E_u2 = |t| (max_action E_G + e |u1|) + |u1| E_t + e |u2|
    v2 = (2 a) t                      E_v2 = 2 |t| E_a + 2 |a| E_t + e |v2|
    den = t + 1e-6, v3 = v2 / den     E_v3 = E_v2 / den + |v2| (E_t + e den) / den^2 + 2 e |v3|
    v4 = cl v3, gx = u2 + v4          E_gx = E_u2 + |v3| E_cl + |cl| E_v3 + e |v4| + e |gx|
    dmean = gx
    r1 = gx sd, r2 = r1 eps           E_r2 = |eps| (sd E_gx + |gx| E_sd + e |r1|) + e |r2|
    draw = r2 - cl inside the clamp   E_draw = E_r2 + E_cl + e |draw|   (0 outside: the test is on raw, exact)
Near saturation den is as small as 1e-6 and E_t about e, so E_v3 / |v3| grows to a few per cent: that
is the conditioning of the reference's own expression 2 a (1 - a^2) / (1 - a^2 + 1e-6), not slack.
The losses:
    la = w (alpha lp - min q)         E_la = |w| (|lp| E_alpha + alpha E_lp + e |alpha lp| + e |d|) + e |la|
    lt = w (lp + te)                  E_lt = |w| (E_lp + e |lp + te|) + e |lt|
    a float32 sum of B terms in any order: sum of the terms' bounds + (B - 1) e sum |terms|
    actor_loss = S_la / Bf            + 2 e |actor_loss|
    log_alpha_grad = -(S_lt / Bf)     + 2 e |log_alpha_grad|
    alpha_loss = log_alpha times it   E = |log_alpha| E_grad + e |alpha_loss|"""
import numpy as np

import sac_grad_nets as gn
import sac_nets as sn
import sac_td_nets as td

SHAPES = gn.SHAPES_N + gn.SHAPES_DEEP
SHAPES_WIDE = [(16, 8, 128, 2), (12, 5, 256, 2), (16, 8, 512, 2)]   # S + A above 16: the actor alone (dheads_in, no critic)
BATCHES = gn.BATCHES
EPS32 = td.EPS32
SECOND_ORDER = td.SECOND_ORDER
TAG_ACT_EPS = 72


def n_partials(H, L):
    return H // 64 + (L - 1) * (H // 16) * (H // 128) + H // 128


def scratch_bytes(n, A, H, L):
    """pd_sac_actor_grad_scratch_bytes' closed form."""
    if n <= 0 or A <= 0 or H <= 0 or L <= 0:
        return 0
    bp = (n + 15) // 16 * 16
    return 4 * (bp * (2 * L * H + 5 * A + 19) + bp // 8)


# ------------------------------------------------------------------ the backward passes
def actor_backward(params, obs, dheads, dtype=np.int64):
    """The actor (pd_sac_actor's parameter order) on obs [n][S] with the upstream gradient dheads
    [n][2A] = dLoss / d(mean | raw log_std): dict of heads [n][2A], grads (the parameters' order), h,
    deltas, abs_sum (the largest sum of absolute terms of any sum formed: forward, deltas, gradient
    entries), terms (per gradient tensor) and zero_pre, live as sac_grad_nets.backward."""
    ps = [np.asarray(p).astype(dtype) for p in params]
    L = len(ps) // 2 - 2
    x = np.asarray(obs).astype(dtype)
    dh = np.asarray(dheads).astype(dtype)
    A = dh.shape[1] // 2
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
    wh = np.concatenate([ps[2 * L], ps[2 * L + 2]], axis=0)              # [2A][H]
    bh = np.concatenate([ps[2 * L + 1], ps[2 * L + 3]], axis=0)
    abs_sum = max(abs_sum, (ab(h) @ ab(wh).T + ab(bh)).max())
    heads = h @ wh.T + bh
    grads = [None] * (2 * (L + 2))
    terms = [None] * (2 * (L + 2))

    def put(k, value, t):
        grads[k], terms[k] = value, t.max() if t.size else 0

    gw, tw = dh.T @ hs[-1], ab(dh).T @ ab(hs[-1])
    gb, tb = dh.sum(axis=0), ab(dh).sum(axis=0)
    put(2 * L, gw[:A], tw[:A]); put(2 * L + 1, gb[:A], tb[:A])
    put(2 * L + 2, gw[A:], tw[A:]); put(2 * L + 3, gb[A:], tb[A:])
    abs_sum = max(abs_sum, (ab(dh) @ ab(wh)).max())
    delta = (dh @ wh) * (hs[-1] > 0)
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
    return dict(heads=heads, grads=grads, h=hs, deltas=deltas, abs_sum=abs_sum, terms=terms, zero_pre=zero_pre,
                live=float((hs[-1] > 0).mean()))


def q_dinput(params, sa, dtype=np.int64):
    """One Q net (pd_sac_critic's parameter order) on sa [n][D]: (q [n], dsa [n][D] = d q / d input
    with unit upstream gradient, abs_sum of every sum formed)."""
    m = gn.backward(params, sa, np.ones(len(sa)), dtype=dtype)
    W1 = np.asarray(params[0]).astype(dtype)
    d0 = m["deltas"][0]
    abs_sum = max(m["abs_sum"], (np.abs(d0) @ np.abs(W1)).max())
    return m["q"], d0 @ W1, abs_sum


# ------------------------------------------------------------------ the integer fixtures
def int_dheads(n, A, seed=0):
    """[n][2A] integer upstream gradients in [-1, 1] (zeros among them), float32."""
    return np.random.default_rng([seed, n, A, 9]).integers(-1, 2, (n, 2 * A)).astype(np.float32)


_int_actor, _int_q = {}, {}


def int_actor_case(S, A, H, L, n=sn.N_EXACT):
    """The actor's integer fixture over the first n of 37 rows (once per (shape, n)): dict of params,
    obs [n][S], dheads [n][2A], heads [n][2A] and grads as float32, the conditions asserted on the
    int64 model: every sum of absolute terms below 2**24, every value a float32 integer, and at n = 37
    a live share in [0.2, 0.8] and no all-zero gradient tensor."""
    key = (S, A, H, L, n)
    if key not in _int_actor:
        params = sn.int_actor(S, A, H, L)
        obs = sn.int_obs(sn.N_EXACT, S)[:n]
        dh = int_dheads(sn.N_EXACT, A)[:n]
        m = actor_backward(params, obs, dh)
        assert m["abs_sum"] < sn.EXACT_LIMIT, (key, m["abs_sum"], sn.EXACT_LIMIT)
        for g in m["grads"] + m["deltas"]:
            assert np.array_equal(g.astype(np.float32).astype(np.int64), g)
        if n == sn.N_EXACT:
            assert 0.2 <= m["live"] <= 0.8, (key, m["live"])
            assert all((g != 0).any() for g in m["grads"]), key
        _int_actor[key] = dict(params=params, obs=np.ascontiguousarray(obs), dheads=np.ascontiguousarray(dh),
                               heads=m["heads"].astype(np.float32), zero_pre=m["zero_pre"],
                               grads=[g.reshape(np.asarray(p).shape).astype(np.float32)
                                      for g, p in zip(m["grads"], params)])
    return _int_actor[key]


def int_dinput_case(S, A, H, L, n=sn.N_EXACT):
    """The Q nets' integer fixture (sac_td_nets.int_critic_case's twin critic and rows): dict of params
    (q1, q2), sa [n][S + A], q [n][2], dsa [n][2][S + A] as float32, every sum below 2**24 asserted."""
    key = (S, A, H, L, n)
    if key not in _int_q:
        p1, p2, states, actions, _ = td.int_critic_case(S, A, H, L)
        sa = np.concatenate([states, actions], axis=1)[:n]
        qs, ds = [], []
        for p in (p1, p2):
            q, dsa, abs_sum = q_dinput(p, sa)
            assert abs_sum < sn.EXACT_LIMIT, (key, abs_sum)
            assert np.array_equal(dsa.astype(np.float32).astype(np.int64), dsa)
            qs.append(q); ds.append(dsa)
        dsa = np.stack(ds, axis=1).astype(np.float32)
        if n == sn.N_EXACT:
            assert (dsa != 0).any(axis=(0, 1)).all(), key          # every input column has a gradient somewhere
        _int_q[key] = dict(params=(p1, p2), sa=np.ascontiguousarray(sa), q=np.stack(qs, axis=1).astype(np.float32), dsa=dsa)
    return _int_q[key]


# ------------------------------------------------------------------ the elementwise chain
def elem(heads, eps, q, dqda, weights, lo, hi, max_action, log_alpha, target_entropy):
    """The actor step's elementwise chain in binary64 from float32 inputs: heads [n][2A] (mean | raw
    log_std), eps [n][A], q [n][2], dqda [n][2][A], weights [n] or None.  dict of new_actions, log_prob,
    dheads [n][2A] (dmean | draw), actor_loss, log_alpha_grad, alpha_loss and the intermediate values
    elem_bound reads."""
    heads, eps, q, dqda = (np.asarray(x, dtype=np.float64) for x in (heads, eps, q, dqda))
    n, A = eps.shape
    f32 = lambda v: float(np.float32(v))
    c = td.chain(heads, eps, q, np.zeros((n, A + 4)), 1, A, lo, hi, max_action, log_alpha, 0.0)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(n)
    raw = heads[:, A:]
    inside = (raw >= f32(lo)) & (raw <= f32(hi))
    q1, q2 = q[:, 0], q[:, 1]
    sel = np.stack([np.where(q1 < q2, 1.0, np.where(q1 > q2, 0.0, 0.5)),
                    np.where(q2 < q1, 1.0, np.where(q2 > q1, 0.0, 0.5))], axis=1)       # [n][2]
    alpha, ma, la, te = c["alpha"], f32(max_action), f32(log_alpha), f32(target_entropy)
    wb = w / n
    cj = -(wb[:, None] * sel)
    cl = (w * alpha / n)[:, None]
    pj = cj[:, :, None] * dqda
    G = pj.sum(axis=1)
    a = c["a"]
    t = 1 - a * a
    u1 = G * ma
    u2 = u1 * t
    v2 = 2 * a * t
    den = t + td.TANH_EPS
    v3 = v2 / den
    v4 = cl * v3
    gx = u2 + v4
    r1 = gx * c["sd"]
    r2 = r1 * eps
    draw = np.where(inside, r2 - cl, 0.0)
    lp = c["next_log_prob"]
    mq = np.minimum(q1, q2)
    la_terms = w * (alpha * lp - mq)
    lt_terms = w * (lp + te)
    ga = -(lt_terms.sum() / n)
    return dict(c=c, new_actions=c["next_actions"], log_prob=lp, dheads=np.concatenate([gx, draw], axis=1),
                actor_loss=la_terms.sum() / n, log_alpha_grad=ga, alpha_loss=la * ga, w=w, n=n, sel=sel, wb=wb, cj=cj, cl=cl,
                pj=pj, G=G, t=t, u1=u1, u2=u2, v2=v2, den=den, v3=v3, v4=v4, gx=gx, r1=r1, r2=r2, draw=draw,
                inside=inside, dqda=dqda, la_terms=la_terms, lt_terms=lt_terms, mq=mq, max_action=ma, log_alpha=la,
                target_entropy=te, alpha=alpha)


def elem_bound(m):
    """Absolute float32 error bounds of elem's results on its own values m (the module docstring):
    dict of new_actions [n][A], log_prob [n], dheads [n][2A], actor_loss, log_alpha_grad, alpha_loss."""
    e, ab = EPS32, np.abs
    c = m["c"]
    E_act, E_lp, _ = (x / SECOND_ORDER for x in td.chain_bound(c))
    E_sd = 2 * td.ULP_EXP * e * c["sd"]
    E_x = ab(c["eps"]) * E_sd + e * ab(c["p"]) + e * ab(c["x"])
    a = c["a"]
    E_a = (1 - a ** 2) * E_x + 2 * td.ULP_TANH * e * ab(a)
    E_alpha = 2 * td.ULP_EXP * e * m["alpha"]
    n, w = m["n"], m["w"]
    E_wb = 2 * e * ab(m["wb"])
    E_cj = m["sel"] * E_wb[:, None]
    wa = w * m["alpha"]
    E_cl = ((ab(w) * E_alpha + e * ab(wa)) / n)[:, None] + 2 * e * ab(m["cl"])
    E_G = (ab(m["dqda"]) * E_cj[:, :, None] + e * ab(m["pj"])).sum(axis=1) + e * ab(m["G"])
    t = m["t"]
    E_t = 2 * ab(a) * E_a + e * a * a + e * ab(t)
    E_u2 = ab(t) * (m["max_action"] * E_G + e * ab(m["u1"])) + ab(m["u1"]) * E_t + e * ab(m["u2"])
    E_v2 = 2 * ab(t) * E_a + 2 * ab(a) * E_t + e * ab(m["v2"])
    den = m["den"]
    E_v3 = E_v2 / den + ab(m["v2"]) * (E_t + e * den) / den ** 2 + 2 * e * ab(m["v3"])
    E_gx = E_u2 + ab(m["v3"]) * E_cl + ab(m["cl"]) * E_v3 + e * ab(m["v4"]) + e * ab(m["gx"])
    E_r2 = ab(c["eps"]) * (c["sd"] * E_gx + ab(m["gx"]) * E_sd + e * ab(m["r1"])) + e * ab(m["r2"])
    E_draw = np.where(m["inside"], E_r2 + E_cl + e * ab(m["draw"]), 0.0)
    lp = m["log_prob"]
    pr = m["alpha"] * lp
    E_la = ab(w) * (ab(lp) * E_alpha + m["alpha"] * E_lp + e * ab(pr) + e * ab(pr - m["mq"])) + e * ab(m["la_terms"])
    E_lt = ab(w) * (E_lp + e * ab(lp + m["target_entropy"])) + e * ab(m["lt_terms"])
    E_aloss = (E_la.sum() + (n - 1) * e * ab(m["la_terms"]).sum()) / n + 2 * e * abs(m["actor_loss"])
    E_ga = (E_lt.sum() + (n - 1) * e * ab(m["lt_terms"]).sum()) / n + 2 * e * abs(m["log_alpha_grad"])
    E_alphaloss = abs(m["log_alpha"]) * E_ga + e * abs(m["alpha_loss"])
    s = SECOND_ORDER
    return dict(new_actions=s * E_act, log_prob=s * E_lp, dheads=s * np.concatenate([E_gx, E_draw], axis=1),
                actor_loss=s * E_aloss, log_alpha_grad=s * E_ga, alpha_loss=s * E_alphaloss)


# ------------------------------------------------------------------ the whole block
def full(actor_params, critic_params, states, eps, weights, lo, hi, max_action, log_alpha, target_entropy):
    """The whole actor step in binary64 on float32 parameters and inputs: the actor's forward pass, the
    sample, the twin critic on state | new_action, its input gradients, elem and the actor's backward
    pass.  dict of elem's entries plus heads, q [n][2], dqda [n][2][A], grads (pd_sac_actor's order),
    terms (per gradient tensor, the largest sum of absolute terms of its batch reduction), and the
    a-priori float32 forward bounds E_heads [n][2A] and E_q [n][2] (forward_bound: the unit the
    real-valued fixture's margins are measured in; E_q takes new_action as an exact input)."""
    states = np.asarray(states, dtype=np.float64)
    n, S = states.shape
    A = np.asarray(eps).shape[1]
    heads, _, _ = sn.forward(actor_params, states, dtype=np.float64)
    zero_q, zero_d = np.zeros((n, 2)), np.zeros((n, 2, A))
    m0 = elem(heads, eps, zero_q, zero_d, weights, lo, hi, max_action, log_alpha, target_entropy)
    sa = np.concatenate([states, m0["new_actions"]], axis=1)
    qs, ds = [], []
    for p in critic_params:
        q, dsa, _ = q_dinput(p, sa, dtype=np.float64)
        qs.append(q); ds.append(dsa[:, S:])
    q, dqda = np.stack(qs, axis=1), np.stack(ds, axis=1)
    m = elem(heads, eps, q, dqda, weights, lo, hi, max_action, log_alpha, target_entropy)
    b = actor_backward(actor_params, states, m["dheads"], dtype=np.float64)
    m.update(heads=heads, q=q, dqda=dqda, grads=[g.reshape(np.asarray(p).shape) for g, p in zip(b["grads"], actor_params)],
             terms=[float(t) for t in b["terms"]], E_heads=forward_bound(actor_params, states, 2),
             E_q=np.stack([forward_bound(p, sa, 1)[:, 0] for p in critic_params], axis=1))
    return m


def forward_bound(params, x, n_heads):
    """The a-priori float32 error bound of every output of an MLP's forward pass on x [n][in], from the
    binary64 model's sums of absolute terms, to first order.  A dot product of k terms and a bias added
    in float32 in any order (fma or not) errs by at most eps_l[j] = (k + 1) e (|W_l| |h_{l-1}| + |b_l|)[j]
    at unit j of layer l, given exact inputs.  Such an error reaches output o through the model's own
    Jacobian J_l[o][j] = d out_o / d pre-activation_j (the product of the layers above with their ReLU
    masks, cancellation included; the masks are taken as the model's, which is what first order means),
    so every local error taken at its bound and with the worst sign:
        E[o] = eps_head[o] + sum_l sum_j |J_l[o][j]| eps_l[j].
    [n][outputs]; n_heads: 2 (an actor: mean and log_std heads on the last hidden layer) or 1 (a Q net)."""
    ps = [np.asarray(p, dtype=np.float64) for p in params]
    L = len(ps) // 2 - n_heads
    h = np.asarray(x, dtype=np.float64)
    ab = np.abs
    local, masks = [], []
    for l in range(L):
        W, b = ps[2 * l], ps[2 * l + 1]
        local.append((W.shape[1] + 1) * EPS32 * (ab(h) @ ab(W).T + ab(b)))
        h = np.maximum(h @ W.T + b, 0)
        masks.append(h > 0)
    wh = np.concatenate([ps[2 * (L + k)] for k in range(n_heads)], axis=0)          # [out][H]
    bh = np.concatenate([ps[2 * (L + k) + 1] for k in range(n_heads)], axis=0)
    E = (wh.shape[1] + 1) * EPS32 * (ab(h) @ ab(wh).T + ab(bh))
    J = np.broadcast_to(wh, (h.shape[0],) + wh.shape)                                # [n][out][H]
    for l in range(L - 1, -1, -1):
        J = J * masks[l][:, None, :]
        E = E + np.einsum("noj,nj->no", ab(J), local[l])
        if l > 0:
            J = J @ ps[2 * l]
    return SECOND_ORDER * E


# ------------------------------------------------------------------ eps
def np_eps(seed, draw, n, A):
    """pd_sac_actor_grad's eps draws [n][A] in NumPy: sac_td_nets.np_eps with the tag 72."""
    import philox_np as ph
    pairs = (A + 1) // 2
    i = np.repeat(np.arange(n, dtype=np.uint64), pairs)
    tag = np.tile(TAG_ACT_EPS + np.arange(pairs, dtype=np.uint64), n)
    d0 = np.full_like(i, draw & 0xFFFFFFFF)
    d1 = np.full_like(i, (draw >> 32) & 0xFFFFFFFF)
    x, y, z, w = ph.philox(i, d0, d1, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1, u2 = 1.0 - ph.u01(x, y), ph.u01(z, w)
    rho = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    zz = np.stack([rho * np.cos(ang), rho * np.sin(ang)], axis=1).reshape(n, 2 * pairs)
    return zz[:, :A]         # binary64: the caller casts


# ------------------------------------------------------------------ the real-valued case
MARGIN = 16              # a kept row's |q1 - q2| and clamp distances, in a-priori forward bounds
MAX_DROPPED = 0.10       # ceil(n / 0.9) candidates are drawn (290 for 261 rows): the first n that keep the margins are the case
LOG_ALPHA = -1.0


def real_case(S, A, H, L, n=sn.N_REAL):
    """The real-valued case of a shape (once per shape): sac_td_nets.td_case's actor (clamp (-5, -1))
    and critic, ceil(n / 0.9) candidate rows [.][2S + A + 2] (states U(-2, 2)), eps, PER weights in (0.2,
    1], of which the first n rows at which the loss is differentiable with margin are kept: the
    binary64 |q1 - q2| at least MARGIN times the a-priori float32 forward bound of q, and the raw
    log_std at least MARGIN times the heads' bound from each clamp bound.  dict with the kept rows,
    eps, weights, the binary64 model `ref` on them, dropped (the share of candidates examined that were
    dropped) and the clamped / unclamped counts."""
    key = (S, A, H, L, n)
    if key in _real:
        return _real[key]
    import copy
    import torch
    base = td.td_case(S, A, H, L, n=8)
    actor, critic = copy.deepcopy(base["actor"]), copy.deepcopy(base["critic"])
    rng = np.random.default_rng([S, A, H, L, 31])
    W = 2 * S + A + 2
    n_cand = int(np.ceil(n / (1 - MAX_DROPPED)))
    rows = rng.uniform(-2, 2, (n_cand, W)).astype(np.float32)
    eps = rng.standard_normal((n_cand, A)).astype(np.float32)
    weights = rng.uniform(0.2, 1.0, n_cand).astype(np.float32)
    # the log_std head's bias is moved so that the upper clamp bound sits in the widest gap between two
    # neighbouring values of the candidates' raw log_std in their upper tail (the 85th to 97th
    # percentile): some components are clamped, most are not, and as few rows as the draw allows stand
    # within the margin of the bound; for the same reason Q2's output bias is moved so that the
    # candidates' q1 - q2 has its mean two standard deviations below zero: either net is still the
    # smaller one on a share of the rows
    raw0 = sn.forward(sn.actor_params(actor), rows[:, :S], dtype=np.float64)[0][:, A:]
    v = np.sort(raw0.ravel())
    i0, i1 = int(0.85 * len(v)), int(0.97 * len(v))
    i = i0 + int(np.argmax(np.diff(v[i0:i1 + 1])))
    with torch.no_grad():
        actor.log_std.bias += float(td.LOG_STD_MAX - 0.5 * (v[i] + v[i + 1]))
    m0 = full(sn.actor_params(actor), td.critic_params(critic), rows[:, :S], eps, weights, td.LOG_STD_MIN, td.LOG_STD_MAX,
              actor.max_action, LOG_ALPHA, -float(A))
    with torch.no_grad():
        dq0 = m0["q"][:, 0] - m0["q"][:, 1]
        critic.q2[-1].bias += float(dq0.mean() + 2.0 * dq0.std())
    ap, cp = sn.actor_params(actor), td.critic_params(critic)
    lo, hi = td.LOG_STD_MIN, td.LOG_STD_MAX
    m = full(ap, cp, rows[:, :S], eps, weights, lo, hi, actor.max_action, LOG_ALPHA, -float(A))
    eq = m["E_q"].max(axis=1)
    eh = m["E_heads"][:, A:]
    raw = m["heads"][:, A:]
    ok = (np.abs(m["q"][:, 0] - m["q"][:, 1]) >= MARGIN * eq) \
        & (np.minimum(np.abs(raw - lo), np.abs(raw - hi)) >= MARGIN * eh).all(axis=1)
    keep = np.flatnonzero(ok)[:n]
    assert len(keep) == n, (key, int(ok.sum()))
    examined = keep[-1] + 1
    rows, eps, weights = (np.ascontiguousarray(x[keep]) for x in (rows, eps, weights))
    ref = full(ap, cp, rows[:, :S], eps, weights, lo, hi, actor.max_action, LOG_ALPHA, -float(A))
    inside = ref["inside"]
    _real[key] = dict(S=S, A=A, H=H, L=L, n=n, actor=actor, critic=critic, rows=rows, eps=eps, weights=weights, ref=ref,
                      dropped=float(examined - n) / examined, clamped=int((~inside).sum()), unclamped=int(inside.sum()),
                      q1_smaller=int((ref["q"][:, 0] < ref["q"][:, 1]).sum()), q2_smaller=int((ref["q"][:, 1] < ref["q"][:, 0]).sum()),
                      log_alpha=LOG_ALPHA, target_entropy=-float(A))
    return _real[key]


_real = {}


# ------------------------------------------------------------------ the reference lines in torch
def torch_block(actor, critic, states, eps, weights, log_alpha, target_entropy):
    """sac_pytorch.py:486-497 and :512-520 with Actor.sample written out on a given eps, in the
    tensors' dtype and on their device (weights [n] or None; log_alpha a one-element tensor): dict of
    grads (the actor's, pd_sac_actor's order, float64 NumPy), log_alpha_grad, actor_loss, alpha_loss,
    new_actions, log_prob [n], q [n][2] (NumPy)."""
    import torch
    import torch.nn as nn
    n = states.shape[0]
    w = None if weights is None else weights.reshape(n, 1)
    la = log_alpha.detach().clone().requires_grad_(True)
    actor.zero_grad()
    mean, log_std = actor(states)
    std = log_std.exp()
    x = mean + std * eps
    action = torch.tanh(x)
    log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727
                - torch.log(1 - action.pow(2) + 1e-6)).sum(-1, keepdim=True)
    new_actions = action * actor.max_action
    q1, q2 = critic(states, new_actions)
    q = torch.min(q1, q2)
    alpha = la.detach().exp()
    actor_loss = (alpha * log_prob - q).mean() if w is None else (w * (alpha * log_prob - q)).mean()
    actor_loss.backward()
    t = (log_prob + target_entropy).detach()
    alpha_loss = -(la * t).mean() if w is None else -(la * w * t).mean()
    alpha_loss.backward()
    lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)] + [actor.mean, actor.log_std]
    f = lambda v: v.detach().cpu().numpy().astype(np.float64)
    return dict(grads=[f(t.grad) for m in lins for t in (m.weight, m.bias)], log_alpha_grad=float(la.grad.reshape(-1)[0]),
                actor_loss=float(actor_loss.detach()), alpha_loss=float(alpha_loss.detach()), new_actions=f(new_actions),
                log_prob=f(log_prob)[:, 0], q=f(torch.cat([q1, q2], dim=1)))
