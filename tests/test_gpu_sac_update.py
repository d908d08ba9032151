"""pd_sac_critic_grad and pd_adam_step (csrc/pdsacupd.hip) and pdenv.sac.CriticUpdate against
references outside the kernels.

1. The gradients exactly: integer nets, integer state | action and integer dq_in
   (sac_grad_nets.int_grad_case: every partial sum an integer below 2**24); every gradient tensor of
   both nets must EQUAL the int64 backward pass and q must equal pd_sac_critic's.
2. The loss gradient: dq_out, td_abs and loss_out of the four loss kinds against a binary64 model on
   the kernel's own q, under an a-priori bound.
3. The whole gradient, real-valued, against binary64 autograd: no worse than REAL_C times torch's
   own float32 autograd.
4. Determinism: equal bits twice, rows independent of the batch, outputs independent of which
   optional outputs are asked for.
5. pd_adam_step against a binary64 clip + Adam under an a-priori bound; Polyak exactly.
6. CriticUpdate end to end on a real torch.optim.Adam; the torch fallback.

The bound of test 2 (sac_grad_nets.loss_model).  q, target and weights are float32 numbers, exact in
the model; e = 2**-24 is one float32 rounding (relative), a float32 division is taken at one ulp = 2 e.
    d = q - t                      E_d = e |d|
    L2: dq = ((2 w) d) / B         E_dq = |2 w| E_d / B + 3 e |dq|   (2 w and B are exact)
    L1: dq = (w sign(d)) / B       E_dq = 2 e |dq|                   (sign(d) is exact, sign(0) = 0)
    td_abs = max(|t - q1|, |t - q2|)   E_td = e td_abs
    loss = (sum over rows and nets of w d d, or of w |d|) / B:
        a term: E = 2 |w d| E_d + 2 e |term| (L2), |w| E_d + e |term| (L1); a float32 sum of N = 2 B
        non-negative terms in any order: (N - 1) e sum; the divisions by B and the last addition: 5 e |loss|
each evaluated on the model's values, times 1.01 for the products of errors.

The bound of test 5 (sac_grad_nets.adam_model), the same way, a division and a square root at 2 e:
    total = sqrt(sum of n partials)    E_total = (n - 1) e total / 2 + 2 e total   (the partials are inputs)
    s = total + 1e-6, c = max_norm / s E_c = c (E_total + e s) / s + 2 e c          (coef = min(1, c))
    g' = g c                           E_g' = |g| E_c + e |g'|                      (0 without clipping)
    d = g' - m, pr = w1 d, m' = m + pr E_m = w1 (E_g' + e |d|) + e |pr| + e |m'|
    v1 = v beta2, t1 = w2 g', t2 = t1 g', v' = v1 + t2
                                       E_v = e |v1| + |g'| (w2 E_g' + e |t1|) + |t1| E_g' + e |t2| + e |v'|
    r = sqrt(v')                       E_r = E_v / (2 r) + 2 e r
    dn = r / bc2s, den = dn + eps      E_den = E_r / bc2s + 2 e dn + e den
    u = m' / den                       E_u = E_m / den + |m'| E_den / den^2 + 2 e |u|
    p' = p - step_size u               E_p = step_size E_u + e |step_size u| + e |p'|
with w1 = fl(1 - beta1), w2 = fl(1 - beta2), step_size and bc2s the float32 numbers the kernel receives.
Nothing in either bound comes from the kernel's output.

The bound of test 3: for every parameter tensor, max |grad - autograd64| <= max(REAL_C err_torch, floor),
err_torch the larger of torch's float32 autograd errors on the GPU and on the CPU against the same
binary64 result, floor = B 2**-24 max over the tensor's entries of sum_b |terms| of the binary64 model
(B terms added in float32 in any order), for tensors where torch's error happens to be zero.

Test 6 checks each of five consecutive updates against the torch block in float64 run on a deep copy
of the state the update started from, with test 3's bound as the gradient's error carried through
test 5's propagation.  That is the statement about a single float64 trajectory as well: the
distance of the kernel's state from a float64 copy that never looks at it again is at most this
per-update bound plus the distance two float64 updates started from the two states end at, which is
a property of the float64 block alone.

Measured (MI355X, `python tests/test_gpu_sac_update.py OUT.json`): profiles/sac_critic_update_shapes.json."""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import sac_grad_nets as gn
import sac_nets as sn
import sac_td_nets as td

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5     # no integer: no gradient of an integer net equals it
GUARD = 16
REAL_C = 4.0            # tests/test_gpu_sac_actor.py: one summation order against another
vp = C.c_void_p


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(x, y):
    import torch
    return torch.equal(bits(x), bits(y))


def ptr_list(ts):
    return (vp * len(ts))(*[t.data_ptr() for t in ts])


def n_partials(H, L):
    return 2 * (H // 64 + (L - 1) * (H // 16) * (H // 128) + H // 128)


def run_grad(params, sa, n, S, A, H, L, target=None, weights=None, kind=gn.L2, dq_in=None,
             outs=("q", "td_abs", "dq_out", "loss", "partials"), pitch=None):
    """One pd_sac_critic_grad call over the first n rows of sa [>= n][pitch] (device).  params: the two
    nets' device tensors.  Every gradient tensor is a fresh buffer of numel + 16 floats filled with the
    sentinel; the outputs asked for are sentinel-filled with 16 guard rows.  Returns dict of grads (two
    lists of flat views), grad_guards, the outputs (views of n rows) and out_guards."""
    import torch
    from pdenv import _lib
    lib = _lib.load()
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    gbufs = [[full(p.numel() + GUARD) for p in ps] for ps in params]
    has_t = target is not None
    o = dict(q=full(n + GUARD, 2) if "q" in outs else None,
             td_abs=full(n + GUARD) if "td_abs" in outs and has_t else None,
             dq_out=full(n + GUARD, 2) if "dq_out" in outs else None,
             loss=full(1 + GUARD) if "loss" in outs and has_t else None,
             partials=full(n_partials(H, L) + GUARD) if "partials" in outs else None)
    nbytes = int(lib.pd_sac_critic_grad_scratch_bytes(n, H, L))
    scratch = torch.empty(nbytes // 4 + GUARD, device="cuda")
    scratch[nbytes // 4:] = SENTINEL
    cnt = C.c_int32(n_partials(H, L))
    P = lambda t: None if t is None else vp(t.data_ptr())
    st = lib.pd_sac_critic_grad(n, S, A, H, L, P(sa), int(sa.stride(0)) if pitch is None else pitch, P(target),
                                P(weights), kind, P(dq_in), ptr_list(params[0]), ptr_list(params[1]),
                                ptr_list(gbufs[0]), ptr_list(gbufs[1]), P(o["q"]), P(o["td_abs"]), P(o["dq_out"]),
                                P(o["loss"]), P(o["partials"]), C.byref(cnt), vp(scratch.data_ptr()), nbytes, None)
    assert st == _lib.PD_OK, lib.pd_last_error()
    torch.cuda.synchronize()
    assert cnt.value == n_partials(H, L)
    assert bool((scratch[nbytes // 4:] == SENTINEL).all()), "scratch written past its closed form"
    res = dict(grads=[[b[:p.numel()] for b, p in zip(bs, ps)] for bs, ps in zip(gbufs, params)],
               grad_guards=[[b[p.numel():] for b, p in zip(bs, ps)] for bs, ps in zip(gbufs, params)])
    lens = dict(q=n, td_abs=n, dq_out=n, loss=1, partials=n_partials(H, L))
    for k, t in o.items():
        res[k] = None if t is None else t[:lens[k]]
        if t is not None:
            assert bool((t[lens[k]:] == SENTINEL).all()), f"{k}: written past its end"
    for w in range(2):
        for k, g in enumerate(res["grad_guards"][w]):
            assert bool((g == SENTINEL).all()), f"net {w} tensor {k}: guard floats after the gradient were written"
    return res


# ------------------------------------------------------------------ 1. the gradients, exact
_int_dev = {}


def int_dev(S, A, H, L):
    """The integer fixture's device side (once per shape): the two nets' parameter tensors, state |
    action in a [37 + 16][S + A] buffer whose last 16 rows are NaN, dq the same way, and a
    CriticKernel's q [37][2] on the same rows."""
    import torch
    from pdenv.sac import Critic, CriticKernel
    key = (S, A, H, L)
    if key not in _int_dev:
        c = gn.int_grad_case(S, A, H, L)
        params = [[torch.from_numpy(np.asarray(p)).cuda() for p in ps] for ps in c["params"]]
        n = sn.N_EXACT
        sa = torch.full((n + GUARD, S + A), float("nan"), device="cuda")
        sa[:n] = torch.from_numpy(c["sa"]).cuda()
        dq = torch.full((n + GUARD, 2), float("nan"), device="cuda")
        dq[:n] = torch.from_numpy(c["dq"]).cuda()
        critic = td.load_critic(Critic(S, A, hidden_dim=H, n_hidden_layers=L), *c["params"]).cuda()
        qk = torch.full((n, 2), float("nan"), device="cuda")
        CriticKernel(critic)(sa[:n, :S].contiguous(), sa[:n, S:].contiguous(), qk)
        torch.cuda.synchronize()
        _int_dev[key] = (params, sa, dq, qk)
    return _int_dev[key]


def check_exact(S, A, H, L, n):
    import torch
    c = gn.int_grad_case(S, A, H, L, n=n)
    params, sa_full, dq_full, qk = int_dev(S, A, H, L)
    # rows n .. n + 15 of the inputs are NaN: the first n rows and 16 NaN rows behind them
    sa = torch.full((n + GUARD, S + A), float("nan"), device="cuda")
    sa[:n] = sa_full[:n]
    dq = torch.full((n + GUARD, 2), float("nan"), device="cuda")
    dq[:n] = dq_full[:n]
    res = run_grad(params, sa, n, S, A, H, L, dq_in=dq, outs=("q", "dq_out", "partials"))
    assert same_bits(res["q"], qk[:n]), "q differs from pd_sac_critic's"
    assert torch.equal(res["q"].cpu(), torch.from_numpy(c["q"]))
    assert same_bits(res["dq_out"], dq[:n])
    total = 0.0
    for w in range(2):
        for k, (got, want) in enumerate(zip(res["grads"][w], c["grads"][w])):
            got = got.cpu().numpy().reshape(want.shape)
            assert not (got == SENTINEL).any(), f"net {w} tensor {k}: elements left unwritten"
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                i = tuple(bad[0])
                raise AssertionError(f"{(S, A, H, L, n)} net {w} tensor {k}: {len(bad)} of {want.size} gradient values "
                                     f"differ from the int64 backward pass; first {i}: got {got[i]}, want {want[i]}")
            total += float((want.astype(np.float64) ** 2).sum())
    # the partials add up to the squared norm (integers; the sum itself may round above 2**24)
    got = float(res["partials"].double().sum())
    assert abs(got - total) <= 1e-5 * total, (got, total)
    return c


@pytest.mark.parametrize("n", gn.BATCHES)
@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_N)
def test_gradients_integer_net_exact(pd, S, A, H, L, n):
    c = check_exact(S, A, H, L, n)
    if n == sn.N_EXACT:
        assert c["zero_pre"] > 0         # pre-activations that are exactly 0: relu'(0) = 0 is exercised


@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_DEEP)
def test_gradients_integer_net_exact_deep(pd, S, A, H, L):
    assert check_exact(S, A, H, L, sn.N_EXACT)["zero_pre"] > 0


def test_gradients_from_wide_rows(pd):
    """pitch = the buffer's row width: the same gradients from [n][2S + A + 2] rows whose other columns
    are NaN."""
    import torch
    S, A, H, L = 2, 1, 256, 2
    n = sn.N_EXACT
    c = gn.int_grad_case(S, A, H, L)
    params, sa, dq, _ = int_dev(S, A, H, L)
    rows = torch.full((n + GUARD, 2 * S + A + 2), float("nan"), device="cuda")
    rows[:n, :S + A] = sa[:n]
    res = run_grad(params, rows, n, S, A, H, L, dq_in=dq, outs=("q",))
    for w in range(2):
        for got, want in zip(res["grads"][w], c["grads"][w]):
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)


# ------------------------------------------------------------------ the real-valued cases
_real = {}


def real_case(S, A, H, L):
    """The real-valued case of a shape on the device (once, never modified): sac_grad_nets.grad_case plus
    the critic's device copy, its parameter tensors per net, rows, target, weights and ONE
    pd_sac_critic_grad call at n = 261 (L2, PER weights, every output)."""
    import torch
    key = (S, A, H, L)
    if key not in _real:
        case = gn.grad_case(S, A, H, L)
        critic = copy.deepcopy(case["critic"]).cuda()
        params = [[t for m in td.q_linears(net) for t in (m.weight.data, m.bias.data)] for net in (critic.q1, critic.q2)]
        dev = dict(critic=critic, params=params, rows=torch.from_numpy(case["rows"]).cuda(),
                   target=torch.from_numpy(case["target"]).cuda(), weights=torch.from_numpy(case["weights"]).cuda())
        dev["out"] = run_grad(params, dev["rows"], case["n"], S, A, H, L, target=dev["target"], weights=dev["weights"])
        case["dev"] = dev
        _real[key] = case
    return _real[key]


# ------------------------------------------------------------------ 2. the loss gradient
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("kind", [gn.L2, gn.L1])
def test_loss_gradient_within_the_a_priori_bound(pd, kind, per):
    import torch
    S, A, H, L = 5, 4, 256, 3
    case = real_case(S, A, H, L)
    dev, n = case["dev"], case["n"]
    q0 = dev["out"]["q"]
    # rows 3 and 100: target == q of net 0 / net 1 exactly (sign(0) = 0, |td| = 0 on that net)
    target = dev["target"].clone()
    target[3], target[100] = q0[3, 0], q0[100, 1]
    weights = dev["weights"] if per else None
    res = run_grad(dev["params"], dev["rows"], n, S, A, H, L, target=target, weights=weights, kind=kind)
    assert same_bits(res["q"], q0)
    m = gn.loss_model(res["q"].cpu().numpy(), target.cpu().numpy(), case["weights"] if per else None, kind)
    dq, tdv, loss = (res[k].cpu().numpy().astype(np.float64) for k in ("dq_out", "td_abs", "loss"))
    assert m["dq"][3, 0] == 0 and m["dq"][100, 1] == 0 and m["dq"][3, 1] != 0
    assert dq[3, 0] == 0 and dq[100, 1] == 0
    e_dq, e_td, e_loss = np.abs(dq - m["dq"]), np.abs(tdv - m["td_abs"]), abs(float(loss[0]) - m["loss"])
    print(f"kind {kind} per {per}: dq err/bound {np.max(e_dq / np.maximum(m['E_dq'], 1e-300)):.3f}, td_abs "
          f"{np.max(e_td / np.maximum(m['E_td'], 1e-300)):.3f}, loss {e_loss / m['E_loss']:.3f} (loss {m['loss']:.6g})")
    assert (e_dq <= m["E_dq"]).all(), float(np.max(e_dq / np.maximum(m["E_dq"], 1e-300)))
    assert (e_td <= m["E_td"]).all()
    assert e_loss <= m["E_loss"], (e_loss, m["E_loss"])
    if kind == gn.L1:
        assert set(np.unique(np.sign(dq))) == {-1.0, 0.0, 1.0}


# ------------------------------------------------------------------ 3. the whole gradient
def torch_grads(critic, rows, target, weights, S, A, kind=gn.L2):
    """The reference's forward, loss and backward in the tensors' dtype and on their device: the
    gradients in parameters() order."""
    import torch
    import torch.nn.functional as F
    critic.zero_grad()
    q1, q2 = critic(rows[:, :S], rows[:, S:S + A])
    t, w = target.reshape(-1, 1), weights.reshape(-1, 1)
    f = F.l1_loss if kind == gn.L1 else F.mse_loss
    loss = (w * f(q1, t, reduction="none") + w * f(q2, t, reduction="none")).mean()
    loss.backward()
    return [p.grad.detach().cpu().numpy().astype(np.float64) for p in critic.parameters()], float(loss.detach())


def measure_real(S, A, H, L):
    """Per parameter tensor: (err_k, err_torch, floor, max |ref|) against float64 autograd."""
    import torch
    case = real_case(S, A, H, L)
    dev = case["dev"]
    c64 = copy.deepcopy(case["critic"]).double()
    rows, target, weights = (torch.from_numpy(case[k]) for k in ("rows", "target", "weights"))
    ref, _ = torch_grads(c64, rows.double(), target.double(), weights.double(), S, A)
    g_gpu, _ = torch_grads(copy.deepcopy(dev["critic"]), dev["rows"], dev["target"], dev["weights"], S, A)
    g_cpu, _ = torch_grads(copy.deepcopy(case["critic"]), rows, target, weights, S, A)
    p1, p2 = td.critic_params(case["critic"])
    model, terms, _ = gn.full_backward((p1, p2), case["rows"][:, :S + A], case["target"], case["weights"], gn.L2)
    got = [g.cpu().numpy().astype(np.float64) for w in range(2) for g in dev["out"]["grads"][w]]
    out = []
    for k, r in enumerate(ref):
        assert np.abs(model[k] - r).max() <= 1e-9 * max(1.0, np.abs(r).max())      # the NumPy model is autograd64
        err_k = float(np.abs(got[k].reshape(r.shape) - r).max())
        err_t = max(float(np.abs(g_gpu[k] - r).max()), float(np.abs(g_cpu[k] - r).max()))
        out.append((err_k, err_t, case["n"] * gn.EPS32 * terms[k], float(np.abs(r).max())))
    return out


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_gradient_error_within_torch_f32_error(pd, S, A, H, L):
    res = measure_real(S, A, H, L)
    for k, (err_k, err_t, floor, top) in enumerate(res):
        print(f"{(S, A, H, L)} tensor {k}: err_k {err_k:.3e} err_torch {err_t:.3e} floor {floor:.3e} max |ref| {top:.3g} "
              f"ratio {err_k / max(err_t, 1e-300):.2f}")
    assert max(top for _, _, _, top in res) > 1e-3
    for k, (err_k, err_t, floor, top) in enumerate(res):
        assert err_k <= max(REAL_C * err_t, floor), (k, err_k, err_t, floor)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_N)
def test_determinism(pd, S, A, H, L):
    import torch
    case = real_case(S, A, H, L)
    dev, n = case["dev"], case["n"]
    first = dev["out"]
    again = run_grad(dev["params"], dev["rows"], n, S, A, H, L, target=dev["target"], weights=dev["weights"])
    for w in range(2):
        for a, b in zip(first["grads"][w], again["grads"][w]):
            assert same_bits(a, b)
    for k in ("q", "td_abs", "dq_out", "loss", "partials"):
        assert same_bits(first[k], again[k]), k
    # no optional output asked for: the same gradients
    bare = run_grad(dev["params"], dev["rows"], n, S, A, H, L, target=dev["target"], weights=dev["weights"], outs=())
    for w in range(2):
        for a, b in zip(first["grads"][w], bare["grads"][w]):
            assert same_bits(a, b)
    # a row's q, dq and td_abs do not depend on the batch it sits in (under dq_in: 1 / B differs otherwise)
    dq_in = first["dq_out"].contiguous()
    big = run_grad(dev["params"], dev["rows"], n, S, A, H, L, target=dev["target"], dq_in=dq_in)
    small = run_grad(dev["params"], dev["rows"], 37, S, A, H, L, target=dev["target"], dq_in=dq_in)
    for k in ("q", "dq_out", "td_abs"):
        assert same_bits(small[k], big[k][:37]), k
    assert same_bits(big["q"], first["q"]) and same_bits(big["td_abs"], first["td_abs"])
    # and dq_in = the loss's own dq gives the loss's own gradients
    for w in range(2):
        for a, b in zip(first["grads"][w], big["grads"][w]):
            assert same_bits(a, b)


# ------------------------------------------------------------------ 5. pd_adam_step
ADAM_NUMEL = [1, 5, 513, 4096, 1024]
LR, BETAS, EPS_ADAM, TAU = 3e-4, (0.9, 0.999), 1e-8, 0.005


def adam_inputs(step, seed=0):
    """Float32 p, g, m, v, t per tensor (NumPy): m and v zero before step 1, else a plausible state."""
    rng = np.random.default_rng([seed, step])
    p = [rng.uniform(-1, 1, k).astype(np.float32) for k in ADAM_NUMEL]
    g = [(rng.standard_normal(k) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32) for k in ADAM_NUMEL]
    g[2][7] = 0.0                                  # a zero gradient
    if step == 1:
        m = [np.zeros(k, dtype=np.float32) for k in ADAM_NUMEL]
        v = [np.zeros(k, dtype=np.float32) for k in ADAM_NUMEL]
    else:
        m = [(x * rng.uniform(0.5, 1.5, x.shape)).astype(np.float32) for x in g]
        v = [(x.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, x.shape)).astype(np.float32) for x in g]
    t = [rng.uniform(-1, 1, k).astype(np.float32) for k in ADAM_NUMEL]
    return p, g, m, v, t


def run_adam(arrs, step, max_norm=0.0, partials=None, targets=True):
    """One pd_adam_step on device copies of the NumPy lists, all carved from ONE buffer with 3 sentinel
    floats between any two tensors (so most tensors start at an odd address); returns the five lists
    after the call (NumPy), grad_norm_out and whether every guard float is intact."""
    import torch
    from pdenv import _lib
    lib = _lib.load()
    flat, spans = [], []
    for lst in arrs:
        for a in lst:
            spans.append((sum(len(x) for x in flat), len(a)))
            flat += [a, np.full(3, SENTINEL, dtype=np.float32)]
    host = np.concatenate(flat)
    buf = torch.from_numpy(host).cuda()
    nt = len(ADAM_NUMEL)
    views = [[buf[o:o + k] for o, k in spans[i * nt:(i + 1) * nt]] for i in range(5)]
    numel = (C.c_int64 * nt)(*ADAM_NUMEL)
    norm = torch.full((1 + GUARD,), SENTINEL, device="cuda")
    parts = None if partials is None else torch.from_numpy(np.asarray(partials, dtype=np.float32)).cuda()
    t = step
    st = lib.pd_adam_step(nt, *[ptr_list(v) for v in views[:4]], numel, ptr_list(views[4]) if targets else None,
                          LR / (1 - BETAS[0] ** t), (1 - BETAS[1] ** t) ** 0.5, BETAS[0], BETAS[1], EPS_ADAM, max_norm,
                          None if parts is None else vp(parts.data_ptr()), 0 if parts is None else parts.numel(),
                          vp(norm.data_ptr()), TAU, None)
    assert st == _lib.PD_OK, lib.pd_last_error()
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    mask = np.ones(len(after), dtype=bool)
    for o, k in spans:
        mask[o:o + k] = False
    guards_ok = bool((after[mask] == SENTINEL).all()) and bool((norm[1:] == SENTINEL).all())
    lists = [[after[o:o + k] for o, k in spans[i * nt:(i + 1) * nt]] for i in range(5)]
    return lists, float(norm[0]), guards_ok


@pytest.mark.parametrize("clip", ["off", "above", "below"])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_step(pd, step, clip):
    p, g, m, v, t = adam_inputs(step)
    # the partials as a caller's: float32 roundings of the tensors' binary64 sums of squares
    parts = np.array([float((x.astype(np.float64) ** 2).sum()) for x in g]).astype(np.float32)
    norm64 = float(np.sqrt(sum((x.astype(np.float64) ** 2).sum() for x in g)))
    max_norm = dict(off=0.0, above=2.0 * norm64, below=0.25 * norm64)[clip]
    (p1, g1, m1, v1, t1), norm, guards_ok = run_adam((p, g, m, v, t), step, max_norm, parts if clip != "off" else None)
    assert guards_ok, "floats between the tensors were written"
    # each partial carries its own rounding (e relative): e total / 2 on the norm
    model = gn.adam_model(p, g, m, v, step, LR, BETAS[0], BETAS[1], EPS_ADAM, max_norm, parts,
                          E_total_extra=gn.EPS32 * norm64 / 2)
    if clip == "off":
        assert norm == SENTINEL                                    # grad_norm_out untouched
    else:
        assert abs(norm - norm64) <= model["E_norm"], (norm, norm64, model["E_norm"])
    if clip != "below":
        assert model["coef"] == 1.0
        for a, b in zip(g, g1):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), "gradients changed without clipping"
    else:
        assert abs(model["coef"] - 0.25) < 1e-3
    worst = {}
    for name, got in (("p", p1), ("g", g1), ("m", m1), ("v", v1)):
        for k in range(len(ADAM_NUMEL)):
            err = np.abs(got[k].astype(np.float64) - model[name][k])
            bound = model["E_" + name][k] + np.zeros_like(err)
            ok = err <= bound
            worst[name] = max(worst.get(name, 0.0), float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0)
            assert ok.all(), (name, k, float(err[~ok][0]), float(bound[~ok][0]))
    print(f"step {step} clip {clip}: worst err/bound {worst}")
    # Polyak on the kernel's own new p: torch's expression, exactly
    for k in range(len(ADAM_NUMEL)):
        want = gn.polyak_f32(t[k], p1[k], TAU)
        assert np.array_equal(t1[k].view(np.int32), want.view(np.int32)), k
    # a zero gradient at step 1 leaves the parameter where it was
    if step == 1 and clip == "off":
        assert p1[2][7] == p[2][7] and m1[2][7] == 0 and v1[2][7] == 0


def test_adam_polyak_equals_torch_and_targets_null(pd):
    import torch
    p, g, m, v, t = adam_inputs(2)
    (p1, g1, m1, v1, t1), _, ok = run_adam((p, g, m, v, t), 2)
    assert ok
    for k in range(len(ADAM_NUMEL)):
        tt, pp = torch.from_numpy(t[k]).cuda(), torch.from_numpy(p1[k].copy()).cuda()
        want = ((1 - TAU) * tt + TAU * pp).cpu().numpy()
        assert np.array_equal(t1[k].view(np.int32), want.view(np.int32)), k
    (p2, g2, m2, v2, t2), _, ok = run_adam((p, g, m, v, t), 2, targets=False)
    assert ok
    for a, b in zip(p1 + m1 + v1 + g1, p2 + m2 + v2 + g2):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(t, t2):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "targets written with targets = NULL"


# ------------------------------------------------------------------ 6. CriticUpdate end to end
def torch_block(critic, target, opt, rows, target_q, weights, S, A, tau, use_l1, max_norm):
    """Steps 2, 3 and 8 of SACPyTorch.update and step 7's |td| (sac_pytorch.py:445-483, :526, :530-531)."""
    import torch
    import torch.nn.functional as F
    q1, q2 = critic(rows[:, :S], rows[:, S:S + A])
    t, w = target_q.reshape(-1, 1), weights.reshape(-1, 1)
    f = F.l1_loss if use_l1 else F.mse_loss
    loss = (w * f(q1, t, reduction="none") + w * f(q2, t, reduction="none")).mean()
    opt.zero_grad()
    loss.backward()
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(critic.parameters(), max_norm=max_norm)
    opt.step()
    for p, tp in zip(critic.parameters(), target.parameters()):
        tp.data.copy_((1 - tau) * tp.data + tau * p.data)
    return loss.detach(), norm, torch.max((t - q1).abs(), (t - q2).abs()).detach().reshape(-1)


def to_np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def test_critic_update_end_to_end(pd):
    import torch
    from pdenv.sac import Critic, CriticUpdate
    S, A, H, L, B = 2, 1, 256, 2, 256
    tau, max_norm = 0.005, 0.05
    critic = td.real_critic(S, A, H, L).cuda()
    target = td.real_critic(S, A, H, L, seed=1).cuda()
    opt = torch.optim.Adam(critic.parameters(), lr=LR)
    assert CriticUpdate.supported(critic, opt, target)
    upd = CriticUpdate(critic, target, opt, tau=tau, max_grad_norm=max_norm)
    assert upd.kernel
    rng = np.random.default_rng(5)
    ptrs = [p.data_ptr() for p in critic.parameters()]
    for it in range(5):
        rows = torch.from_numpy(rng.uniform(-1, 1, (B, 2 * S + A + 2)).astype(np.float32)).cuda()
        tq = torch.from_numpy(rng.uniform(-2, 2, (B, 1)).astype(np.float32)).cuda()
        w = torch.from_numpy(rng.uniform(0.2, 1, (B, 1)).astype(np.float32)).cuda()
        if it == 3:      # parameters are read and written in place: an outside write is seen
            with torch.no_grad():
                for p in critic.parameters():
                    p.data.copy_(p.data * 0.5)
        # ---- the state this update starts from, as float64 copies on the CPU
        c64, t64 = copy.deepcopy(critic).cpu().double(), copy.deepcopy(target).cpu().double()
        o64 = torch.optim.Adam(c64.parameters(), lr=LR)
        if it > 0:
            sd = copy.deepcopy(opt.state_dict())
            for s in sd["state"].values():
                s["exp_avg"], s["exp_avg_sq"] = s["exp_avg"].cpu().double(), s["exp_avg_sq"].cpu().double()
            o64.load_state_dict(sd)
        before = dict(p=to_np(critic.parameters()), t=to_np(target.parameters()),
                      m=[np.zeros_like(x) for x in to_np(critic.parameters())] if it == 0 else
                        to_np([opt.state[p]["exp_avg"] for p in critic.parameters()]),
                      v=[np.zeros_like(x) for x in to_np(critic.parameters())] if it == 0 else
                        to_np([opt.state[p]["exp_avg_sq"] for p in critic.parameters()]))
        # float64 gradients, torch's float32 gradients at the same state, test 3's bound per tensor
        g64, _ = torch_grads(copy.deepcopy(c64), rows.cpu().double(), tq.cpu().double(), w.cpu().double(), S, A)
        g32, _ = torch_grads(copy.deepcopy(critic), rows, tq, w, S, A)
        p1, p2 = td.critic_params(copy.deepcopy(critic).cpu())
        _, terms, _ = gn.full_backward((p1, p2), rows.cpu().numpy()[:, :S + A], tq.cpu().numpy()[:, 0],
                                       w.cpu().numpy()[:, 0], gn.L2)
        E_g = [max(REAL_C * float(np.abs(a - b).max()), B * gn.EPS32 * t) for a, b, t in zip(g32, g64, terms)]
        # ---- the kernel's update and the float64 block
        td_abs = upd(rows, tq, w).clone()
        torch.cuda.synchronize()
        loss64, norm64, td64 = torch_block(c64, t64, o64, rows.cpu().double(), tq.cpu().double(), w.cpu().double(),
                                           S, A, tau, False, max_norm)
        assert [p.data_ptr() for p in critic.parameters()] == ptrs
        # ---- test 5's propagation with E_g; the partials are the kernel's own sums (about 24 float32
        # additions each on top of their count), the norm carries the gradients' error
        parts = [float((x ** 2).sum()) for x in g64]
        extra = float(np.sqrt(sum(e ** 2 * x.size for e, x in zip(E_g, g64)))) + 24 * gn.EPS32 * float(norm64)
        model = gn.adam_model(before["p"], g64, before["m"], before["v"], it + 1, LR, BETAS[0], BETAS[1], EPS_ADAM, max_norm,
                              parts, E_g=E_g, sum_terms=upd.n_partials, E_total_extra=extra)
        assert abs(model["norm"] - float(norm64)) <= 1e-12 * float(norm64)
        assert float(norm64) > max_norm                          # the clip is active
        assert abs(float(upd.grad_norm) - float(norm64)) <= model["E_norm"]
        got = dict(p=to_np(critic.parameters()), m=to_np([opt.state[p]["exp_avg"] for p in critic.parameters()]),
                   v=to_np([opt.state[p]["exp_avg_sq"] for p in critic.parameters()]), t=to_np(target.parameters()))
        ref = dict(p=to_np(c64.parameters()), m=to_np([o64.state[p]["exp_avg"] for p in c64.parameters()]),
                   v=to_np([o64.state[p]["exp_avg_sq"] for p in c64.parameters()]), t=to_np(t64.parameters()))
        worst = {}
        for name in ("p", "m", "v"):
            for k in range(len(ref["p"])):
                # (the float64 block's constants are binary64, the model's the float32 ones the kernel receives:
                # the distance between the two references is added, a property of the references alone)
                bound = model["E_" + name][k] + np.abs(model[name][k].reshape(ref[name][k].shape) - ref[name][k])
                err = np.abs(got[name][k].astype(np.float64) - ref[name][k])
                worst[name] = max(worst.get(name, 0.0), float(np.max(err / np.maximum(bound, 1e-300))))
                assert (err <= bound).all(), (it, name, k, float(np.max(err / np.maximum(bound, 1e-300))))
        for k in range(len(ref["p"])):
            # t' = fl(1 - tau) t + fl(tau) p': three roundings, tau E_p, and the two constants' roundings
            tp = ref["t"][k]
            bound = (tau * (model["E_p"][k] + np.abs(model["p"][k] - ref["p"][k]))
                     + 5 * gn.EPS32 * (np.abs(before["t"][k]) + tau * np.abs(ref["p"][k]) + np.abs(tp)))
            assert (np.abs(got["t"][k].astype(np.float64) - tp) <= bound).all(), (it, "t", k)
        lm = gn.loss_model(upd.q.cpu().numpy(), tq.cpu().numpy()[:, 0], w.cpu().numpy()[:, 0], gn.L2)
        assert abs(float(upd.critic_loss) - lm["loss"]) <= lm["E_loss"]
        assert (np.abs(td_abs.cpu().numpy() - lm["td_abs"]) <= lm["E_td"]).all()
        assert abs(float(loss64) - lm["loss"]) <= 1e-4 * abs(lm["loss"])
        assert int(opt.state[next(iter(critic.parameters()))]["step"].item()) == it + 1
        print(f"update {it}: worst err/bound {worst}, loss {float(upd.critic_loss):.6g}, norm {float(upd.grad_norm):.6g}")
    # ---- the optimizer's state dict loads into a fresh torch Adam, which continues with torch's own step
    sd = opt.state_dict()
    twin = copy.deepcopy(critic)
    fresh = torch.optim.Adam(twin.parameters(), lr=LR)
    fresh.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(critic.parameters(), twin.parameters()):
        assert same_bits(opt.state[p]["exp_avg"], fresh.state[q]["exp_avg"])
        assert float(fresh.state[q]["step"]) == 5
    rows = torch.from_numpy(rng.uniform(-1, 1, (B, 2 * S + A + 2)).astype(np.float32)).cuda()
    tq = torch.from_numpy(rng.uniform(-2, 2, (B, 1)).astype(np.float32)).cuda()
    w = torch.ones(B, 1, device="cuda")
    t_twin = copy.deepcopy(target)
    before6 = [p.detach().clone() for p in critic.parameters()]
    torch_block(twin, t_twin, fresh, rows, tq, w, S, A, tau, False, max_norm)
    upd(rows, tq, w)
    torch.cuda.synchronize()
    assert float(fresh.state[next(iter(twin.parameters()))]["step"]) == 6
    for p, q, b in zip(critic.parameters(), twin.parameters(), before6):
        # the sixth update both ways from the same state.  One Adam step moves a parameter by at most
        # lr (1 - beta1) / sqrt(1 - beta2) / sqrt(1 - beta1^2 / beta2) sqrt(bc2) / bc1 = 1.2 lr at t = 6
        # (Cauchy-Schwarz on the two moving averages), so the two ends are within 2.5 lr of each other
        assert bool(torch.isfinite(q).all()) and not torch.equal(q, b) and not torch.equal(p, b)
        assert float((p - q).detach().abs().max()) <= 2.5 * LR


def test_critic_update_backward_and_fallback(pd):
    """backward() alone leaves the gradients in p.grad (overwritten, also under dq); an unsupported
    critic (hidden 64) or optimizer takes the torch path and returns the same fields."""
    import torch
    from pdenv.sac import Critic, CriticUpdate
    S, A, B = 5, 4, 37
    case = real_case(S, A, 256, 3)
    dev = case["dev"]
    critic, target = copy.deepcopy(dev["critic"]), copy.deepcopy(dev["critic"])
    opt = torch.optim.Adam(critic.parameters(), lr=LR)
    upd = CriticUpdate(critic, target, opt)
    assert upd.kernel
    for p in critic.parameters():
        p.grad = torch.full_like(p, 7.0)                     # overwritten, not accumulated into
    before = [p.detach().clone() for p in critic.parameters()]
    td_abs = upd.backward(dev["rows"], dev["target"], dev["weights"])
    torch.cuda.synchronize()
    flat = [g for w in range(2) for g in dev["out"]["grads"][w]]
    for p, g, b in zip(critic.parameters(), flat, before):
        assert same_bits(p.grad.reshape(-1), g) and same_bits(p, b)
    assert same_bits(td_abs, dev["out"]["td_abs"]) and same_bits(upd.q, dev["out"]["q"])
    assert same_bits(upd.critic_loss, dev["out"]["loss"]) and len(opt.state) == 0
    upd.backward(dev["rows"], None, dq=dev["out"]["dq_out"].contiguous())
    torch.cuda.synchronize()
    for p, g in zip(critic.parameters(), flat):
        assert same_bits(p.grad.reshape(-1), g)
    # ---- the fallback
    torch.manual_seed(3)
    small, small_t = Critic(S, A, hidden_dim=64, n_hidden_layers=2).cuda(), Critic(S, A, hidden_dim=64, n_hidden_layers=2).cuda()
    opt2 = torch.optim.Adam(small.parameters(), lr=LR)
    assert not CriticUpdate.supported(small, opt2, small_t)
    fb = CriticUpdate(small, small_t, opt2, tau=0.01, max_grad_norm=0.5)
    assert not fb.kernel
    twin, twin_t = copy.deepcopy(small), copy.deepcopy(small_t)
    opt3 = torch.optim.Adam(twin.parameters(), lr=LR)
    rows, tq, w = dev["rows"][:B], dev["target"][:B].reshape(B, 1), dev["weights"][:B].reshape(B, 1)
    got = fb(rows, tq, w)
    loss, norm, td_ref = torch_block(twin, twin_t, opt3, rows, tq, w, S, A, 0.01, False, 0.5)
    assert got.shape == (B,) and torch.equal(got, td_ref)
    assert fb.q.shape == (B, 2) and fb.critic_loss.shape == (1,) and fb.grad_norm.shape == (1,)
    assert float(fb.critic_loss) == float(loss) and float(fb.grad_norm) == float(norm)
    for a, b in zip(list(small.parameters()) + list(small_t.parameters()), list(twin.parameters()) + list(twin_t.parameters())):
        assert torch.equal(a, b)
    wd = torch.optim.Adam(critic.parameters(), lr=LR, weight_decay=1e-2)
    assert not CriticUpdate(critic, target, wd).kernel


if __name__ == "__main__":     # python tests/test_gpu_sac_update.py OUT.json: the measurements alone
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "psso-sac-for-powered-descent_amd"))
    shapes = []
    for shape in td.SHAPES:
        res = measure_real(*shape)
        row = dict(shape=list(shape), n=sn.N_REAL, loss="L2 with PER weights",
                   tensors=[dict(err_kernel=k, err_torch=t, floor=f, max_abs_ref=top, ratio=(k / t if t > 0 else None))
                            for k, t, f, top in res])
        row["worst_ratio"] = max(x["ratio"] for x in row["tensors"] if x["ratio"] is not None)
        shapes.append(row)
        print(shape, "worst ratio", row["worst_ratio"])
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(what="pd_sac_critic_grad and torch float32 autograd (the larger of its GPU and CPU errors) against "
                            "float64 autograd of the same float32 parameters, rows, targets and PER weights: max |grad - "
                            "ref64| per parameter tensor (q1's then q2's, parameters() order)",
                       bound_c=REAL_C, shapes=shapes), fh, indent=1)
        fh.write("\n")
