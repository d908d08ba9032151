"""pd_sac_critic and pd_sac_td_target (csrc/pdsactd.hip) against references outside the kernels.

1. The twin critic exactly: integer nets (sac_td_nets.int_critic_case) whose every partial sum is
   an integer below 2**24; q must EQUAL the int64 forward pass, Q1 in column 0 and Q2 in column 1.
2. The fused kernel equals its pieces bit for bit (pd_sac_actor, pd_sac_critic, eps_in).
3. The elementwise chain between the pieces against a binary64 model, under an a-priori bound.
4. The whole block against binary64, no worse than REAL_C times torch's own float32 evaluations.
5. The eps draws: reproducible, independent of batch and grid, the NumPy restatement's values.
6. Parameters and log_alpha are read in place.
7. Refusals before any launch, and the torch fallback.

The bound of test 3 (sac_td_nets.chain_bound).  The inputs -- the kernel's own heads, eps_out and
next_q, and the rows -- are float32 numbers, exact in the model, so only the chain's own roundings
count.  With e = 2**-24 (one float32 rounding, relative) and the device library's expf, logf and
tanhf taken at the OpenCL full-profile bounds its math library is built to (3, 3 and 5 ulp; k ulp
is at most 2 k e relative), first-order propagation gives, as absolute errors E:
    sd = expf(ls)            E_sd = 6 e sd                      (ls: a clamp, exact)
    p = sd eps, x = m + p    E_x = |eps| E_sd + e |p| + e |x|
    a = tanhf(x)             E_a = (1 - a^2) E_x + 10 e |a|     (tanh' = 1 - a^2 <= 1)
    act = a max_action       E_act = max_action E_a + e |act|
    d = x - m                E_d = E_x + e |d|                  (e |x| of x's rounding comes back:
                                                                 for a small sd it is large against d)
    t1 = d d / (2 sd sd)     E_t1 = (2 |d| E_d + e d^2) / den + d^2 E_den / den^2 + e t1,
                             den = 2 sd^2, E_den = 2 (2 sd E_sd + e sd^2)
    w = 1 - a a + 1e-6       E_w = 2 |a| E_a + e a^2 + e |1 - a^2| + e w
    lg = logf(w)             E_lg = E_w / w + 6 e |lg|          (the amplification 1 / (1 - a^2 + 1e-6))
    lp_k = -t1 - ls - c - lg E_lpk = E_t1 + E_lg + e (|-t1 - ls| + |-t1 - ls - c| + |lp_k|)
    lp = sum_k lp_k          E_lp = sum E_lpk + e sum of the |partial sums| after the first
    alpha = expf(log_alpha)  E_alpha = 6 e alpha
    nq = minq - alpha lp     E_nq = |lp| E_alpha + alpha E_lp + e |alpha lp| + e |nq|
    f = (1 - done) gamma     E_f = e |f| + e |1 - done| gamma
    tq = r + f nq            E_tq = |nq| E_f + |f| E_nq + e |f nq| + e |tq|
each evaluated on the model's values, times 1.01 for the products of errors.  Nothing in it comes
from the kernel's output.  The comparisons are reported in float32 ulps at the model's value; the
condition on the inputs, asserted on the model, is 1 - a^2 >= 1e-3 on every row.

Measured (MI355X, `python tests/test_gpu_sac_td.py OUT.json`): profiles/sac_td_target_shapes.json."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import sac_nets as sn
import sac_td_nets as td

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5     # no integer: no output of an integer net equals it
GUARD = 16
REAL_C = 4.0            # tests/test_gpu_sac_actor.py: one fma chain against blocked GEMM sums, a maximum
                        # over a few hundred values -- the same situation, the same constant
OUTS = ("next_actions", "next_log_prob", "next_q", "heads", "eps_out")


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


# ------------------------------------------------------------------ 1. the critic, exact
_int = {}


def int_kernel(S, A, H, L):
    """The integer case of a shape (computed once, never modified): CriticKernel, states, actions and
    the reference q [37][2] on the device."""
    import torch
    from pdenv.sac import Critic, CriticKernel
    key = (S, A, H, L)
    if key not in _int:
        p1, p2, states, actions, ref = td.int_critic_case(S, A, H, L)
        critic = td.load_critic(Critic(S, A, hidden_dim=H, n_hidden_layers=L), p1, p2).cuda()
        assert CriticKernel.supported(critic)
        _int[key] = (CriticKernel(critic), torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda(),
                     torch.from_numpy(ref).cuda())
    return _int[key]


def run_guarded(kern, dstates, dactions, n):
    """One pd_sac_critic launch over the first n rows, copied into [n + 16] row buffers whose 16 rows
    past n hold NaN; q [n + 16][2] with the sentinel in the 16 guard rows."""
    import torch
    q = torch.full((n + GUARD, 2), SENTINEL, device="cuda")
    s = torch.full((n + GUARD, dstates.shape[1]), float("nan"), device="cuda")
    a = torch.full((n + GUARD, dactions.shape[1]), float("nan"), device="cuda")
    s[:n] = dstates[:n]
    a[:n] = dactions[:n]
    kern(s[:n], a[:n], q[:n])
    torch.cuda.synchronize()
    return q[:n], q[n:]


def assert_exact(got, guard, ref, what):
    import torch
    assert bool((guard == SENTINEL).all()), f"{what}: q rows past n were written"
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} values differ from the integer reference; "
                             f"first (row, net) {i}: got {float(got[i])}, want {float(ref[i])}")


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_critic_integer_net_exact(pd, S, A, H, L):
    """n = 37: q equals the int64 reference, column 0 from Q1's parameters and column 1 from Q2's
    (the nets differ by construction), guard rows intact, NaN input rows past n reach no output."""
    kern, ds, da, ref = int_kernel(S, A, H, L)
    assert bool((ref[:, 0] != ref[:, 1]).any())
    got, guard = run_guarded(kern, ds, da, sn.N_EXACT)
    assert_exact(got, guard, ref, (S, A, H, L))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("S,A,H,L", td.SHAPES_N)
def test_critic_integer_net_exact_batch_sizes(pd, S, A, H, L, n):
    kern, ds, da, ref = int_kernel(S, A, H, L)
    got, guard = run_guarded(kern, ds, da, n)
    assert_exact(got, guard, ref[:n], (S, A, H, L, n))


# ------------------------------------------------------------------ the real-valued cases
_real = {}


def real_case(S, A, H, L):
    """The real-valued case of a shape on the device (computed once, never modified): the CPU case of
    sac_td_nets.td_case plus device copies of the nets, rows [261][W], eps and log_alpha, a TdTarget
    over them and the outputs of ONE call at n = 261 with eps_in and every optional output."""
    import copy
    import torch
    from pdenv.sac import TdTarget
    key = (S, A, H, L)
    if key not in _real:
        case = td.td_case(S, A, H, L)
        dev = dict(actor=copy.deepcopy(case["actor"]).cuda(), critic=copy.deepcopy(case["critic"]).cuda(),
                   rows=torch.from_numpy(case["rows"]).cuda(), eps=torch.from_numpy(case["eps"]).cuda(),
                   log_alpha=case["log_alpha"].clone().cuda())
        assert TdTarget.supported(dev["actor"], dev["critic"], dev["log_alpha"])
        dev["td"] = TdTarget(dev["actor"], dev["critic"], dev["log_alpha"], case["gamma"], seed=1234)
        dev["out"] = run_td(dev["td"], dev["rows"], A, eps=dev["eps"])
        case["dev"] = dev
        _real[key] = case
    return _real[key]


def run_td(tdt, rows, A, eps=None, draw=None, optional=True):
    """One TdTarget call into fresh NaN-filled outputs: dict of target_q [n] and, with optional, the
    five optional outputs."""
    import torch
    n = rows.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    out = dict(target_q=nan(n))
    if optional:
        out.update(next_actions=nan(n, A), next_log_prob=nan(n), next_q=nan(n, 2), heads=nan(n, 2 * A), eps_out=nan(n, A))
    tdt(rows, out=out["target_q"], draw=draw, eps=eps, **{k: out[k] for k in OUTS if k in out})
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    return out


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(x, y):
    import torch
    return torch.equal(bits(x), bits(y))


# ------------------------------------------------------------------ 2. fused = pieces
@pytest.mark.parametrize("B", [37, 1, 16, 17])
@pytest.mark.parametrize("S,A,H,L", td.SHAPES_N)
def test_fused_equals_pieces_bit_for_bit(pd, S, A, H, L, B):
    import torch
    from pdenv.sac import ActorKernel, CriticKernel
    case = real_case(S, A, H, L)
    dev = case["dev"]
    rows, eps = dev["rows"][:B].contiguous(), dev["eps"][:B].contiguous()
    out = run_td(dev["td"], rows, A, eps=eps)
    ns = rows[:, S + A + 1:2 * S + A + 1].contiguous()
    heads = torch.full((B, 2 * A), float("nan"), device="cuda")
    ActorKernel(dev["actor"])(ns, heads)
    q = torch.full((B, 2), float("nan"), device="cuda")
    CriticKernel(dev["critic"])(ns, out["next_actions"], q)
    torch.cuda.synchronize()
    assert same_bits(out["heads"], heads), "heads differ from pd_sac_actor(next_state)"
    assert same_bits(out["next_q"], q), "next_q differs from pd_sac_critic(next_state, next_actions)"
    assert same_bits(out["eps_out"], eps), "eps_out differs from eps_in"
    bare = run_td(dev["td"], rows, A, eps=eps, optional=False)
    assert same_bits(bare["target_q"], out["target_q"]), "target_q depends on which outputs are requested"
    # the rows are the first B of the n = 261 call: a row's values do not depend on the batch
    for k in ("target_q",) + OUTS:
        assert same_bits(out[k], dev["out"][k][:B]), k


# ------------------------------------------------------------------ 3. the elementwise chain
def chain_errors(case, out, log_alpha=None):
    """{name: (error / ulp, bound / ulp) arrays} of next_actions, next_log_prob and target_q against
    the binary64 chain on the kernel's own heads, eps_out and next_q; and the chain."""
    S, A, actor = case["S"], case["A"], case["actor"]
    la = float(case["log_alpha"][0]) if log_alpha is None else log_alpha
    c = td.chain(out["heads"].cpu().numpy(), out["eps_out"].cpu().numpy(), out["next_q"].cpu().numpy(), case["rows"],
                 S, A, actor.log_std_min, actor.log_std_max, actor.max_action, la, case["gamma"])
    res = {}
    for name, bound in zip(("next_actions", "next_log_prob", "target_q"), td.chain_bound(c)):
        model = c[name]
        ulp = np.spacing(np.abs(model).astype(np.float32)).astype(np.float64)
        err = np.abs(out[name].cpu().numpy().astype(np.float64) - model)
        res[name] = (err / ulp, bound / ulp)
    return res, c


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_elementwise_chain_within_the_a_priori_bound(pd, S, A, H, L):
    case = real_case(S, A, H, L)
    out = case["dev"]["out"]
    res, c = chain_errors(case, out)
    # conditions on the inputs, on the model: no row is left out
    assert (1 - c["a"] ** 2).min() >= 1e-3, (1 - c["a"] ** 2).min()
    done = case["rows"][:, -1] == 1
    assert done.sum() >= 5 and (~done).sum() >= 5
    for name, (err, bound) in res.items():
        k = int(np.argmax(err / bound))
        print(f"{(S, A, H, L)} {name}: max err {err.max():.2f} ulp, median bound {np.median(bound):.1f} ulp, "
              f"worst err/bound {err.flat[k] / bound.flat[k]:.3f} (err {err.flat[k]:.2f} ulp, bound {bound.flat[k]:.1f} ulp)")
    for name, (err, bound) in res.items():
        assert (err <= bound).all(), (name, float((err / bound).max()))
    # done = 1 with a finite next_q: the reward's bits
    tq = out["target_q"].cpu().numpy()
    assert np.isfinite(c["nq"][done]).all()
    assert np.array_equal(tq[done].view(np.int32), case["rows"][done, S + A].view(np.int32))


# ------------------------------------------------------------------ 4. end to end against torch
def measure_real(S, A, H, L):
    """(err_k, err_g, err_c, max |ref|, min 1 - a^2): max over rows of |target_q - ref64| of the kernel,
    torch float32 on the GPU and torch float32 on the CPU, on the same float32 parameters and eps."""
    import torch
    case = real_case(S, A, H, L)
    dev = case["dev"]
    c, _, _ = td.full(case)
    ref = c["target_q"]
    g = td.torch_block(dev["actor"], dev["critic"], dev["rows"], dev["eps"], dev["log_alpha"], case["gamma"], S, A)[0]
    cpu = td.torch_block(case["actor"], case["critic"], torch.from_numpy(case["rows"]), torch.from_numpy(case["eps"]),
                         case["log_alpha"], case["gamma"], S, A)[0]
    err = [float(np.abs(x.cpu().numpy().astype(np.float64).reshape(-1) - ref).max())
           for x in (dev["out"]["target_q"], g, cpu)]
    return err[0], err[1], err[2], float(np.abs(ref).max()), float((1 - c["a"] ** 2).min())


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_target_q_error_within_torch_f32_error(pd, S, A, H, L):
    err_k, err_g, err_c, top, margin = measure_real(S, A, H, L)
    print(f"(S, A, H, L) = {(S, A, H, L)}: err_k {err_k:.3e} err_g {err_g:.3e} err_c {err_c:.3e} "
          f"ratio {err_k / max(err_g, err_c):.2f} max |ref| {top:.3g} min 1 - a^2 {margin:.3g}")
    assert margin >= 1e-3, margin
    assert 0.1 <= top <= 1e3, top
    assert max(err_g, err_c) > 0
    assert err_k <= REAL_C * max(err_g, err_c), (err_k, err_g, err_c)


# ------------------------------------------------------------------ 5. the eps draws
def test_eps_draws(pd):
    import torch
    case = real_case(5, 4, 256, 3)
    dev, A = case["dev"], 4
    tdt = dev["td"]
    seed, draw = tdt.seed, (3 << 32) | 77
    a = run_td(tdt, dev["rows"][:37].contiguous(), A, draw=draw)
    b = run_td(tdt, dev["rows"][:37].contiguous(), A, draw=draw)
    for k in a:
        assert same_bits(a[k], b[k]), k                       # the same (seed, draw): the same bits
    small = run_td(tdt, dev["rows"][:17].contiguous(), A, draw=draw)
    assert same_bits(small["eps_out"], a["eps_out"][:17])     # independent of the batch and the grid
    assert same_bits(small["target_q"], a["target_q"][:17])
    other = run_td(tdt, dev["rows"][:37].contiguous(), A, draw=draw + 1)
    assert not bool((other["eps_out"] == a["eps_out"]).any())
    tdt.seed = seed + 1
    try:
        reseeded = run_td(tdt, dev["rows"][:37].contiguous(), A, draw=draw)
    finally:
        tdt.seed = seed
    assert not bool((reseeded["eps_out"] == a["eps_out"]).any())
    # against the NumPy Box-Muller on philox_np's blocks: the kernel's binary64 normal is accurate to
    # about 1e-15, so only a rounding boundary of the cast can differ
    ref = td.np_eps(seed, draw, 37, A)
    got = a["eps_out"].cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - ref) <= ulp).all(), float((np.abs(got - ref) / ulp).max())
    assert (got == ref.astype(np.float32)).mean() > 0.99
    # the default draw is a counter that advances by one per call
    tdt.draws = draw
    c = run_td(tdt, dev["rows"][:37].contiguous(), A)
    d = run_td(tdt, dev["rows"][:37].contiguous(), A)
    assert tdt.draws == draw + 2
    assert same_bits(c["eps_out"], a["eps_out"]) and same_bits(d["eps_out"], other["eps_out"])


def test_eps_moments(pd):
    """B = 1024, A = 8: 8192 normals, |mean| <= 5 / sqrt(8192) and |var - 1| <= 5 sqrt(2 / 8192)."""
    import torch
    from pdenv.sac import Actor, Critic, TdTarget
    S, A, B = 2, 8, 1024
    torch.manual_seed(0)
    actor, critic = Actor(S, A, hidden_dim=128, n_hidden_layers=1).cuda(), Critic(S, A, hidden_dim=128, n_hidden_layers=1).cuda()
    tdt = TdTarget(actor, critic, torch.zeros(1, device="cuda"), 0.99, seed=99)
    assert tdt.kernel
    rows = torch.rand(B, 2 * S + A + 2, device="cuda")
    eps = run_td(tdt, rows, A, draw=5)["eps_out"].cpu().numpy().astype(np.float64)
    n = eps.size
    assert n == 8192
    assert abs(eps.mean()) <= 5 / np.sqrt(n), eps.mean()
    assert abs(eps.var() - 1) <= 5 * np.sqrt(2 / n), eps.var()
    # no block served twice: 8192 float32 normals meet by chance about once (n^2 / 2 over some 2^25
    # float32 values in the bulk), a repeated block would repeat hundreds
    assert len(np.unique(eps)) >= n - 16


# ------------------------------------------------------------------ 6. in place
def test_in_place_updates_are_seen_by_the_next_call(pd):
    """After log_alpha.data.add_(0.5) and a Polyak-style copy_ into the target critic, the next call on
    the SAME TdTarget gives the new values: target_q follows the chain model with the new alpha under
    test 3's bound and no longer the old alpha's, next_q equals pd_sac_critic on the new parameters
    and differs from the old, the whole block is within test 4's criterion of the binary64 model of
    the new parameters; ptrs() is unchanged."""
    import copy
    import torch
    from pdenv.sac import CriticKernel, TdTarget
    S, A, H, L = 5, 4, 256, 3
    case = dict(real_case(S, A, H, L))
    dev = case["dev"]
    actor, critic = dev["actor"], copy.deepcopy(dev["critic"])
    log_alpha = dev["log_alpha"].clone()
    tdt = TdTarget(actor, critic, log_alpha, case["gamma"])
    before = run_td(tdt, dev["rows"], A, eps=dev["eps"])
    assert same_bits(before["target_q"], dev["out"]["target_q"])
    ptrs = [list(p) for p in tdt.ptrs()]
    online = td.real_critic(S, A, H, L, seed=1).cuda()
    tau = 0.25
    with torch.no_grad():
        log_alpha.data.add_(0.5)
        for tp, p in zip(critic.parameters(), online.parameters()):
            tp.data.copy_(tau * p.data + (1 - tau) * tp.data)
    assert [list(p) for p in tdt.ptrs()] == ptrs               # in place: the same addresses
    after = run_td(tdt, dev["rows"], A, eps=dev["eps"])
    la = float(log_alpha[0])
    res, _ = chain_errors(case, after, log_alpha=la)
    for name, (err, bound) in res.items():
        assert (err <= bound).all(), (name, float((err / bound).max()))
    stale, _ = chain_errors(case, after, log_alpha=la - 0.5)
    assert (stale["target_q"][0] > stale["target_q"][1]).mean() > 0.5     # (done rows do not see alpha)
    ns = dev["rows"][:, S + A + 1:2 * S + A + 1].contiguous()
    q = torch.full((case["n"], 2), float("nan"), device="cuda")
    CriticKernel(critic)(ns, after["next_actions"], q)
    torch.cuda.synchronize()
    assert same_bits(after["next_q"], q)
    assert not bool((after["next_q"] == before["next_q"]).any())
    new = dict(case, critic=copy.deepcopy(critic).cpu(), log_alpha=log_alpha.cpu())
    ref = td.full(new)[0]["target_q"]
    g = td.torch_block(actor, critic, dev["rows"], dev["eps"], log_alpha, case["gamma"], S, A)[0]
    err_k = np.abs(after["target_q"].cpu().numpy().astype(np.float64) - ref).max()
    err_g = np.abs(g.cpu().numpy().astype(np.float64).reshape(-1) - ref).max()
    assert err_g > 0 and err_k <= REAL_C * err_g, (err_k, err_g)


# ------------------------------------------------------------------ 7. refusals and the fallback
def test_refusals_launch_nothing(pd):
    """Both exports refuse, before any launch (the output buffers keep their sentinel): S + A = 17,
    H = 64, L = 9, a misaligned parameter, and for pd_sac_td_target a wrong width, a NULL target_q
    with B > 0 and a NULL log_alpha.  pd_sac_critic splits as pd_sac_actor (a dimension out of range:
    PD_ERR_INVALID; a hidden width or an alignment: PD_ERR_UNSUPPORTED); pd_sac_td_target answers
    PD_ERR_UNSUPPORTED for everything outside the two nets' domains."""
    import torch
    from pdenv import _lib
    L_ = pd.load()
    vp = C.c_void_p
    INV, UNS = _lib.PD_ERR_INVALID, _lib.PD_ERR_UNSUPPORTED
    B = 32
    buf = torch.zeros(1 << 16, device="cuda")                   # every input pointer: readable zeros
    out = torch.full((B * 16,), SENTINEL, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    good = (vp * 20)(*([p] * 20))
    odd = (vp * 20)(*([p] * 20))
    odd[3] = p + 4

    def critic(S=2, A=1, H=256, nl=2, p1=good, p2=good):
        return L_.pd_sac_critic(B, S, A, H, nl, vp(p), vp(p), p1, p2, vp(out.data_ptr()), None)

    def target(S=2, A=1, width=None, ha=256, la=2, pa=good, hc=256, lc=2, p1=good, p2=good, log_alpha=vp(p),
               tq=vp(out.data_ptr())):
        width = 2 * S + A + 2 if width is None else width
        return L_.pd_sac_td_target(B, S, A, vp(p), width, ha, la, pa, -5.0, -1.0, 1.0, hc, lc, p1, p2, log_alpha,
                                   0.99, 0, 0, None, tq, None, None, None, None, None, None)

    assert critic(S=12, A=5) == INV and critic(S=16, A=1) == INV
    assert critic(H=64) == UNS and b"hidden" in L_.pd_last_error()
    assert critic(nl=9) == INV
    assert critic(p2=odd) == UNS and b"aligned" in L_.pd_last_error()
    assert critic(p1=odd) == UNS
    assert target(S=12, A=5) == UNS and target(S=16, A=1) == UNS
    assert target(hc=64) == UNS and target(ha=64) == UNS
    assert target(lc=9) == UNS and target(la=9) == UNS
    assert target(p1=odd) == UNS and target(pa=odd) == UNS and b"aligned" in L_.pd_last_error()
    assert target(width=8) == INV and b"width" in L_.pd_last_error()
    assert target(width=6) == INV
    assert target(tq=None) == INV
    assert target(log_alpha=None) == INV
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # an empty batch: PD_OK without a launch, whatever the data pointers are
    assert L_.pd_sac_critic(0, 2, 1, 256, 2, None, None, good, good, None, None) == _lib.PD_OK
    assert L_.pd_sac_td_target(0, 2, 1, None, 7, 256, 2, good, -5.0, -1.0, 1.0, 256, 2, good, good, vp(p), 0.99, 0, 0,
                               None, None, None, None, None, None, None, None) == _lib.PD_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_unsupported_critic_takes_the_torch_fallback(pd):
    """TdTarget on a critic the kernels do not cover (H = 64): the torch evaluation of the same block,
    with eps given and with the kernel's eps source restated in torch (pdenv.sac.td_eps)."""
    import torch
    from pdenv.sac import Actor, Critic, CriticKernel, TdTarget, td_eps
    S, A, B = 5, 4, 37
    torch.manual_seed(3)
    actor = Actor(S, A, hidden_dim=128, n_hidden_layers=2, log_std_min=-5.0, log_std_max=-1.0).cuda()
    critic = Critic(S, A, hidden_dim=64, n_hidden_layers=2).cuda()
    assert not CriticKernel.supported(critic)
    log_alpha = torch.full((1,), -0.7, device="cuda")
    tdt = TdTarget(actor, critic, log_alpha, 0.99, seed=11)
    assert not tdt.kernel
    rows = torch.rand(B, 2 * S + A + 2, device="cuda")
    rows[:, -1] = (torch.arange(B, device="cuda") % 3 == 0).float()
    eps = torch.randn(B, A, device="cuda")
    got = tdt(rows, eps=eps).clone()
    want = td.torch_block(actor, critic, rows, eps, log_alpha, 0.99, S, A)[0]
    assert got.shape == (B, 1) and torch.equal(got, want)
    drawn = torch.full((B, A), float("nan"), device="cuda")
    got = tdt(rows, draw=9, eps_out=drawn).clone()
    ref = td.np_eps(11, 9, B, A)
    e = drawn.cpu().numpy().astype(np.float64)
    assert (np.abs(e - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    assert torch.equal(drawn, td_eps(11, 9, B, A, rows.device))
    assert torch.equal(got, td.torch_block(actor, critic, rows, drawn, log_alpha, 0.99, S, A)[0])
    # and the same eps as the kernel path draws, to float32 rounding: a supported pair, same seed
    critic2 = Critic(S, A, hidden_dim=128, n_hidden_layers=2).cuda()
    k = run_td(TdTarget(actor, critic2, log_alpha, 0.99, seed=11), rows, A, draw=9)["eps_out"]
    assert (np.abs(k.cpu().numpy().astype(np.float64) - e) <= np.spacing(np.abs(ref).astype(np.float32))).all()


def test_buffers_expose_the_rows_of_the_last_sample(pd):
    import torch
    from pdenv.sac import DevicePrioritizedReplayBuffer, DeviceReplayBuffer, KernelPrioritizedReplayBuffer
    S, A = 2, 1
    slab = torch.rand(64, 2 * S + A + 2, device="cuda")
    for cls in (DeviceReplayBuffer, DevicePrioritizedReplayBuffer, KernelPrioritizedReplayBuffer):
        buf = cls(128, S, A, torch.device("cuda", 0))
        assert buf.last_rows is None
        buf.add_batch(slab)
        out = buf.sample(16)
        assert buf.last_rows.shape == (16, 2 * S + A + 2) and buf.last_rows.is_contiguous()
        assert torch.equal(torch.cat(out[:5], dim=1), buf.last_rows)


if __name__ == "__main__":     # python tests/test_gpu_sac_td.py OUT.json: the measurements alone
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "psso-sac-for-powered-descent_amd"))
    shapes = []
    for shape in td.SHAPES:
        k, g, c, top, margin = measure_real(*shape)
        res, _ = chain_errors(real_case(*shape), real_case(*shape)["dev"]["out"])
        row = dict(shape=list(shape), n=sn.N_REAL, err_k=k, err_g=g, err_c=c, ratio=k / max(g, c), max_abs_ref=top,
                   min_one_minus_a2=margin)
        for name, (err, bound) in res.items():
            row[name] = dict(max_err_ulp=float(err.max()), median_bound_ulp=float(np.median(bound)),
                             max_err_over_bound=float((err / bound).max()))
        shapes.append(row)
        print(row)
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(what="pd_sac_td_target, torch f32 on the GPU and torch f32 on the CPU against the binary64 "
                            "evaluation of the same float32 parameters and eps: max |target_q - ref64| over the rows; "
                            "and the kernel's elementwise chain against its binary64 model in float32 ulps",
                       bound_c=REAL_C, shapes=shapes), fh, indent=1)
        fh.write("\n")
