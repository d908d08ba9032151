"""pd_sac_critic_dinput and pd_sac_actor_grad (csrc/pdsacact.hip), pdenv.sac.ActorUpdate and
pdenv.sac.sac_update against references outside the kernels.

1. Exactly: integer Q nets and integer state | action -- pd_sac_critic_dinput's dsa must EQUAL the
   int64 model and q pd_sac_critic's; integer actor, integer observations and an integer dheads_in --
   every actor gradient tensor must EQUAL the int64 backward pass, also from wide rows.
2. The fused call equals its pieces bit for bit: heads pd_sac_actor's, new_actions and log_prob
   pd_sac_td_target's, q pd_sac_critic's, dq_da pd_sac_critic_dinput's action columns; dheads_out fed
   back as dheads_in gives the same gradients; the drawn eps is the NumPy Philox model's.
3. The elementwise chain: dheads_out and the three losses against the binary64 model on the kernel's
   own heads, q, dq_da and eps within the a-priori bound of sac_actor_grad_nets.elem_bound (derived in
   that module's docstring; nothing in it comes from the kernel's output), with and without weights, on
   rows built for the tie, both clamp sides, the exact bounds and saturation.
4. The whole gradient, real-valued, against binary64 autograd: per actor tensor max |grad - ref64| <=
   max(REAL_C err_torch, floor), REAL_C and the floor those of tests/test_gpu_sac_update.py test 3 with
   the same reasoning (err_torch the larger of torch's float32 autograd errors on the GPU and the CPU;
   floor = B 2**-24 max sum_b |terms|).  min and clamp make the loss non-differentiable where q1 = q2
   or raw = a bound, and a float32 flip there is not a rounding error: the fixture keeps the rows that
   stand 16 a-priori forward bounds away (sac_actor_grad_nets.real_case; its conditions are asserted
   on the CPU, tests/test_sac_actor_update_cpu.py).
5. Determinism: equal bits twice, the same gradients whichever optional outputs are asked for, a
   row's outputs independent of the batch it sits in.
6. ActorUpdate end to end on real torch.optim.Adams over five consecutive updates, each checked
   against the float64 torch block started from that update's own starting state (the argument of
   tests/test_gpu_sac_update.py test 6), the gradient bound test 4's carried through
   sac_grad_nets.adam_model; the state dict round trip; the torch fallback.
7. sac_update on a small KernelPrioritizedReplayBuffer equals its five pieces called by hand.

Measured (MI355X, `python tests/test_gpu_sac_actor_update.py OUT.json`):
profiles/sac_actor_update_shapes.json."""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import sac_actor_grad_nets as an
import sac_grad_nets as gn
import sac_nets as sn
import sac_td_nets as td

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5     # no integer: no gradient of an integer net equals it
GUARD = 16
REAL_C = 4.0            # tests/test_gpu_sac_update.py test 3
LO, HI = td.LOG_STD_MIN, td.LOG_STD_MAX
vp = C.c_void_p
OUTS = ("new_actions", "log_prob", "q", "heads", "eps_out", "dq_da", "dheads_out", "actor_loss", "alpha_loss",
        "log_alpha_grad", "partials")


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


def dev_list(params):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in params]


def run_actor(aparams, cparams, rows, n, S, A, H, L, HC=0, LC=0, weights=None, eps=None, dheads=None, log_alpha=None,
              te=None, ma=1.0, lo=LO, hi=HI, seed=0, draw=0, outs=OUTS, pitch=None):
    """One pd_sac_actor_grad call over the first n rows of rows [>= n][pitch] (device).  aparams: the
    actor's device tensors, cparams: the two nets' (None with dheads).  Every gradient tensor is a fresh
    buffer of numel + 16 floats filled with the sentinel, every output asked for is sentinel-filled with
    16 guard rows, 16 guard floats sit behind the scratch.  Returns dict of grads (flat views) and the
    outputs (views of n rows)."""
    import torch
    from pdenv import _lib
    lib = _lib.load()
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    gbufs = [full(p.numel() + GUARD) for p in aparams]
    np_ = an.n_partials(H, L)
    lens = dict(new_actions=(n, A), log_prob=(n,), q=(n, 2), heads=(n, 2 * A), eps_out=(n, A), dq_da=(n, 2 * A),
                dheads_out=(n, 2 * A), actor_loss=(1,), alpha_loss=(1,), log_alpha_grad=(1,), partials=(np_,))
    o = {k: (full(lens[k][0] + GUARD, *lens[k][1:]) if k in outs else None) for k in lens}
    nbytes = int(lib.pd_sac_actor_grad_scratch_bytes(n, A, H, L))
    assert nbytes == an.scratch_bytes(n, A, H, L)
    scratch = torch.empty(nbytes // 4 + GUARD, device="cuda")
    scratch[nbytes // 4:] = SENTINEL
    cnt = C.c_int32(np_)
    P = lambda t: None if t is None else vp(t.data_ptr())
    la = log_alpha if log_alpha is not None else torch.full((1,), an.LOG_ALPHA, device="cuda")
    st = lib.pd_sac_actor_grad(n, S, A, P(rows), int(rows.stride(0)) if pitch is None else pitch, P(weights), H, L,
                               ptr_list(aparams), ptr_list(gbufs), lo, hi, ma, HC, LC,
                               None if cparams is None else ptr_list(cparams[0]),
                               None if cparams is None else ptr_list(cparams[1]), P(la), -float(A) if te is None else te,
                               seed, draw, P(eps), P(dheads), P(o["new_actions"]), P(o["log_prob"]), P(o["q"]),
                               P(o["heads"]), P(o["eps_out"]), P(o["dq_da"]), P(o["dheads_out"]), P(o["actor_loss"]),
                               P(o["alpha_loss"]), P(o["log_alpha_grad"]), P(o["partials"]), C.byref(cnt),
                               vp(scratch.data_ptr()), nbytes, None)
    assert st == _lib.PD_OK, lib.pd_last_error()
    torch.cuda.synchronize()
    assert cnt.value == np_
    assert bool((scratch[nbytes // 4:] == SENTINEL).all()), "scratch written past its closed form"
    res = dict(grads=[b[:p.numel()] for b, p in zip(gbufs, aparams)])
    for k, (b, p) in enumerate(zip(gbufs, aparams)):
        assert bool((b[p.numel():] == SENTINEL).all()), f"tensor {k}: guard floats after the gradient were written"
        assert not bool((b[:p.numel()] == SENTINEL).any()), f"tensor {k}: gradient elements left unwritten"
    skipped = ("q", "dq_da", "actor_loss") if dheads is not None else ()
    for k, t in o.items():
        res[k] = None if t is None else t[:lens[k][0]]
        if t is None:
            continue
        assert bool((t[lens[k][0]:] == SENTINEL).all()), f"{k}: written past its end"
        if k in skipped:
            assert bool((t == SENTINEL).all()), f"{k}: written under dheads_in"
        else:
            assert not bool((t[:lens[k][0]] == SENTINEL).any()), f"{k}: elements left unwritten"
    return res


def run_dinput(cparams, sa, n, S, A, H, L, pitch=None):
    """One pd_sac_critic_dinput call: (q [n][2], dsa [n][2][S + A]) with guard rows checked."""
    import torch
    from pdenv import _lib
    lib = _lib.load()
    D = S + A
    q = torch.full((n + GUARD, 2), SENTINEL, device="cuda")
    dsa = torch.full((n + GUARD, 2, D), SENTINEL, device="cuda")
    st = lib.pd_sac_critic_dinput(n, S, A, H, L, vp(sa.data_ptr()), int(sa.stride(0)) if pitch is None else pitch,
                                  ptr_list(cparams[0]), ptr_list(cparams[1]), vp(q.data_ptr()), vp(dsa.data_ptr()), None)
    assert st == _lib.PD_OK, lib.pd_last_error()
    torch.cuda.synchronize()
    assert bool((q[n:] == SENTINEL).all()) and bool((dsa[n:] == SENTINEL).all()), "written past the batch"
    assert not bool((q[:n] == SENTINEL).any()) and not bool((dsa[:n] == SENTINEL).any())
    return q[:n], dsa[:n]


# ------------------------------------------------------------------ 1. exact
def check_dinput_exact(S, A, H, L, n):
    import torch
    from pdenv.sac import Critic, CriticKernel
    c = an.int_dinput_case(S, A, H, L, n=n)
    cparams = [dev_list(ps) for ps in c["params"]]
    sa = torch.full((n + GUARD, S + A), float("nan"), device="cuda")      # NaN rows behind the batch
    sa[:n] = torch.from_numpy(c["sa"]).cuda()
    q, dsa = run_dinput(cparams, sa, n, S, A, H, L)
    critic = td.load_critic(Critic(S, A, hidden_dim=H, n_hidden_layers=L), *c["params"]).cuda()
    qk = torch.full((n, 2), float("nan"), device="cuda")
    CriticKernel(critic)(sa[:n, :S].contiguous(), sa[:n, S:].contiguous(), qk)
    torch.cuda.synchronize()
    assert same_bits(q, qk), "q differs from pd_sac_critic's"
    assert np.array_equal(q.cpu().numpy(), c["q"])
    got = dsa.cpu().numpy()
    if not np.array_equal(got, c["dsa"]):
        bad = np.argwhere(got != c["dsa"])
        i = tuple(bad[0])
        raise AssertionError(f"{(S, A, H, L, n)}: {len(bad)} of {got.size} input gradients differ from the int64 model; "
                             f"first {i}: got {got[i]}, want {c['dsa'][i]}")


def check_actor_exact(S, A, H, L, n, wide=False):
    import torch
    c = an.int_actor_case(S, A, H, L, n=n)
    aparams = dev_list(c["params"])
    W = 2 * S + A + 2 if wide else S
    rows = torch.full((n + GUARD, W), float("nan"), device="cuda")
    rows[:n, :S] = torch.from_numpy(c["obs"]).cuda()
    dh = torch.full((n + GUARD, 2 * A), float("nan"), device="cuda")
    dh[:n] = torch.from_numpy(c["dheads"]).cuda()
    eps = torch.zeros(n, A, device="cuda")
    res = run_actor(aparams, None, rows, n, S, A, H, L, dheads=dh, eps=eps)
    assert np.array_equal(res["heads"].cpu().numpy(), c["heads"])
    assert same_bits(res["dheads_out"], dh[:n])
    total = 0.0
    for k, (got, want) in enumerate(zip(res["grads"], c["grads"])):
        got = got.cpu().numpy().reshape(want.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            i = tuple(bad[0])
            raise AssertionError(f"{(S, A, H, L, n)} tensor {k}: {len(bad)} of {want.size} gradient values differ from "
                                 f"the int64 backward pass; first {i}: got {got[i]}, want {want[i]}")
        total += float((want.astype(np.float64) ** 2).sum())
    got = float(res["partials"].double().sum())
    assert abs(got - total) <= 1e-5 * total, (got, total)
    return c


@pytest.mark.parametrize("n", an.BATCHES)
@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_N)
def test_integer_nets_exact(pd, S, A, H, L, n):
    check_dinput_exact(S, A, H, L, n)
    check_actor_exact(S, A, H, L, n)


@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_DEEP)
def test_integer_nets_exact_deep(pd, S, A, H, L):
    check_dinput_exact(S, A, H, L, sn.N_EXACT)
    check_actor_exact(S, A, H, L, sn.N_EXACT)


@pytest.mark.parametrize("S,A,H,L", an.SHAPES_WIDE)
def test_actor_alone_exact_above_16_inputs(pd, S, A, H, L):
    """Under dheads_in there is no critic, and the domain is the actor's: S <= 16 and A <= 8, so S + A may
    exceed the 16 inputs of a Q net.  The gradients, the heads and the forward outputs' guards at such
    shapes (the kernel must not stage state | action for a critic it does not run)."""
    import torch
    assert S + A > 16
    check_actor_exact(S, A, H, L, sn.N_EXACT)
    # and the sample of such a shape is the per-row sample: new_actions and log_prob of the first 17 rows
    # do not depend on the batch
    c = an.int_actor_case(S, A, H, L)
    aparams = dev_list(c["params"])
    rows = torch.from_numpy(c["obs"]).cuda()
    dh = torch.from_numpy(c["dheads"]).cuda()
    eps = torch.from_numpy(np.random.default_rng([S, A]).standard_normal((sn.N_EXACT, A)).astype(np.float32)).cuda()
    big = run_actor(aparams, None, rows, sn.N_EXACT, S, A, H, L, dheads=dh, eps=eps)
    small = run_actor(aparams, None, rows, 17, S, A, H, L, dheads=dh, eps=eps)
    for k in ("new_actions", "log_prob", "heads", "eps_out"):
        assert same_bits(small[k], big[k][:17]), k
    m = an.elem(big["heads"].cpu().numpy(), eps.cpu().numpy(), np.zeros((sn.N_EXACT, 2)), np.zeros((sn.N_EXACT, 2, A)), None,
                LO, HI, 1.0, an.LOG_ALPHA, -float(A))
    E = an.elem_bound(m)
    assert (np.abs(big["log_prob"].cpu().numpy() - m["log_prob"]) <= E["log_prob"]).all()
    assert (np.abs(big["new_actions"].cpu().numpy() - m["new_actions"]) <= E["new_actions"]).all()


def test_gradients_from_wide_rows(pd):
    """pitch = 2S + A + 2, the buffer's row width: the same gradients, the other columns NaN; and
    pd_sac_critic_dinput from rows with a pitch."""
    import torch
    S, A, H, L = 2, 1, 256, 2
    check_actor_exact(S, A, H, L, sn.N_EXACT, wide=True)
    c = an.int_dinput_case(S, A, H, L)
    rows = torch.full((sn.N_EXACT + GUARD, 2 * S + A + 2), float("nan"), device="cuda")
    rows[:sn.N_EXACT, :S + A] = torch.from_numpy(c["sa"]).cuda()
    _, dsa = run_dinput([dev_list(ps) for ps in c["params"]], rows, sn.N_EXACT, S, A, H, L)
    assert np.array_equal(dsa.cpu().numpy(), c["dsa"])


# ------------------------------------------------------------------ the real-valued cases
_real = {}


def real_dev(S, A, H, L):
    """The real-valued case of a shape on the device (once, never modified): sac_actor_grad_nets.real_case
    plus device copies of the nets, rows, eps, weights, log_alpha and ONE pd_sac_actor_grad call at n =
    261 with PER weights, eps_in and every output."""
    import torch
    key = (S, A, H, L)
    if key not in _real:
        case = an.real_case(S, A, H, L)
        actor, critic = copy.deepcopy(case["actor"]).cuda(), copy.deepcopy(case["critic"]).cuda()
        aparams = [t.data for t in actor_tensors(actor)]
        cparams = [[t for m in td.q_linears(net) for t in (m.weight.data, m.bias.data)] for net in (critic.q1, critic.q2)]
        dev = dict(actor=actor, critic=critic, aparams=aparams, cparams=cparams, rows=torch.from_numpy(case["rows"]).cuda(),
                   eps=torch.from_numpy(case["eps"]).cuda(), weights=torch.from_numpy(case["weights"]).cuda(),
                   log_alpha=torch.full((1,), case["log_alpha"], device="cuda"))
        dev["out"] = run_actor(aparams, cparams, dev["rows"], case["n"], S, A, H, L, H, L, weights=dev["weights"],
                               eps=dev["eps"], log_alpha=dev["log_alpha"], ma=actor.max_action)
        _real[key] = dict(case, dev=dev)
    return _real[key]


def actor_tensors(actor):
    import torch.nn as nn
    lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)] + [actor.mean, actor.log_std]
    return [t for m in lins for t in (m.weight, m.bias)]


# ------------------------------------------------------------------ 2. fused equals pieces
@pytest.mark.parametrize("S,A,H,L", an.SHAPES)
def test_fused_equals_its_pieces(pd, S, A, H, L):
    import torch
    from pdenv.sac import ActorKernel, CriticKernel, TdTarget
    case = real_dev(S, A, H, L)
    dev, n = case["dev"], case["n"]
    out = dev["out"]
    states = dev["rows"][:, :S].contiguous()
    heads = torch.full((n, 2 * A), float("nan"), device="cuda")
    ActorKernel(dev["actor"])(states, heads)
    assert same_bits(out["heads"], heads), "heads differ from pd_sac_actor's"
    # pd_sac_td_target on rows whose next_state is the state, the same eps
    rows2 = dev["rows"].clone()
    rows2[:, S + A + 1:2 * S + A + 1] = states
    na, lp = torch.full((n, A), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    TdTarget(dev["actor"], dev["critic"], dev["log_alpha"], 0.99)(rows2, eps=dev["eps"], next_actions=na, next_log_prob=lp)
    assert same_bits(out["new_actions"], na) and same_bits(out["log_prob"], lp)
    assert same_bits(out["eps_out"], dev["eps"])
    q = torch.full((n, 2), float("nan"), device="cuda")
    CriticKernel(dev["critic"])(states, out["new_actions"].contiguous(), q)
    assert same_bits(out["q"], q), "q differs from pd_sac_critic's"
    sa = torch.cat([states, out["new_actions"]], dim=1).contiguous()
    q2, dsa = run_dinput(dev["cparams"], sa, n, S, A, H, L)
    assert same_bits(q2, q) and same_bits(out["dq_da"].reshape(n, 2, A), dsa[:, :, S:])
    # dheads_out fed back as dheads_in: the same gradient bits, no critic
    back = run_actor(dev["aparams"], None, dev["rows"], n, S, A, H, L, weights=dev["weights"], eps=dev["eps"],
                     dheads=out["dheads_out"].contiguous(), log_alpha=dev["log_alpha"], ma=dev["actor"].max_action)
    for a, b in zip(out["grads"], back["grads"]):
        assert same_bits(a, b)
    for k in ("partials", "alpha_loss", "log_alpha_grad", "log_prob", "new_actions", "heads"):
        assert same_bits(out[k], back[k]), k


def test_drawn_eps_is_the_philox_model(pd):
    import torch
    S, A, H, L = 5, 4, 256, 3
    case = real_dev(S, A, H, L)
    dev = case["dev"]
    seed, draw, n = 0x1234567890ABCDEF, 0x100000003, 37
    run = lambda nn, **kw: run_actor(dev["aparams"], dev["cparams"], dev["rows"], nn, S, A, H, L, H, L,
                                     log_alpha=dev["log_alpha"], **kw)
    a = run(n, seed=seed, draw=draw)
    ref = an.np_eps(seed, draw, n, A)
    got = a["eps_out"].cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - ref) <= ulp).all(), float((np.abs(got - ref) / ulp).max())
    assert (got == ref.astype(np.float32)).mean() > 0.99
    assert same_bits(run(17, seed=seed, draw=draw)["eps_out"], a["eps_out"][:17])
    assert not bool((run(n, seed=seed, draw=draw + 1)["eps_out"] == a["eps_out"]).any())
    # the TD target's draws under the same (seed, draw) are other numbers (tag 64 there, 72 here)
    assert not (got == td.np_eps(seed, draw, n, A).astype(np.float32)).any()
    # and eps_in = the drawn eps gives the drawn call's bits
    b = run(n, eps=a["eps_out"].contiguous())
    for k in ("new_actions", "log_prob", "q", "dheads_out", "actor_loss"):
        assert same_bits(a[k], b[k]), k


# ------------------------------------------------------------------ 3. the elementwise chain
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("S,A,H,L", [(2, 1, 256, 2), (5, 4, 256, 3)])
def test_elementwise_chain_within_the_a_priori_bound(pd, S, A, H, L, per):
    """The corners are built into the call.  The tie: a call whose two nets are both given Q1's
    parameters, so every row ties (sel = 1/2 each); the calls with the two nets cover either net being
    the smaller.  The clamp: the call's bounds are set from the kernel's own float32 raw log_std of rows
    2 and 5 (component 0) -- exactly at them (those rows sit AT a bound: inside), one ulp inwards
    (outside) and one ulp outwards (inside) -- and the other rows fall on both sides of both bounds.
    Saturation: rows 7 and 8 get eps = +-2000, so a = +-1 exactly."""
    import torch
    case = real_dev(S, A, H, L)
    dev, n = case["dev"], case["n"]
    raw = dev["out"]["heads"][:, A:].cpu().numpy()
    eps = dev["eps"].clone()
    eps[7], eps[8] = 2000.0, -2000.0
    w = dev["weights"] if per else None
    f = np.float32
    worst = {}
    # the clamp bounds as float32 numbers around chosen rows' raw log_std (component 0): lo at row 2's
    # value (row 2 AT the lower bound), then nudged one ulp either way; the same for hi at row 5
    r_lo, r_hi = sorted([float(raw[2, 0]), float(raw[5, 0])])
    variants = [(r_lo, r_hi), (float(np.nextafter(f(r_lo), f(np.inf))), float(np.nextafter(f(r_hi), f(-np.inf)))),
                (float(np.nextafter(f(r_lo), f(-np.inf))), float(np.nextafter(f(r_hi), f(np.inf))))]
    seen_inside = set()
    for tie in (False, True):
        cparams = [dev["cparams"][0], dev["cparams"][0]] if tie else dev["cparams"]
        for lo, hi in (variants if not tie else variants[:1]):
            res = run_actor(dev["aparams"], cparams, dev["rows"], n, S, A, H, L, H, L, weights=w, eps=eps,
                            log_alpha=dev["log_alpha"], ma=dev["actor"].max_action, lo=lo, hi=hi)
            g = {k: res[k].cpu().numpy() for k in ("heads", "eps_out", "q", "dq_da", "dheads_out", "new_actions", "log_prob")}
            m = an.elem(g["heads"], g["eps_out"], g["q"], g["dq_da"].reshape(n, 2, A), case["weights"] if per else None,
                        lo, hi, dev["actor"].max_action, case["log_alpha"], case["target_entropy"])
            E = an.elem_bound(m)
            if tie:
                assert (g["q"][:, 0] == g["q"][:, 1]).all() and (m["sel"] == 0.5).all()
            else:
                assert (m["sel"][:, 0] == 1).any() and (m["sel"][:, 1] == 1).any()
            for r in (2, 5):
                seen_inside.add((r, bool(m["inside"][r, 0])))
            assert not m["inside"].all() and m["inside"].any()
            assert (np.abs(g["new_actions"][7:9]) == dev["actor"].max_action).all()          # saturated: a = +-1
            for name, got, want, bound in (("dheads", g["dheads_out"], m["dheads"], E["dheads"]),
                                           ("log_prob", g["log_prob"], m["log_prob"], E["log_prob"]),
                                           ("new_actions", g["new_actions"], m["new_actions"], E["new_actions"])):
                err = np.abs(got.astype(np.float64) - want)
                ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert (err <= bound).all(), (name, tie, lo, hi, ratio)
            for name in ("actor_loss", "alpha_loss", "log_alpha_grad"):
                err = abs(float(res[name][0]) - m[name])
                worst[name] = max(worst.get(name, 0.0), err / E[name])
                assert err <= E[name], (name, tie, err, E[name])
            # outside the clamp the log_std head gets exactly nothing
            assert (g["dheads_out"][:, A:][~m["inside"]] == 0).all()
    assert seen_inside == {(2, True), (2, False), (5, True), (5, False)}      # at the bound inside, one ulp off outside
    print(f"{(S, A, H, L)} per {per}: worst err/bound {worst}")


# ------------------------------------------------------------------ 4. the whole gradient
def measure_real(S, A, H, L):
    """Per actor tensor: (err_k, err_torch, floor, max |ref|) against float64 autograd (the NumPy model,
    which tests/test_sac_actor_update_cpu.py holds to torch's float64 autograd)."""
    import torch
    case = real_dev(S, A, H, L)
    dev, ref = case["dev"], case["ref"]
    a64, c64 = copy.deepcopy(case["actor"]).double(), copy.deepcopy(case["critic"]).double()
    rows, eps, w = (torch.from_numpy(case[k]) for k in ("rows", "eps", "weights"))
    la = torch.full((1,), case["log_alpha"])
    r64 = an.torch_block(a64, c64, rows[:, :S].double(), eps.double(), w.double(), la.double(), case["target_entropy"])
    g_cpu = an.torch_block(copy.deepcopy(case["actor"]), copy.deepcopy(case["critic"]), rows[:, :S], eps, w, la,
                           case["target_entropy"])
    g_gpu = an.torch_block(copy.deepcopy(dev["actor"]), copy.deepcopy(dev["critic"]), dev["rows"][:, :S], dev["eps"],
                           dev["weights"], dev["log_alpha"], case["target_entropy"])
    got = [g.cpu().numpy().astype(np.float64) for g in dev["out"]["grads"]]
    out = []
    for k, r in enumerate(r64["grads"]):
        assert np.abs(ref["grads"][k] - r).max() <= 1e-9 * max(1.0, np.abs(r).max())
        err_k = float(np.abs(got[k].reshape(r.shape) - r).max())
        err_t = max(float(np.abs(g_gpu["grads"][k] - r).max()), float(np.abs(g_cpu["grads"][k] - r).max()))
        out.append((err_k, err_t, case["n"] * gn.EPS32 * ref["terms"][k], float(np.abs(r).max())))
    return out


@pytest.mark.parametrize("S,A,H,L", an.SHAPES)
def test_gradient_error_within_torch_f32_error(pd, S, A, H, L):
    case = real_dev(S, A, H, L)
    assert case["clamped"] > 0 and case["unclamped"] > 0
    # the kernel stands on the model's side of every kink at the kept rows
    out, ref = case["dev"]["out"], case["ref"]
    q = out["q"].cpu().numpy()
    assert ((q[:, 0] < q[:, 1]) == (ref["q"][:, 0] < ref["q"][:, 1])).all()
    raw = out["heads"][:, A:].cpu().numpy()
    assert (((raw >= LO) & (raw <= HI)) == ref["inside"]).all()
    res = measure_real(S, A, H, L)
    for k, (err_k, err_t, floor, top) in enumerate(res):
        print(f"{(S, A, H, L)} tensor {k}: err_k {err_k:.3e} err_torch {err_t:.3e} floor {floor:.3e} max |ref| {top:.3g} "
              f"ratio {err_k / max(err_t, 1e-300):.2f}")
    assert max(top for _, _, _, top in res) > 1e-4
    for k, (err_k, err_t, floor, top) in enumerate(res):
        assert err_k <= max(REAL_C * err_t, floor), (k, err_k, err_t, floor)


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_N)
def test_determinism(pd, S, A, H, L):
    case = real_dev(S, A, H, L)
    dev, n = case["dev"], case["n"]
    first = dev["out"]
    kw = dict(weights=dev["weights"], eps=dev["eps"], log_alpha=dev["log_alpha"], ma=dev["actor"].max_action)
    again = run_actor(dev["aparams"], dev["cparams"], dev["rows"], n, S, A, H, L, H, L, **kw)
    for a, b in zip(first["grads"], again["grads"]):
        assert same_bits(a, b)
    for k in OUTS:
        assert same_bits(first[k], again[k]), k
    bare = run_actor(dev["aparams"], dev["cparams"], dev["rows"], n, S, A, H, L, H, L, outs=(), **kw)
    for a, b in zip(first["grads"], bare["grads"]):
        assert same_bits(a, b)
    # a row's outputs do not depend on the batch it sits in (the loss coefficients hold 1 / B: under
    # dheads_in for dheads_out, and for the forward outputs in any case)
    dh = first["dheads_out"].contiguous()
    kw2 = dict(eps=dev["eps"], log_alpha=dev["log_alpha"], ma=dev["actor"].max_action)
    big = run_actor(dev["aparams"], None, dev["rows"], n, S, A, H, L, dheads=dh, **kw2)
    small = run_actor(dev["aparams"], None, dev["rows"], 37, S, A, H, L, dheads=dh, **kw2)
    for k in ("new_actions", "log_prob", "heads", "eps_out", "dheads_out"):
        assert same_bits(small[k], big[k][:37]), k
    small_q = run_actor(dev["aparams"], dev["cparams"], dev["rows"], 37, S, A, H, L, H, L, **kw2)
    for k in ("q", "dq_da", "new_actions", "log_prob"):
        assert same_bits(small_q[k], first[k][:37]), k


# ------------------------------------------------------------------ 6. ActorUpdate end to end
LR, LR_ALPHA, BETAS, EPS_ADAM = 3e-4, 1e-3, (0.9, 0.999), 1e-8


def to_np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def torch_update(actor, critic, la, opt, aopt, rows, eps, w, S, te, max_norm):
    """Steps 4 to 6 of SACPyTorch.update in the tensors' dtype (sac_pytorch.py:485-521): the gradients
    by sac_actor_grad_nets.torch_block, then clip and the optimizers' own steps."""
    import torch
    import torch.nn as nn
    r = an.torch_block(actor, critic, rows[:, :S], eps, w, la.detach(), te)
    norm = None
    if max_norm is not None:
        norm = float(nn.utils.clip_grad_norm_(actor.parameters(), max_norm=max_norm))
    opt.step()
    if aopt is not None:
        la.grad = torch.full_like(la, r["log_alpha_grad"])
        aopt.step()
    return r, norm


@pytest.mark.parametrize("mode", ["clip_above_per_alpha", "clip_below_noper_alpha", "noclip_per_noalpha"])
def test_actor_update_end_to_end(pd, mode):
    import torch
    from pdenv.sac import ActorUpdate
    S, A, H, L, B = 2, 1, 256, 2, 256
    case = an.real_case(S, A, H, L)
    actor, critic = copy.deepcopy(case["actor"]).cuda(), copy.deepcopy(case["critic"]).cuda()
    la = torch.full((1,), -1.0, device="cuda", requires_grad=True)
    per, tune = "noper" not in mode, "noalpha" not in mode
    opt = torch.optim.Adam(actor.parameters(), lr=LR)
    aopt = torch.optim.Adam([la], lr=LR_ALPHA) if tune else None
    # the gradient norm of this case is measured once in float64 and the clip set around it
    probe = an.torch_block(copy.deepcopy(case["actor"]).double(), copy.deepcopy(case["critic"]).double(),
                           torch.from_numpy(case["rows"][:B, :S]).double(), torch.from_numpy(case["eps"][:B]).double(),
                           torch.from_numpy(case["weights"][:B]).double() if per else None, torch.full((1,), -1.0).double(),
                           -float(A))
    norm0 = float(np.sqrt(sum((g ** 2).sum() for g in probe["grads"])))
    max_norm = dict(clip_above_per_alpha=0.25 * norm0, clip_below_noper_alpha=50.0 * norm0, noclip_per_noalpha=None)[mode]
    assert ActorUpdate.supported(actor, critic, la, opt, aopt)
    upd = ActorUpdate(actor, critic, la, opt, aopt, max_grad_norm=max_norm, seed=3)
    assert upd.kernel and upd.target_entropy == -float(A)
    params = actor_tensors(actor)
    ptrs = [p.data_ptr() for p in params]
    rng = np.random.default_rng(7)
    for p in critic.parameters():
        p.grad = torch.full_like(p, 3.0)                      # the critic's p.grad is not this step's
    for it in range(5):
        idx = rng.permutation(case["n"])[:B]
        rows = torch.from_numpy(case["rows"][idx]).cuda()
        eps = torch.from_numpy(case["eps"][idx]).cuda()
        w = torch.from_numpy(case["weights"][idx]).cuda() if per else None
        # ---- the state this update starts from, as float64 copies on the CPU
        a64, c64 = copy.deepcopy(actor).cpu().double(), copy.deepcopy(critic).cpu().double()
        la64 = la.detach().cpu().double().clone().requires_grad_(True)
        o64 = torch.optim.Adam(a64.parameters(), lr=LR)
        ao64 = torch.optim.Adam([la64], lr=LR_ALPHA) if tune else None
        for src, dst in ((opt, o64), (aopt, ao64)):
            if it > 0 and src is not None:
                sd = copy.deepcopy(src.state_dict())
                for s in sd["state"].values():
                    s["exp_avg"], s["exp_avg_sq"] = s["exp_avg"].cpu().double(), s["exp_avg_sq"].cpu().double()
                dst.load_state_dict(sd)
        zeros = lambda: [np.zeros_like(x) for x in to_np(params)]
        before = dict(p=to_np(params), m=zeros() if it == 0 else to_np([opt.state[p]["exp_avg"] for p in params]),
                      v=zeros() if it == 0 else to_np([opt.state[p]["exp_avg_sq"] for p in params]), la=float(la.detach()))
        if tune:
            before.update(la_m=0.0 if it == 0 else float(aopt.state[la]["exp_avg"]),
                          la_v=0.0 if it == 0 else float(aopt.state[la]["exp_avg_sq"]))
        # float64 gradients, torch's float32 gradients at the same state on both devices, test 4's bound
        cw = None if w is None else w.cpu()
        g32 = an.torch_block(copy.deepcopy(actor), copy.deepcopy(critic), rows[:, :S], eps, w, la.detach(), -float(A))
        g32c = an.torch_block(copy.deepcopy(actor).cpu(), copy.deepcopy(critic).cpu(), rows[:, :S].cpu(), eps.cpu(), cw,
                              la.detach().cpu(), -float(A))
        model = an.full(to_np(params), td.critic_params(copy.deepcopy(critic).cpu()), rows[:, :S].cpu().numpy(),
                        eps.cpu().numpy(), None if w is None else cw.numpy(), LO, HI, actor.max_action, before["la"], -float(A))
        # ---- the kernel's update and the float64 block from the same state
        lp = upd(rows, w, eps=eps).clone()
        torch.cuda.synchronize()
        r64, norm64 = torch_update(a64, c64, la64, o64, ao64, rows.cpu().double()[:, :], eps.cpu().double(),
                                   None if w is None else cw.double(), S, -float(A), max_norm)
        g64 = r64["grads"]
        assert [p.data_ptr() for p in params] == ptrs
        E_g = [max(REAL_C * max(float(np.abs(a - r).max()), float(np.abs(b - r).max())), B * gn.EPS32 * t)
               for a, b, r, t in zip(g32["grads"], g32c["grads"], g64, model["terms"])]
        parts = [float((x ** 2).sum()) for x in g64]
        tot = float(np.sqrt(sum(parts)))
        extra = float(np.sqrt(sum(e ** 2 * x.size for e, x in zip(E_g, g64)))) + 24 * gn.EPS32 * tot
        am = gn.adam_model(before["p"], g64, before["m"], before["v"], it + 1, LR, BETAS[0], BETAS[1], EPS_ADAM,
                           max_norm or 0.0, parts if max_norm else None, E_g=E_g, sum_terms=upd.n_partials,
                           E_total_extra=extra)
        if max_norm is not None:
            assert abs(am["norm"] - norm64) <= 1e-12 * norm64
            assert abs(float(upd.grad_norm) - norm64) <= am["E_norm"]
            if "above" in mode and it == 0:
                assert norm64 > max_norm
            if "below" in mode:
                assert norm64 < max_norm and am["coef"] == 1.0
        else:
            assert upd.grad_norm is None
        got = dict(p=to_np(params), m=to_np([opt.state[p]["exp_avg"] for p in params]),
                   v=to_np([opt.state[p]["exp_avg_sq"] for p in params]))
        p64 = actor_tensors(a64)
        ref = dict(p=to_np(p64), m=to_np([o64.state[p]["exp_avg"] for p in p64]),
                   v=to_np([o64.state[p]["exp_avg_sq"] for p in p64]))
        worst = {}
        for name in ("p", "m", "v"):
            for k in range(len(ref["p"])):
                bound = am["E_" + name][k] + np.abs(am[name][k].reshape(ref[name][k].shape) - ref[name][k])
                err = np.abs(got[name][k].astype(np.float64) - ref[name][k])
                worst[name] = max(worst.get(name, 0.0), float(np.max(err / np.maximum(bound, 1e-300))))
                assert (err <= bound).all(), (it, name, k, float(np.max(err / np.maximum(bound, 1e-300))))
        # ---- the losses and the temperature: test 3's bound on the kernel's own intermediate values is
        # test 3's business; here against the float64 block with the forward pass's float32 error taken
        # from torch's own float32 evaluations (REAL_C times, as for the gradients)
        for name in ("actor_loss", "alpha_loss"):
            tol = REAL_C * max(abs(g32[name] - r64[name]), abs(g32c[name] - r64[name])) + 64 * gn.EPS32 * (1 + abs(r64[name]))
            if name == "alpha_loss" and not tune:
                assert float(getattr(upd, name)) == 0.0
            else:
                assert abs(float(getattr(upd, name)) - r64[name]) <= tol, (it, name)
        # (the returned tensors' plumbing: their bits are test 2's, their error test 3's)
        assert np.abs(lp[:, 0].cpu().numpy() - r64["log_prob"]).max() <= 1e-3 and lp.shape == (B, 1)
        assert upd.new_actions.shape == (B, A) and upd.q.shape == (B, 2)
        if tune:
            E_ga = REAL_C * max(abs(g32["log_alpha_grad"] - r64["log_alpha_grad"]),
                                abs(g32c["log_alpha_grad"] - r64["log_alpha_grad"])) + 64 * gn.EPS32 * (1 + abs(r64["log_alpha_grad"]))
            assert abs(float(la.grad) - r64["log_alpha_grad"]) <= E_ga
            lm = gn.adam_model([np.float32([before["la"]])], [np.array([r64["log_alpha_grad"]])], [np.float32([before["la_m"]])],
                               [np.float32([before["la_v"]])], it + 1, LR_ALPHA, BETAS[0], BETAS[1], EPS_ADAM, E_g=[E_ga])
            bound = float(lm["E_p"][0][0]) + abs(float(lm["p"][0][0]) - float(la64.detach()))
            assert abs(float(la.detach()) - float(la64.detach())) <= bound, (it, float(la.detach()), float(la64.detach()), bound)
            assert float(la.detach()) != before["la"]
            assert int(aopt.state[la]["step"].item()) == it + 1
        else:
            assert float(la.detach()) == -1.0 and la.grad is None
        assert int(opt.state[params[0]]["step"].item()) == it + 1
        print(f"{mode} update {it}: worst err/bound {worst}, actor_loss {float(upd.actor_loss):.6g}")
    for p in critic.parameters():
        assert bool((p.grad == 3.0).all())
    # ---- the state dicts load into fresh torch Adams, which continue with torch's own step
    twin = copy.deepcopy(actor)
    fresh = torch.optim.Adam(twin.parameters(), lr=LR)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))
    for p, q in zip(actor.parameters(), twin.parameters()):
        assert same_bits(opt.state[p]["exp_avg"], fresh.state[q]["exp_avg"]) and float(fresh.state[q]["step"]) == 5
    la_t = la.detach().clone().requires_grad_(True)
    fresh_a = None
    if tune:
        fresh_a = torch.optim.Adam([la_t], lr=LR_ALPHA)
        fresh_a.load_state_dict(copy.deepcopy(aopt.state_dict()))
        assert float(fresh_a.state[la_t]["step"]) == 5
    rows, eps = torch.from_numpy(case["rows"][:B]).cuda(), torch.from_numpy(case["eps"][:B]).cuda()
    w = torch.from_numpy(case["weights"][:B]).cuda() if per else None
    before6 = [p.detach().clone() for p in actor.parameters()]
    torch_update(twin, copy.deepcopy(critic), la_t, fresh, fresh_a, rows, eps, w, S, -float(A), max_norm)
    upd(rows, w, eps=eps)
    torch.cuda.synchronize()
    for p, q, b in zip(actor.parameters(), twin.parameters(), before6):
        # one Adam step moves a parameter by at most 1.2 lr at t = 6 (tests/test_gpu_sac_update.py)
        assert bool(torch.isfinite(q).all()) and not torch.equal(p, b)
        assert float((p - q).detach().abs().max()) <= 2.5 * LR
    if tune:
        assert abs(float(la.detach()) - float(la_t.detach())) <= 2.5 * LR_ALPHA


def test_actor_update_backward_and_fallback(pd):
    """backward() alone leaves the gradients in p.grad (overwritten) and touches no optimizer; an actor
    outside the shapes (hidden 64) or a float64 log_alpha takes the torch path and returns the same
    things, within float32 tolerance of the float64 block."""
    import torch
    from pdenv.sac import Actor, ActorUpdate, Critic
    S, A, H, L = 5, 4, 256, 3
    case = real_dev(S, A, H, L)
    dev, n = case["dev"], case["n"]
    actor = copy.deepcopy(dev["actor"])
    la = dev["log_alpha"].clone().requires_grad_(True)
    opt, aopt = torch.optim.Adam(actor.parameters(), lr=LR), torch.optim.Adam([la], lr=LR_ALPHA)
    upd = ActorUpdate(actor, dev["critic"], la, opt, aopt, max_grad_norm=1.0)
    assert upd.kernel
    for p in actor.parameters():
        p.grad = torch.full_like(p, 7.0)
    dh = torch.full((n, 2 * A), float("nan"), device="cuda")
    lp = upd.backward(dev["rows"], dev["weights"], eps=dev["eps"], dheads_out=dh)
    torch.cuda.synchronize()
    out = dev["out"]
    for p, g in zip(actor_tensors(actor), out["grads"]):
        assert same_bits(p.grad.reshape(-1), g)
    assert same_bits(lp.reshape(-1), out["log_prob"]) and same_bits(upd.q, out["q"]) and same_bits(dh, out["dheads_out"])
    assert same_bits(upd.new_actions, out["new_actions"]) and same_bits(upd.actor_loss, out["actor_loss"])
    assert same_bits(upd.alpha_loss, out["alpha_loss"]) and same_bits(la.grad, out["log_alpha_grad"])
    assert len(opt.state) == 0 and len(aopt.state) == 0
    # ---- the fallbacks: hidden 64, and a float64 log_alpha (the reference's construction)
    B = 37
    rows, eps, w = dev["rows"][:B], dev["eps"][:B], dev["weights"][:B]
    for which in ("hidden64", "log_alpha64"):
        torch.manual_seed(3)
        small = Actor(S, A, hidden_dim=64 if which == "hidden64" else 128, log_std_min=LO, log_std_max=HI).cuda()
        crit = Critic(S, A, hidden_dim=128).cuda()
        la2 = (torch.tensor(np.log(0.2), device="cuda") if which == "log_alpha64"
               else torch.full((1,), -1.0, device="cuda")).requires_grad_(True)
        assert (la2.dtype == torch.float64) == (which == "log_alpha64")
        o2, ao2 = torch.optim.Adam(small.parameters(), lr=LR), torch.optim.Adam([la2], lr=LR_ALPHA)
        why = ActorUpdate.reasons(small, crit, la2, o2, ao2)
        assert why == (["actor"] if which == "hidden64" else ["log_alpha"]), why
        fb = ActorUpdate(small, crit, la2, o2, ao2, max_grad_norm=0.5)
        assert not fb.kernel
        a64, c64 = copy.deepcopy(small).cpu().double(), copy.deepcopy(crit).cpu().double()
        l64 = la2.detach().cpu().double().clone().requires_grad_(True)
        o64, ao64 = torch.optim.Adam(a64.parameters(), lr=LR), torch.optim.Adam([l64], lr=LR_ALPHA)
        lp = fb(rows, w, eps=eps)
        r64, norm64 = torch_update(a64, c64, l64, o64, ao64, rows.cpu().double(), eps.cpu().double(), w.cpu().double(), S,
                                   -float(A), 0.5)
        assert lp.shape == (B, 1) and fb.new_actions.shape == (B, A) and fb.q.shape == (B, 2)
        assert fb.actor_loss.shape == (1,) and fb.alpha_loss.shape == (1,) and fb.grad_norm.shape == (1,)
        assert np.abs(lp[:, 0].cpu().numpy() - r64["log_prob"]).max() <= 1e-4 * max(1.0, np.abs(r64["log_prob"]).max())
        assert np.abs(fb.q.cpu().numpy() - r64["q"]).max() <= 1e-4 * max(1.0, np.abs(r64["q"]).max())
        for name in ("actor_loss", "alpha_loss"):
            assert abs(float(getattr(fb, name)) - r64[name]) <= 1e-4 * max(1.0, abs(r64[name])), name
        assert abs(float(fb.grad_norm) - norm64) <= 1e-3 * norm64
        for p, q in zip(small.parameters(), a64.parameters()):
            # one Adam step each way from the same state: within 2.5 lr (tests/test_gpu_sac_update.py)
            assert float((p.detach().cpu().double() - q.detach()).abs().max()) <= 2.5 * LR
        assert abs(float(la2.detach()) - float(l64.detach())) <= 2.5 * LR_ALPHA
        assert float(la2.detach()) != float(np.log(0.2) if which == "log_alpha64" else -1.0)
        # the drawn eps of the fallback is the kernel's, to float32 rounding
        drawn = torch.full((B, A), float("nan"), device="cuda")
        fb.backward(rows, w, draw=9, eps_out=drawn)
        refe = an.np_eps(0, 9, B, A)
        assert (np.abs(drawn.cpu().numpy().astype(np.float64) - refe) <= np.spacing(np.abs(refe).astype(np.float32))).all()


# ------------------------------------------------------------------ 7. sac_update
def test_sac_update_equals_its_pieces(pd):
    import torch
    from pdenv.sac import ActorUpdate, CriticUpdate, KernelPrioritizedReplayBuffer, TdTarget, sac_update
    S, A, H, L, B, CAP = 2, 1, 256, 2, 64, 300
    case = an.real_case(S, A, H, L)

    def learner():
        actor, critic = copy.deepcopy(case["actor"]).cuda(), copy.deepcopy(case["critic"]).cuda()
        target = td.real_critic(S, A, H, L, seed=1).cuda()
        la = torch.full((1,), -1.0, device="cuda", requires_grad=True)
        buf = KernelPrioritizedReplayBuffer(CAP, S, A, "cuda", seed=5)
        rows = torch.from_numpy(case["rows"]).cuda().clone()
        rows[:, -1] = (torch.arange(rows.shape[0], device="cuda") % 5 == 3).float()
        buf.add_batch(rows)
        copt, aopt, lopt = (torch.optim.Adam(critic.parameters(), lr=LR), torch.optim.Adam(actor.parameters(), lr=LR),
                            torch.optim.Adam([la], lr=LR_ALPHA))
        tdt = TdTarget(actor, target, la, 0.99, seed=11)
        cu = CriticUpdate(critic, target, copt, tau=0.005, max_grad_norm=1.0)
        au = ActorUpdate(actor, critic, la, aopt, lopt, max_grad_norm=1.0, seed=13)
        assert tdt.kernel and cu.kernel and au.kernel
        return dict(actor=actor, critic=critic, target=target, la=la, buf=buf, tdt=tdt, cu=cu, au=au)

    one, two = learner(), learner()
    start = {k: [p.detach().clone() for p in one[k].parameters()] for k in ("actor", "critic", "target")}
    for _ in range(3):
        assert sac_update(one["buf"], one["tdt"], one["cu"], one["au"], B) is None
        # the five pieces by hand, the same draws (every object's draw counter advances by one per call)
        b = two["buf"]
        s, a, r, ns, d, w, idx = b.sample(B)
        tq = two["tdt"](b.last_rows)
        td_abs = two["cu"](b.last_rows, tq, w)
        two["au"](b.last_rows, w)
        b.update_priorities(idx, td_abs)
    torch.cuda.synchronize()
    for k in ("actor", "critic", "target"):
        for p, q, p0 in zip(one[k].parameters(), two[k].parameters(), start[k]):
            assert same_bits(p, q), k
            assert not torch.equal(p, p0), f"{k} did not change"
    assert same_bits(one["la"], two["la"]) and float(one["la"].detach()) != -1.0
    assert same_bits(one["buf"].priorities, two["buf"].priorities) and same_bits(one["buf"].max_prio_dev, two["buf"].max_prio_dev)
    assert not bool((one["buf"].priorities[:case["n"]] == 1.0).all())
    assert one["au"].draws == 3 and one["tdt"].draws == 3 and one["buf"].draws == 3


if __name__ == "__main__":     # python tests/test_gpu_sac_actor_update.py OUT.json: the measurements alone
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "psso-sac-for-powered-descent_amd"))
    shapes = []
    for shape in an.SHAPES:
        res = measure_real(*shape)
        case = an.real_case(*shape)
        row = dict(shape=list(shape), n=sn.N_REAL, loss="PER weights, log_alpha -1, clamp (-5, -1)", dropped=case["dropped"],
                   clamped=case["clamped"], unclamped=case["unclamped"],
                   tensors=[dict(err_kernel=k, err_torch=t, floor=f, max_abs_ref=top, ratio=(k / t if t > 0 else None))
                            for k, t, f, top in res])
        row["worst_ratio"] = max(x["ratio"] for x in row["tensors"] if x["ratio"] is not None)
        shapes.append(row)
        print(shape, "worst ratio", row["worst_ratio"])
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(what="pd_sac_actor_grad and torch float32 autograd (the larger of its GPU and CPU errors) against "
                            "float64 autograd of the same float32 parameters, rows, eps and PER weights: max |grad - ref64| "
                            "per actor tensor (pd_sac_actor's parameter order)",
                       bound_c=REAL_C, shapes=shapes), fh, indent=1)
        fh.write("\n")
