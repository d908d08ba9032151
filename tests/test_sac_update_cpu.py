"""CPU anchors of the SAC critic-update tests: the three exports of csrc/pdsacupd.hip load and refuse
bad arguments before any launch; the scratch size follows its closed form; CriticUpdate.supported
names what it does not take; the integer gradient fixture (tests/sac_grad_nets.py) meets its
conditions for every shape and batch size the GPU tests use; and the binary64 NumPy models the GPU
tests compare the kernels with agree with torch's own float64 autograd and float64 Adam."""
import copy
import ctypes as C

import numpy as np
import pytest

import sac_grad_nets as gn
import sac_nets as sn
import sac_td_nets as td

NEW = ["pd_sac_critic_grad_scratch_bytes", "pd_sac_critic_grad", "pd_adam_step"]


def test_exports_load_and_the_abi_is_still_11():
    import pdenv
    from pdenv import _lib
    from test_abi import header_symbols
    L = pdenv.load()
    syms = header_symbols()
    for name in NEW:
        assert name in syms, f"{name}: not found by the header scan"
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.pd_abi_version() == _lib.ABI_VERSION == 11


@pytest.mark.parametrize("B,H,L", [(256, 256, 2), (37, 512, 8), (1, 128, 1)])
def test_scratch_bytes_closed_form(B, H, L):
    import pdenv
    lib = pdenv.load()
    bp = 16 * ((B + 15) // 16)
    assert lib.pd_sac_critic_grad_scratch_bytes(B, H, L) == 4 * (4 * L * H * bp + 4 * bp + bp // 8)
    assert lib.pd_sac_critic_grad_scratch_bytes(0, H, L) == 0 and lib.pd_sac_critic_grad_scratch_bytes(-3, H, L) == 0


def test_refusals_before_any_launch():
    """Every refusal of pd_sac_critic_grad and pd_adam_step, callable without a GPU: the pointers below
    are never dereferenced."""
    import pdenv
    from pdenv import _lib
    lib = pdenv.load()
    vp = C.c_void_p
    INV, UNS, OK = _lib.PD_ERR_INVALID, _lib.PD_ERR_UNSUPPORTED, _lib.PD_OK
    ok = vp(0x10000)
    good = (vp * 18)(*([0x10000] * 18))
    odd = (vp * 18)(*([0x10000] * 18))
    odd[3] = 0x10004
    null = (vp * 18)(*([0x10000] * 18))
    null[2] = 0
    B, H, Ln = 32, 256, 2
    need = lib.pd_sac_critic_grad_scratch_bytes(B, H, Ln)
    n_part = 2 * (H // 64 + (Ln - 1) * (H // 16) * (H // 128) + H // 128)

    def grad(batch=B, S=2, A=1, H=H, nl=Ln, sa=ok, pitch=7, target=ok, weights=None, kind=0, dq_in=None, p1=good,
             p2=good, g1=good, g2=good, q=ok, td_abs=ok, dq_out=None, loss=ok, partials=ok, count=n_part,
             scratch=ok, nbytes=need):
        cnt = C.c_int32(count or 0)
        return lib.pd_sac_critic_grad(batch, S, A, H, nl, sa, pitch, target, weights, kind, dq_in, p1, p2, g1, g2, q,
                                      td_abs, dq_out, loss, partials, C.byref(cnt) if count is not None else None,
                                      scratch, nbytes, None)

    for kw in (dict(batch=-1), dict(S=0), dict(A=0), dict(S=12, A=5), dict(nl=0), dict(nl=9), dict(pitch=2),
               dict(kind=2), dict(kind=-1), dict(sa=None), dict(target=None), dict(p1=None), dict(g2=None),
               dict(p2=null), dict(g1=null), dict(scratch=None), dict(nbytes=need - 4), dict(scratch=vp(0x10004)),
               dict(count=n_part - 1), dict(count=None),
               dict(target=None, dq_in=ok, dq_out=ok)):          # (td_abs and loss asked for without a target)
        assert grad(**kw) == INV, kw
    assert b"loss kind" in (grad(kind=7), lib.pd_last_error())[1]
    assert b"scratch" in (grad(nbytes=8), lib.pd_last_error())[1]
    for kw in (dict(H=64), dict(H=384), dict(p1=odd), dict(g2=odd)):
        assert grad(**kw) == UNS, kw
    assert b"aligned" in lib.pd_last_error()
    assert b"hidden" in (grad(H=64), lib.pd_last_error())[1]
    # an empty batch: PD_OK without a launch, whatever the data pointers are
    assert grad(batch=0, sa=None, target=None, q=None, td_abs=None, loss=None, scratch=None, nbytes=0) == OK
    assert grad(batch=0, H=64) == UNS and grad(batch=0, kind=3) == INV

    numel = (C.c_int64 * 4)(5, 0, 7, 1)
    four = (vp * 4)(*([0x10000] * 4))
    hole = (vp * 4)(0x10000, 0, 0, 0x10000)                    # (tensor 1 has no elements: its null is skipped)

    def adam(n=4, p=four, g=four, m=four, v=four, numel=numel, targets=None, max_norm=0.0, partials=None, n_partials=0):
        return lib.pd_adam_step(n, p, g, m, v, numel, targets, 1e-3, 1.0, 0.9, 0.999, 1e-8, max_norm, partials,
                                n_partials, None, 0.005, None)

    neg = (C.c_int64 * 4)(5, -1, 7, 1)
    for kw in (dict(n=-1), dict(n=65), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(numel=None),
               dict(p=hole), dict(targets=hole), dict(numel=neg), dict(max_norm=1.0),
               dict(max_norm=1.0, partials=ok, n_partials=0)):
        assert adam(**kw) == INV, kw
    assert b"pd_adam_step" in lib.pd_last_error()
    assert adam(n=0, p=None, g=None, m=None, v=None, numel=None) == OK
    empty = (C.c_int64 * 4)(0, 0, 0, 0)
    assert adam(numel=empty, p=hole) == OK                      # nothing to do: nothing launched


def test_supported_names_what_it_does_not_take():
    """CriticUpdate.reasons on CPU modules (so "tensors" -- not on the device -- is always among them, and
    is the only one for a plain Adam over a critic of a supported shape)."""
    import torch
    from pdenv.sac import Critic, CriticUpdate
    critic, target = Critic(2, 1, 256, 2), Critic(2, 1, 256, 2)
    Adam = torch.optim.Adam
    assert CriticUpdate.reasons(critic, Adam(critic.parameters()), target) == ["tensors"]
    assert not CriticUpdate.supported(critic, Adam(critic.parameters()), target)
    for kw, word in ((dict(weight_decay=1e-2), "weight_decay"), (dict(amsgrad=True), "amsgrad"),
                     (dict(maximize=True), "maximize"), (dict(capturable=True), "capturable"),
                     (dict(lr=torch.tensor(1e-3)), "lr")):
        why = CriticUpdate.reasons(critic, Adam(critic.parameters(), **kw), target)
        assert word in why and not CriticUpdate.supported(critic, Adam(critic.parameters(), **kw), target), (kw, why)
    assert "adam" in CriticUpdate.reasons(critic, torch.optim.AdamW(critic.parameters(), weight_decay=0.0), target)
    assert "adam" in CriticUpdate.reasons(critic, torch.optim.SGD(critic.parameters(), lr=0.1), target)
    two = Adam([dict(params=list(critic.q1.parameters())), dict(params=list(critic.q2.parameters()))])
    assert "param_groups" in CriticUpdate.reasons(critic, two, target)
    assert "params" in CriticUpdate.reasons(critic, Adam(critic.q1.parameters()), target)
    assert "params" in CriticUpdate.reasons(critic, Adam(list(critic.parameters())[::-1]), target)
    for shape in ((2, 1, 64, 2), (2, 1, 384, 2), (12, 5, 256, 2), (2, 1, 128, 9)):
        c = Critic(*shape)
        assert "shape" in CriticUpdate.reasons(c, Adam(c.parameters()), Critic(*shape)), shape
    assert "target" in CriticUpdate.reasons(critic, Adam(critic.parameters()), Critic(2, 1, 128, 2))
    assert "target" in CriticUpdate.reasons(critic, Adam(critic.parameters()), Critic(2, 1, 256, 3))
    half = Critic(2, 1, 256, 2).double()
    assert "tensors" in CriticUpdate.reasons(half, Adam(half.parameters()))
    # the fallback object on the CPU: the torch block, the same fields
    upd = CriticUpdate(critic, target, Adam(critic.parameters()), max_grad_norm=1.0)
    assert not upd.kernel
    rows, tq = torch.rand(8, 7), torch.rand(8, 1)
    td_abs = upd(rows, tq)
    assert td_abs.shape == (8,) and upd.q.shape == (8, 2) and upd.critic_loss.shape == (1,) and upd.grad_norm.shape == (1,)


@pytest.mark.parametrize("n", gn.BATCHES)
@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_N)
def test_integer_gradient_fixture_is_valid(S, A, H, L, n):
    """For every shape and batch size of the GPU tests: on the int64 model, the sum of the absolute
    values of the terms of every partial sum -- forward, every delta, every gradient entry -- is below
    2**24 (asserted inside int_grad_case, repeated here on the model's figures)."""
    c = gn.int_grad_case(S, A, H, L, n=n)
    for w in range(2):
        m = gn.backward(c["params"][w], c["sa"], c["dq"][:, w])
        assert 0 < m["abs_sum"] < 2 ** 24
        assert max(m["terms"]) <= m["abs_sum"]
        for g, want in zip(m["grads"], c["grads"][w]):
            assert np.array_equal(g.reshape(want.shape), want.astype(np.int64))
    assert c["sa"].shape == (n, S + A) and c["dq"].shape == (n, 2) and c["q"].shape == (n, 2)
    assert (c["dq"] == 0).any() or n == 1
    if n == sn.N_EXACT:
        assert c["zero_pre"] > 0


@pytest.mark.parametrize("S,A,H,L", gn.SHAPES_DEEP)
def test_integer_gradient_fixture_is_valid_deep(S, A, H, L):
    c = gn.int_grad_case(S, A, H, L)
    for w in range(2):
        assert gn.backward(c["params"][w], c["sa"], c["dq"][:, w])["abs_sum"] < 2 ** 24
    assert c["zero_pre"] > 0


def test_integer_backward_is_autograd():
    """The int64 backward pass against torch's float64 autograd on the same integers (exact there too)."""
    import torch
    from pdenv.sac import Critic
    S, A, H, L = 5, 4, 256, 3
    c = gn.int_grad_case(S, A, H, L)
    critic = td.load_critic(Critic(S, A, hidden_dim=H, n_hidden_layers=L), *c["params"]).double()
    sa = torch.from_numpy(c["sa"]).double()
    q1, q2 = critic(sa[:, :S], sa[:, S:])
    dq = torch.from_numpy(c["dq"]).double()
    torch.autograd.backward([q1, q2], [dq[:, :1], dq[:, 1:]])
    want = [g for w in range(2) for g in c["grads"][w]]
    for p, g in zip(critic.parameters(), want):
        assert np.array_equal(p.grad.numpy(), g.astype(np.float64))


@pytest.mark.parametrize("kind", [gn.L2, gn.L1])
@pytest.mark.parametrize("per", [False, True])
def test_models_agree_with_torch_float64(kind, per):
    """loss_model and full_backward against the reference's loss expressions and autograd in float64."""
    import torch
    import torch.nn.functional as F
    S, A, H, L = 2, 1, 128, 2
    case = gn.grad_case(S, A, H, L, n=37)
    c64 = copy.deepcopy(case["critic"]).double()
    rows, t = torch.from_numpy(case["rows"]).double(), torch.from_numpy(case["target"]).double().reshape(-1, 1)
    w = torch.from_numpy(case["weights"]).double().reshape(-1, 1)
    q1, q2 = c64(rows[:, :S], rows[:, S:S + A])
    f = F.l1_loss if kind == gn.L1 else F.mse_loss
    if per:
        loss = (w * f(q1, t, reduction="none") + w * f(q2, t, reduction="none")).mean()
    else:
        loss = f(q1, t) + f(q2, t)
    loss.backward()
    grads, terms, qs = gn.full_backward(td.critic_params(case["critic"]), case["rows"][:, :S + A], case["target"],
                                        case["weights"] if per else None, kind)
    m = gn.loss_model(qs, case["target"], case["weights"] if per else None, kind)
    assert abs(m["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    td_abs = torch.max((t - q1).abs(), (t - q2).abs()).detach().numpy()[:, 0]
    np.testing.assert_allclose(m["td_abs"], td_abs, rtol=0, atol=1e-12)
    for p, g, tm in zip(c64.parameters(), grads, terms):
        np.testing.assert_allclose(g, p.grad.numpy(), rtol=0, atol=1e-12 * max(1.0, tm))
        assert tm >= np.abs(g).max() * (1 - 1e-12)
    assert (m["E_dq"] >= 0).all() and m["E_loss"] > 0 and (m["E_td"] >= 0).all()


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_model_is_torch_adam(step):
    """adam_model and polyak_f32 against clip_grad_norm_ + torch.optim.Adam in float64 (whose constants
    are binary64 where the model's are the float32 numbers the kernel receives: 2**-23 relative)."""
    import torch
    rng = np.random.default_rng(step)
    shapes = [1, 5, 513]
    p = [rng.uniform(-1, 1, k).astype(np.float32) for k in shapes]
    g = [rng.standard_normal(k).astype(np.float32) for k in shapes]
    m = [np.zeros(k, dtype=np.float32) if step == 1 else (0.5 * x).astype(np.float32) for k, x in zip(shapes, g)]
    v = [np.zeros(k, dtype=np.float32) if step == 1 else (x * x).astype(np.float32) for k, x in zip(shapes, g)]
    tp = [torch.nn.Parameter(torch.from_numpy(x).double()) for x in p]
    opt = torch.optim.Adam(tp, lr=3e-4)
    for q, gg, mm, vv in zip(tp, g, m, v):
        q.grad = torch.from_numpy(gg).double()
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(mm).double(),
                            exp_avg_sq=torch.from_numpy(vv).double())
    parts = [float((x.astype(np.float64) ** 2).sum()) for x in g]
    norm = float(np.sqrt(sum(parts)))
    total = torch.nn.utils.clip_grad_norm_(tp, max_norm=0.5 * norm)
    opt.step()
    model = gn.adam_model(p, g, m, v, step, 3e-4, 0.9, 0.999, 1e-8, 0.5 * norm, parts)
    assert abs(model["norm"] - float(total)) <= 1e-12 * norm and abs(model["coef"] - 0.5) < 1e-5
    for k, q in enumerate(tp):
        s = opt.state[q]
        np.testing.assert_allclose(model["m"][k], s["exp_avg"].numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(model["v"][k], s["exp_avg_sq"].numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(model["p"][k], q.detach().numpy(), rtol=0, atol=3e-4 * 1e-5)
        assert (model["E_p"][k] > 0).all() and (model["E_p"][k] < 1e-6).all()
    t = rng.uniform(-1, 1, 513).astype(np.float32)
    want = ((1 - 0.005) * torch.from_numpy(t) + 0.005 * torch.from_numpy(p[2])).numpy()
    assert np.array_equal(gn.polyak_f32(t, p[2], 0.005).view(np.int32), want.view(np.int32))
