"""CPU checks of the SAC actor update (csrc/pdsacact.hip, pdenv.sac.ActorUpdate): the exports and
their refusals (made before any launch, so callable without a GPU), the scratch closed form,
ActorUpdate.reasons on CPU modules, and the fixtures and NumPy models of
tests/test_gpu_sac_actor_update.py -- the integer fixtures are valid for every shape and batch, the
binary64 models are torch's float64 autograd of the reference lines, and the real-valued fixture keeps
its conditions."""
import copy
import ctypes as C

import numpy as np
import pytest

import sac_actor_grad_nets as an
import sac_nets as sn
import sac_td_nets as td

vp = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from pdenv import _lib
    return _lib.load(), _lib


def test_exports_load_and_abi_is_11(lib):
    L, _lib = lib
    assert L.pd_abi_version() == _lib.ABI_VERSION == 11
    for name in ("pd_sac_critic_dinput", "pd_sac_actor_grad_scratch_bytes", "pd_sac_actor_grad"):
        assert hasattr(L, name) and name in _lib.EXPORTS


def test_scratch_closed_form(lib):
    L, _ = lib
    for n in (1, 15, 16, 17, 37, 256, 261, 512):
        for A, H, nl in ((1, 256, 2), (2, 128, 1), (4, 512, 2), (4, 256, 3), (8, 128, 8)):
            assert L.pd_sac_actor_grad_scratch_bytes(n, A, H, nl) == an.scratch_bytes(n, A, H, nl)
    for bad in ((0, 1, 256, 2), (-1, 1, 256, 2), (16, 0, 256, 2), (16, 1, 0, 2), (16, 1, 256, 0)):
        assert L.pd_sac_actor_grad_scratch_bytes(*bad) == 0


def actor_call(L, batch=37, S=2, A=1, rows=0x10000, pitch=7, weights=None, H=256, nl=2, params="ok", grads="ok",
               HC=256, nc=2, p1="ok", p2="ok", log_alpha=0x10000, dheads=None, partials=None, n_partials=None,
               scratch=0x10000, scratch_bytes=None):
    """pd_sac_actor_grad on made-up pointers (never dereferenced: every case is refused before a launch)."""
    def plist(v, n):
        if v == "ok":
            return (vp * n)(*([0x10000] * n))
        return v
    P = lambda v: None if v is None else vp(v)
    if scratch_bytes is None:
        scratch_bytes = an.scratch_bytes(batch, A, H, nl)
    return L.pd_sac_actor_grad(batch, S, A, P(rows), pitch, P(weights), H, nl, plist(params, 2 * (nl + 2)),
                               plist(grads, 2 * (nl + 2)), -5.0, -1.0, 1.0, HC, nc, plist(p1, 2 * (nc + 1)),
                               plist(p2, 2 * (nc + 1)), P(log_alpha), -1.0, 0, 0, None, P(dheads), None, None, None, None,
                               None, None, None, None, None, None, P(partials), n_partials, P(scratch), scratch_bytes, None)


def test_actor_grad_refusals_before_any_launch(lib):
    L, _lib = lib
    INV, UNS, OK = _lib.PD_ERR_INVALID, _lib.PD_ERR_UNSUPPORTED, _lib.PD_OK
    assert actor_call(L, batch=0) == OK                              # nothing launched
    cnt = C.c_int32(99)
    assert actor_call(L, batch=0, partials=0x10000, n_partials=C.byref(cnt)) == OK and cnt.value == 0
    assert actor_call(L, batch=-1) == INV
    assert actor_call(L, S=0) == INV and actor_call(L, A=0) == INV
    assert actor_call(L, rows=None) == INV
    assert actor_call(L, pitch=1) == INV and b"pitch" in L.pd_last_error()
    assert actor_call(L, params=None) == INV and actor_call(L, grads=None) == INV
    assert actor_call(L, log_alpha=None) == INV
    assert actor_call(L, p1=None) == INV and actor_call(L, p2=None) == INV
    assert actor_call(L, partials=0x10000, n_partials=None) == INV
    short = C.c_int32(an.n_partials(256, 2) - 1)
    assert actor_call(L, partials=0x10000, n_partials=C.byref(short)) == INV and b"sumsq_partials" in L.pd_last_error()
    null_param = (vp * 8)(*([0x10000] * 7 + [0]))
    assert actor_call(L, params=null_param) == INV and actor_call(L, grads=null_param) == INV
    assert actor_call(L, p1=(vp * 6)(*([0x10000] * 5 + [0]))) == INV
    for scratch, nb in ((None, None), (0x10000, an.scratch_bytes(37, 1, 256, 2) - 4), (0x10004, None)):
        assert actor_call(L, scratch=scratch, scratch_bytes=nb) == INV and b"scratch" in L.pd_last_error()
    assert actor_call(L, H=64) == UNS and actor_call(L, HC=64) == UNS
    assert actor_call(L, S=17, pitch=40) == UNS and actor_call(L, A=9, pitch=40) == UNS
    assert actor_call(L, S=12, A=5, pitch=40) == UNS               # the critic's input above 16
    assert actor_call(L, nl=9, params=(vp * 22)(*([0x10000] * 22)), grads=(vp * 22)(*([0x10000] * 22))) == UNS
    assert actor_call(L, nc=9, p1=(vp * 20)(*([0x10000] * 20)), p2=(vp * 20)(*([0x10000] * 20))) == UNS
    odd = (vp * 8)(*([0x10000] * 7 + [0x10004]))
    assert actor_call(L, params=odd) == UNS and b"aligned" in L.pd_last_error()
    assert actor_call(L, grads=odd) == UNS
    assert actor_call(L, p2=(vp * 6)(*([0x10000] * 5 + [0x10008]))) == UNS
    # with dheads_in the critic may be missing, and its shape is not looked at
    assert actor_call(L, batch=0, dheads=0x10000, p1=None, p2=None, HC=0, nc=0) == OK
    assert actor_call(L, dheads=0x10000, p1=None, p2=None, HC=0, nc=0, scratch=None) == INV and b"scratch" in L.pd_last_error()
    # ... and the domain is the actor's alone: S + A above 16 passes every check up to the scratch
    for S, A in ((12, 5), (16, 8)):
        assert actor_call(L, S=S, A=A, pitch=40, dheads=0x10000, p1=None, p2=None, HC=0, nc=0, scratch=None) == INV
        assert b"scratch" in L.pd_last_error()
        assert actor_call(L, batch=0, S=S, A=A, pitch=40, dheads=0x10000, p1=None, p2=None, HC=0, nc=0) == OK
    assert actor_call(L, S=17, A=1, pitch=40, dheads=0x10000, p1=None, p2=None) == UNS
    assert actor_call(L, S=4, A=9, pitch=40, dheads=0x10000, p1=None, p2=None) == UNS


def test_critic_dinput_refusals_before_any_launch(lib):
    L, _lib = lib
    INV, UNS, OK = _lib.PD_ERR_INVALID, _lib.PD_ERR_UNSUPPORTED, _lib.PD_OK
    ok = (vp * 6)(*([0x10000] * 6))

    def call(batch=37, S=2, A=1, H=256, nl=2, sa=0x10000, pitch=3, p1=ok, p2=ok):
        return L.pd_sac_critic_dinput(batch, S, A, H, nl, None if sa is None else vp(sa), pitch, p1, p2, vp(0x10000),
                                      vp(0x10000), None)
    assert call(batch=0) == OK
    assert call(batch=-1) == INV and call(S=0) == INV and call(A=0) == INV and call(S=12, A=5, pitch=17) == INV
    assert call(sa=None) == INV and call(p1=None) == INV and call(nl=0) == INV and call(nl=9) == INV
    assert call(pitch=2) == INV and b"pitch" in L.pd_last_error()
    assert call(p2=(vp * 6)(*([0x10000] * 5 + [0]))) == INV
    assert call(H=64) == UNS
    assert call(p1=(vp * 6)(*([0x10000] * 5 + [0x10004]))) == UNS and b"aligned" in L.pd_last_error()


def test_actor_update_reasons_on_cpu_modules():
    import torch
    from pdenv.sac import Actor, ActorUpdate, Critic
    actor, critic = Actor(2, 1), Critic(2, 1)
    la = torch.zeros(1, requires_grad=True)
    opt, aopt = torch.optim.Adam(actor.parameters(), lr=3e-4), torch.optim.Adam([la], lr=3e-4)
    why = ActorUpdate.reasons(actor, critic, la, opt, aopt)
    assert why == ["tensors", "log_alpha"], why                    # CPU tensors: the only defects
    assert not ActorUpdate.supported(actor, critic, la, opt, aopt)
    la64 = torch.tensor(np.log(0.2), requires_grad=True)             # the reference's construction: float64
    assert la64.dtype == torch.float64
    assert "log_alpha" in ActorUpdate.reasons(actor, critic, la64, opt, torch.optim.Adam([la64]))
    assert "actor" in ActorUpdate.reasons(Actor(2, 1, hidden_dim=64), critic, la, opt)
    assert "critic" in ActorUpdate.reasons(actor, Critic(2, 1, hidden_dim=64), la, opt)
    assert "critic" in ActorUpdate.reasons(actor, Critic(3, 1), la, opt)         # its input is not S + A
    assert "adam" in ActorUpdate.reasons(actor, critic, la, torch.optim.SGD(actor.parameters(), lr=0.1))
    assert "weight_decay" in ActorUpdate.reasons(actor, critic, la, torch.optim.Adam(actor.parameters(), weight_decay=0.1))
    assert "params" in ActorUpdate.reasons(actor, critic, la, torch.optim.Adam(list(actor.parameters())[:-1]))
    assert "alpha_adam" in ActorUpdate.reasons(actor, critic, la, opt, torch.optim.SGD([la], lr=0.1))
    assert "alpha_amsgrad" in ActorUpdate.reasons(actor, critic, la, opt, torch.optim.Adam([la], amsgrad=True))
    assert "alpha_params" in ActorUpdate.reasons(actor, critic, la, opt, torch.optim.Adam([torch.zeros(1, requires_grad=True)]))
    # CriticUpdate's words are what they were
    from pdenv.sac import CriticUpdate
    copt = torch.optim.Adam(critic.parameters(), amsgrad=True)
    assert CriticUpdate.reasons(critic, copt) == ["tensors", "amsgrad"]
    assert CriticUpdate.reasons(critic, torch.optim.SGD(critic.parameters(), lr=0.1)) == ["tensors", "adam"]


def test_actor_update_fallback_on_cpu_matches_the_reference_lines():
    """Outside the domain (CPU modules here) ActorUpdate runs the same steps in torch: one update equals
    the reference lines followed by clip and the two optimizers' steps, and the critic's p.grad is
    left alone."""
    import torch
    from pdenv.sac import ActorUpdate
    S, A, H, L = 2, 1, 256, 2
    case = an.real_case(S, A, H, L)
    n = 64
    rows, eps, w = (torch.from_numpy(case[k][:n]) for k in ("rows", "eps", "weights"))
    actor, critic = copy.deepcopy(case["actor"]), copy.deepcopy(case["critic"])
    la = torch.full((1,), -1.0, requires_grad=True)
    opt, aopt = torch.optim.Adam(actor.parameters(), lr=1e-3), torch.optim.Adam([la], lr=1e-2)
    upd = ActorUpdate(actor, critic, la, opt, aopt, max_grad_norm=1.0)
    assert not upd.kernel and upd.target_entropy == -float(A)
    ref_actor, ref_la = copy.deepcopy(actor), la.detach().clone()
    want = an.torch_block(ref_actor, critic, rows[:, :S], eps, w, ref_la, -float(A))
    sentinel = [torch.full_like(p, 3.0) for p in critic.parameters()]
    for p, g in zip(critic.parameters(), sentinel):
        p.grad = g.clone()
    lp = upd(rows, w, eps=eps)
    assert lp.shape == (n, 1) and np.allclose(lp[:, 0].numpy(), want["log_prob"], rtol=1e-6, atol=1e-6)
    assert np.allclose(upd.new_actions.numpy(), want["new_actions"], atol=1e-7) and upd.q.shape == (n, 2)
    assert abs(float(upd.actor_loss) - want["actor_loss"]) < 1e-6 and abs(float(upd.alpha_loss) - want["alpha_loss"]) < 1e-6
    for p, g in zip(critic.parameters(), sentinel):
        assert torch.equal(p.grad, g)
    ropt, raopt = torch.optim.Adam(ref_actor.parameters(), lr=1e-3), torch.optim.Adam([ref_la.requires_grad_(True)], lr=1e-2)
    ref_la.grad = torch.full((1,), want["log_alpha_grad"])
    norm = torch.nn.utils.clip_grad_norm_(ref_actor.parameters(), max_norm=1.0)
    ropt.step(); raopt.step()
    assert abs(float(upd.grad_norm) - float(norm)) < 1e-6 * float(norm)
    for p, r in zip(actor.parameters(), ref_actor.parameters()):
        assert torch.allclose(p, r, atol=1e-7)
    assert abs(la.item() - ref_la.item()) < 1e-7 and la.item() != -1.0
    # no alpha optimizer: alpha_loss 0 and log_alpha untouched
    la2 = torch.full((1,), -1.0, requires_grad=True)
    upd2 = ActorUpdate(actor, critic, la2, opt)
    upd2(rows, eps=eps)
    assert float(upd2.alpha_loss) == 0.0 and la2.item() == -1.0 and la2.grad is None and upd2.grad_norm is None


@pytest.mark.parametrize("S,A,H,L", an.SHAPES_WIDE)
def test_integer_actor_fixtures_above_16_inputs_are_valid(S, A, H, L):
    for n in (17, sn.N_EXACT):
        c = an.int_actor_case(S, A, H, L, n=n)
        assert c["obs"].shape == (n, S) and S + A > 16 and len(c["grads"]) == 2 * (L + 2)


def test_actor_update_takes_an_actor_of_another_build():
    """An actor _actor_shape rejects -- a first module that is no Linear, or no shared_net at all -- is
    a reason ("actor"), not an AttributeError: the constructor works and the torch path runs it."""
    import torch
    import torch.nn as nn
    from pdenv.sac import Actor, ActorUpdate, Critic
    S, A, B = 3, 2, 8

    odd = Actor(S, A, hidden_dim=32)
    odd.shared_net = nn.Sequential(nn.Identity(), *odd.shared_net)

    class Plain(nn.Module):                       # the reference's interface only: forward() -> mean, log_std
        max_action = 1.0

        def __init__(self):
            super().__init__()
            self.body, self.mean, self.ls = nn.Linear(S, 16), nn.Linear(16, A), nn.Linear(16, A)

        def forward(self, x):
            f = torch.relu(self.body(x))
            return self.mean(f), torch.clamp(self.ls(f), -5.0, 2.0)

    class Headless(nn.Module):
        def forward(self, x):
            return x, x

    critic = Critic(S, A, hidden_dim=32)
    rows, eps = torch.randn(B, 2 * S + A + 2), torch.randn(B, A)
    for actor in (odd, Plain()):
        la = torch.zeros(1, requires_grad=True)
        opt, aopt = torch.optim.Adam(actor.parameters(), lr=1e-3), torch.optim.Adam([la], lr=1e-3)
        assert "actor" in ActorUpdate.reasons(actor, critic, la, opt, aopt)
        upd = ActorUpdate(actor, critic, la, opt, aopt, max_grad_norm=1.0)
        assert not upd.kernel and (upd.S, upd.A) == (S, A) and upd.target_entropy == -float(A)
        before = [p.detach().clone() for p in actor.parameters()]
        lp = upd(rows, eps=eps)
        assert lp.shape == (B, 1) and upd.new_actions.shape == (B, A) and upd.q.shape == (B, 2)
        assert bool(torch.isfinite(upd.actor_loss).all()) and la.item() != 0.0
        assert any(not torch.equal(p, b) for p, b in zip(actor.parameters(), before))
    with pytest.raises(ValueError):
        ActorUpdate(Headless(), critic, torch.zeros(1), torch.optim.Adam([torch.zeros(1, requires_grad=True)]))


def test_sac_update_is_the_five_pieces_in_order():
    """sac_update holds the order and nothing else: on recording stand-ins it calls sample, TdTarget,
    CriticUpdate, ActorUpdate and update_priorities once each, in that order, with the sample's rows,
    weights and indices and the critic step's td_abs, and returns nothing."""
    from pdenv.sac import sac_update
    log = []

    class Buf:
        last_rows = None

        def sample(self, b):
            log.append(("sample", b))
            self.last_rows = "rows"
            return ("s", "a", "r", "s2", "d", "w", "idx")

        def update_priorities(self, idx, td):
            log.append(("update_priorities", idx, td))

    tdt = lambda rows: log.append(("td_target", rows)) or "tq"
    cu = lambda rows, tq, w: log.append(("critic", rows, tq, w)) or "td_abs"
    au = lambda rows, w: log.append(("actor", rows, w)) or "lp"
    assert sac_update(Buf(), tdt, cu, au, 64) is None
    assert log == [("sample", 64), ("td_target", "rows"), ("critic", "rows", "tq", "w"), ("actor", "rows", "w"),
                   ("update_priorities", "idx", "td_abs")]


@pytest.mark.parametrize("S,A,H,L", an.SHAPES)
def test_integer_fixtures_are_valid(S, A, H, L):
    """Every partial sum below 2**24 for every batch the GPU tests use (asserted inside the cases), the
    two heads' gradients and every input column's gradient not all zero."""
    for n in an.BATCHES:
        c = an.int_actor_case(S, A, H, L, n=n)
        assert c["obs"].shape == (n, S) and c["dheads"].shape == (n, 2 * A) and len(c["grads"]) == 2 * (L + 2)
        d = an.int_dinput_case(S, A, H, L, n=n)
        assert d["dsa"].shape == (n, 2, S + A) and d["q"].shape == (n, 2)
    assert set(np.unique(an.int_actor_case(S, A, H, L)["dheads"])) == {-1.0, 0.0, 1.0}
    # the int64 Q-net input gradient is the binary64 one (the same code in another dtype)
    d = an.int_dinput_case(S, A, H, L)
    for w in range(2):
        q, dsa, _ = an.q_dinput(d["params"][w], d["sa"], dtype=np.float64)
        assert np.array_equal(dsa, d["dsa"][:, w]) and np.array_equal(q, d["q"][:, w])


def special_rows(n, A, lo, hi, rng):
    """heads, eps, q, dq/da [n] for the elementwise chain with the corner rows the kernel has a branch
    or a saturation for: row 0 a tie q1 == q2, rows 1-6 a raw log_std just below, at and just above each
    clamp bound, rows 7 and 8 a saturated a = +1 and -1 (|eps| = 200 at the upper bound's std)."""
    heads = rng.uniform(-1.5, 1.5, (n, 2 * A)).astype(np.float32)
    heads[:, A:] = rng.uniform(lo - 1.0, hi + 1.0, (n, A))
    eps = rng.standard_normal((n, A)).astype(np.float32)
    q = rng.uniform(-2, 2, (n, 2)).astype(np.float32)
    dqda = rng.uniform(-2, 2, (n, 2, A)).astype(np.float32)
    q[0, 1] = q[0, 0]
    f = np.float32
    for r, v in enumerate((np.nextafter(f(lo), f(-np.inf)), f(lo), np.nextafter(f(lo), f(np.inf)),
                           np.nextafter(f(hi), f(-np.inf)), f(hi), np.nextafter(f(hi), f(np.inf)))):
        heads[1 + r, A:] = v
    heads[7:9, A:] = hi
    eps[7], eps[8] = 200.0, -200.0
    return heads, eps, q, dqda


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("A", [1, 3])
def test_elementwise_model_is_float64_autograd(A, per):
    """elem's dheads and losses against torch float64 autograd of sac_pytorch.py:486-497, 512-520 with
    the heads as leaves and each Q a function of new_action with the given value and gradient -- the
    tie, the clamp's six sides and both saturations among the rows."""
    import torch
    n, lo, hi, ma, la, te = 40, td.LOG_STD_MIN, td.LOG_STD_MAX, 1.5, -0.7, -float(A)
    rng = np.random.default_rng([A, 3])
    heads, eps, q, dqda = special_rows(n, A, lo, hi, rng)
    w = rng.uniform(0.2, 1.0, n).astype(np.float32) if per else None
    m = an.elem(heads, eps, q, dqda, w, lo, hi, ma, la, te)
    T = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    mean, raw = T(heads[:, :A]).requires_grad_(True), T(heads[:, A:]).requires_grad_(True)
    log_std = torch.clamp(raw, lo, hi)
    std = log_std.exp()
    x = mean + std * T(eps)
    action = torch.tanh(x)
    log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - float(np.float32(0.9189385332046727))
                - torch.log(1 - action.pow(2) + float(np.float32(1e-6)))).sum(-1, keepdim=True)
    na = action * ma
    qs = [T(q[:, j:j + 1]) + (T(dqda[:, j]) * (na - na.detach())).sum(-1, keepdim=True) for j in range(2)]
    alpha = float(np.exp(np.float64(np.float32(la))))
    t = alpha * log_prob - torch.min(qs[0], qs[1])
    wt = None if w is None else T(w).reshape(n, 1)
    loss = (t if wt is None else wt * t).mean()
    loss.backward()
    got = np.concatenate([mean.grad.numpy(), raw.grad.numpy()], axis=1)
    scale = np.abs(got).max()
    # (autograd keeps the rounding residue of the quadratic term's two cancelling paths, about eps^2
    # 2**-53 of cl: 1e-11 at the rows with |eps| = 200)
    assert np.abs(m["dheads"] - got).max() <= 1e-10 * scale, np.abs(m["dheads"] - got).max()
    la_t = torch.tensor(float(np.float32(la)), dtype=torch.float64, requires_grad=True)
    tt = (log_prob + te).detach()
    alpha_loss = -(la_t * (tt if wt is None else wt * tt)).mean()
    alpha_loss.backward()
    loss, alpha_loss = loss.item(), alpha_loss.item()
    assert abs(m["actor_loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(m["alpha_loss"] - alpha_loss) <= 1e-12 * max(1.0, abs(alpha_loss))
    assert abs(m["log_alpha_grad"] - la_t.grad.item()) <= 1e-12 * max(1.0, abs(la_t.grad.item()))
    assert np.abs(m["log_prob"] - log_prob.detach().numpy()[:, 0]).max() <= 1e-12 * np.abs(m["log_prob"]).max()
    # the corners are what they are meant to be
    assert m["sel"][0].tolist() == [0.5, 0.5]
    assert m["inside"][1:7, 0].tolist() == [False, True, True, True, True, False]
    assert (got[[1, 6], A:] == 0).all() and (got[[2, 5], A:] != 0).all()       # torch.clamp passes at the bounds
    assert np.abs(m["c"]["a"][7]).min() > 1 - 1e-12 and (m["c"]["a"][7] > 0).all() and (m["c"]["a"][8] < 0).all()
    # the a-priori bound is finite and positive wherever the value is not exactly zero
    E = an.elem_bound(m)
    assert np.isfinite(E["dheads"]).all() and (E["dheads"][m["dheads"] != 0] > 0).all()
    assert all(np.isfinite(E[k]) and E[k] > 0 for k in ("actor_loss", "alpha_loss", "log_alpha_grad"))


@pytest.mark.parametrize("S,A,H,L", [(2, 1, 256, 2), (5, 4, 256, 3)])
def test_whole_block_model_is_float64_autograd(S, A, H, L):
    """full (the fixture's reference) against torch float64 autograd of the reference lines on the nets."""
    import torch
    case = an.real_case(S, A, H, L)
    ref = case["ref"]
    a64, c64 = copy.deepcopy(case["actor"]).double(), copy.deepcopy(case["critic"]).double()
    rows, eps, w = (torch.from_numpy(case[k]).double() for k in ("rows", "eps", "weights"))
    la = torch.full((1,), case["log_alpha"], dtype=torch.float64)
    want = an.torch_block(a64, c64, rows[:, :S], eps, w, la, case["target_entropy"])
    for k, (g, r) in enumerate(zip(ref["grads"], want["grads"])):
        assert np.abs(g - r).max() <= 1e-9 * max(1.0, np.abs(r).max()), k
    # (the model carries the float32 constants of the kernel's expression: 0.9189385332046727 rounded to
    # float32 is off by less than 2**-25 per component, which log_prob and the losses see)
    tol = A * 2.0 ** -24
    for name in ("actor_loss", "alpha_loss", "log_alpha_grad"):
        assert abs(ref[name] - want[name]) <= tol * max(1.0, abs(want[name])), name
    assert np.abs(ref["q"] - want["q"]).max() <= 1e-9 and np.abs(ref["log_prob"] - want["log_prob"]).max() <= tol
    assert max(np.abs(g).max() for g in want["grads"]) > 1e-3


@pytest.mark.parametrize("S,A,H,L", an.SHAPES)
def test_real_fixture_conditions(S, A, H, L):
    """At most 10 % of the candidate rows were dropped for standing within the margin of a kink of the
    loss; clamped and unclamped components both occur and either net is the smaller one somewhere; the
    kept rows keep the margins."""
    case = an.real_case(S, A, H, L)
    ref = case["ref"]
    print(f"{(S, A, H, L)}: dropped {case['dropped']:.3f}, clamped {case['clamped']}, unclamped {case['unclamped']}, "
          f"q1 smaller {case['q1_smaller']}, q2 smaller {case['q2_smaller']}")
    assert case["rows"].shape == (sn.N_REAL, 2 * S + A + 2)
    assert case["dropped"] <= 0.10, case["dropped"]
    assert case["clamped"] > 0 and case["unclamped"] > 0
    assert case["q1_smaller"] > 0 and case["q2_smaller"] > 0
    raw = ref["heads"][:, A:]
    assert (np.abs(ref["q"][:, 0] - ref["q"][:, 1]) >= an.MARGIN * ref["E_q"].max(axis=1)).all()
    assert (np.minimum(np.abs(raw - td.LOG_STD_MIN), np.abs(raw - td.LOG_STD_MAX)) >= an.MARGIN * ref["E_heads"][:, A:]).all()
    heads_top = np.abs(ref["heads"]).max()
    assert 0.1 <= heads_top <= 1e3, heads_top


def test_eps_draws_use_their_own_tag():
    a = an.np_eps(5, 9, 40, 3)
    b = td.np_eps(5, 9, 40, 3)
    assert a.shape == (40, 3) and np.isfinite(a).all() and not np.array_equal(a, b)
    assert abs(a.mean()) < 0.5 and 0.5 < a.std() < 1.5
    import torch
    from pdenv.sac import td_eps, _TAG_ACT_EPS
    t = td_eps(5, 9, 40, 3, "cpu", tag=_TAG_ACT_EPS).numpy()
    assert _TAG_ACT_EPS == an.TAG_ACT_EPS and np.abs(t - a.astype(np.float32)).max() <= 1e-6
    assert np.array_equal(td_eps(5, 9, 40, 3, "cpu").numpy(), td_eps(5, 9, 40, 3, "cpu", tag=64).numpy())
