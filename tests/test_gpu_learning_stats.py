"""GPU checks of pd_sac_learning_stats (csrc/pdsacstats.hip), LearningStats on the kernel,
sac_update(..., stats=) and pdenv.agent.SACPyTorch on the device, against the NumPy binary64 model
(tests/learning_stats_ref.py).

The bound of the computed columns: binary64 two-pass sums of n <= 8232 terms err by at most about
8 n 2^-53 (max|x| / std) relative to the column's scale (max|x| of the series for mean and std,
kurtosis + 3 for the kurtosis); the inputs meet max|x| <= 64 std, so that is 4.7e-10 at the largest
series (B = 1029, A = 8) and under 2^-30 = 9.3e-10 -- some 6000 times below the float32 reference's own
deviation from the model.  min and max are equal as numbers, the copied scalars, step and per_beta
have the same bits, alpha_value is within 2 float32 ulp of exp in binary64."""
import ctypes as C

import numpy as np
import pytest
import torch

import learning_stats_ref as M

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -30
NAN = float("nan")


def _lib():
    import pdenv
    from pdenv import _lib
    return pdenv.load(), _lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _call(S, A, rows, q, tq, lp, w, scalars, log_alpha, per_beta, step, out):
    """One pd_sac_learning_stats call on device tensors; scalars: critic_loss, actor_loss, alpha_loss,
    max_priority, actor_grad_norm, critic_grad_norm (each a [1] tensor or None)."""
    L, lib = _lib()
    st = L.pd_sac_learning_stats(int(rows.shape[0]), S, A, _ptr(rows), int(rows.shape[1]), _ptr(q), _ptr(tq), _ptr(lp),
                                 _ptr(w), _ptr(scalars[0]), _ptr(scalars[1]), _ptr(scalars[2]), _ptr(log_alpha),
                                 _ptr(scalars[3]), _ptr(scalars[4]), _ptr(scalars[5]), per_beta, step, _ptr(out),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.PD_OK, L.pd_last_error()


def _case(seed, S, A, B, width=None, per=True, scalars=True):
    """Seeded inputs on the host and the device, and the model's row and scales."""
    rng = np.random.default_rng(seed)
    rows, q, tq, lp, w = M.make_inputs(rng, S, A, B, width=width, per=per)
    sc = np.abs(rng.standard_normal(6)).astype(np.float32) + np.float32(0.25)
    sc[:3] *= np.float32(-1.0)
    la = np.float32(-1.0 - 0.01 * seed)
    have = [scalars] * 6
    have[3] = scalars and per
    vals = [sc[k] if have[k] else None for k in range(6)]
    step, beta = 1000 + seed, 0.4 + 1e-3 * seed
    model, scale = M.model_row(rows, q, tq, lp, S, A, weights=w, critic_loss=vals[0], actor_loss=vals[1],
                               alpha_loss=vals[2], log_alpha=la, max_priority=vals[3], actor_grad_norm=vals[4],
                               critic_grad_norm=vals[5], per_beta=beta, step=step, scales=True)
    dev = dict(rows=_dev(rows), q=_dev(q), tq=_dev(tq), lp=_dev(lp), w=_dev(w),
               scalars=[None if v is None else _dev(np.array([v], dtype=np.float32)) for v in vals],
               la=_dev(np.array([la], dtype=np.float32)))
    return dict(S=S, A=A, B=B, host=(rows, q, tq, lp, w), dev=dev, beta=beta, step=step, model=model, scale=scale)


def _run(c, out=None):
    d = c["dev"]
    out = torch.full((M.N_STATS,), 7.25, dtype=torch.float64, device="cuda") if out is None else out
    _call(c["S"], c["A"], d["rows"], d["q"], d["tq"], d["lp"], d["w"], d["scalars"], d["la"], c["beta"], c["step"], out)
    return out.cpu().numpy()


def _check_row(got, model, scale, what=""):
    dev = np.abs(got - model) / np.abs(scale)
    with np.errstate(invalid="ignore"):
        print(f"{what}: largest |got - model| / scale over the bounded columns "
              f"{np.nanmax(np.append(dev[M.BOUNDED], 0.0)):.3e} (bound {BOUND:.3e}), alpha {dev[M.ALPHA]:.3e}")
    assert M.same_number(got[M.MINMAX], model[M.MINMAX]), [(M.NAMES[k], got[k], model[k]) for k in M.MINMAX]
    assert M.same_bits(got[M.COPIED], model[M.COPIED]), [(M.NAMES[k], got[k], model[k]) for k in M.COPIED]
    ok = M.within(got[M.BOUNDED], model[M.BOUNDED], scale[M.BOUNDED], BOUND)
    assert ok.all(), [(M.NAMES[M.BOUNDED[i]], got[M.BOUNDED[i]], model[M.BOUNDED[i]]) for i in np.nonzero(~ok)[0]]
    assert abs(got[M.ALPHA] - model[M.ALPHA]) <= 2 * np.spacing(np.float32(model[M.ALPHA]))


# ------------------------------------------------------------------ the kernel against the model
SHAPES = [  # S, A, B, width, per, scalars
    (1, 1, 1, None, True, True), (2, 1, 2, None, False, False), (5, 4, 63, None, True, False),
    (16, 8, 64, None, False, True), (2, 1, 65, 7, True, True), (5, 4, 261, 16, True, True),
    (2, 1, 261, 7, False, True), (16, 8, 1029, None, True, True), (1, 1, 1029, 9, True, False),
    (16, 8, 2, 42, True, True), (5, 4, 1, None, False, False)]


@pytest.mark.parametrize("S,A,B,width,per,scalars", SHAPES)
def test_kernel_against_the_model(S, A, B, width, per, scalars):
    c = _case(S * 7 + A + B, S, A, B, width=width, per=per, scalars=scalars)
    if B > 2:
        for name, x in M.series_of(*c["host"][:4], S, A).items():
            for s in (x if name == "state" else [x]):
                assert np.abs(s).max() <= 64 * s.astype(np.float64).std()
    got = _run(c)
    _check_row(got, c["model"], c["scale"], f"(S, A, B) = {(S, A, B)}")
    if not per:
        assert np.isnan(got[32:35]).all()
    if not scalars:
        assert np.isnan(got[[16, 17, 18, 34, 35, 36]]).all()
    if B == 1:
        r = dict(zip(M.NAMES, got))
        one = ("state", "reward") + (("action",) if A == 1 else ())     # (the action series has B x A values)
        assert all(r[f"{p}_std"] == 0 for p in one + ("q_value", "log_prob", "target_q"))
        assert all(np.isnan(r[f"{p}_kurtosis"]) for p in one)


def test_special_values():
    """A constant series: std 0, kurtosis NaN.  One NaN in a series: its statistics NaN, min and max
    included, the other series' unchanged."""
    S, A, B = 3, 2, 130
    c = _case(3, S, A, B)
    base = _run(c)
    d = c["dev"]
    rows0 = d["rows"].clone()
    d["rows"][:, 1] = 2.5                                      # state dimension 1 constant
    d["rows"][:, S + A] = -0.75                                # the reward constant
    got = dict(zip(M.NAMES, _run(c)))
    assert got["reward_std"] == 0 and np.isnan(got["reward_kurtosis"])
    assert got["reward_mean"] == got["reward_min"] == got["reward_max"] == -0.75
    assert np.isnan(got["state_kurtosis"]) and np.isfinite(got["state_std"])      # (the mean over the dimensions)
    assert got["action_kurtosis"] == base[10]
    d["rows"].copy_(rows0)
    cols = {"state": range(1, 6), "action": range(6, 11), "reward": range(11, 16), "q_value": range(20, 24),
            "log_prob": range(24, 28), "target_q": range(28, 32), "weights": [33]}
    where = {"state": ("rows", (77, 2)), "action": ("rows", (129, S + 1)), "reward": ("rows", (0, S + A)),
             "q_value": ("q", (64, 0)), "log_prob": ("lp", (65, 0)), "target_q": ("tq", (128, 0)), "weights": ("w", (3, 0))}
    for name, (key, at) in where.items():
        keep = d[key].clone()
        d[key][at] = NAN
        if name == "q_value":                                  # (fminf(q1, q2) drops a NaN on one side alone)
            d[key][at[0], 1] = NAN
        got = _run(c)
        d[key].copy_(keep)
        hit = list(cols[name])
        assert np.isnan(got[hit]).all(), (name, got[hit])
        rest = [k for k in range(M.N_STATS) if k not in hit]
        assert M.same_bits(got[rest], base[rest]), name
    assert M.same_bits(_run(c), base)


def test_determinism_and_bystanders():
    """Two calls give equal bytes; only out_row is written: the rows around it and the inputs are
    intact."""
    c = _case(11, 5, 4, 517, width=20)
    d = c["dev"]
    tensors = [d["rows"], d["q"], d["tq"], d["lp"], d["w"], d["la"]] + d["scalars"]
    before = [t.clone() for t in tensors]
    ring = torch.full((3, M.N_STATS), -123.5, dtype=torch.float64, device="cuda")
    first = _run(c, ring[1]).copy()
    ring[1].fill_(55.0)
    second = _run(c, ring[1]).copy()
    assert first.tobytes() == second.tobytes()
    assert bool((ring[0] == -123.5).all()) and bool((ring[2] == -123.5).all())
    assert all(torch.equal(a, b) for a, b in zip(before, tensors))
    _check_row(first, c["model"], c["scale"], "bystanders")


# ------------------------------------------------------------------ a real learner
S_, A_, H_, B_ = 2, 1, 128, 64


def _slab(n, seed=0):
    rng = np.random.default_rng(seed)
    slab = rng.standard_normal((n, 2 * S_ + A_ + 2)).astype(np.float32)
    slab[:, S_:S_ + A_] = np.tanh(slab[:, S_:S_ + A_])
    slab[:, -1] = (np.arange(n) % 5 == 3)
    return torch.from_numpy(slab).cuda()


def _learner(per=True, clip=True, seed=0):
    """The hand-wired update, its nets created in the agent's order from torch.manual_seed(seed)."""
    from pdenv.sac import (Actor, ActorUpdate, Critic, CriticUpdate, DeviceReplayBuffer, KernelPrioritizedReplayBuffer,
                           TdTarget)
    torch.manual_seed(seed)
    actor, critic, target = Actor(S_, A_, H_, 2).cuda(), Critic(S_, A_, H_, 2).cuda(), Critic(S_, A_, H_, 2).cuda()
    target.load_state_dict(critic.state_dict())
    aopt, copt = torch.optim.Adam(actor.parameters(), lr=3e-4), torch.optim.Adam(critic.parameters(), lr=3e-4)
    la = torch.tensor([np.log(0.2)], dtype=torch.float32, device="cuda", requires_grad=True)
    lopt = torch.optim.Adam([la], lr=3e-4)
    buf = (KernelPrioritizedReplayBuffer if per else DeviceReplayBuffer)(512, S_, A_, torch.device("cuda"))
    buf.add_batch(_slab(300))
    td = TdTarget(actor, target, la, 0.99)
    cu = CriticUpdate(critic, target, copt, tau=0.005, max_grad_norm=1.0 if clip else None)
    au = ActorUpdate(actor, critic, la, aopt, lopt, target_entropy=-A_, max_grad_norm=1.0 if clip else None)
    assert td.kernel and cu.kernel and au.kernel
    return dict(actor=actor, critic=critic, target=target, la=la, aopt=aopt, copt=copt, lopt=lopt, buf=buf, td=td, cu=cu,
                au=au)


def _state_tensors(k):
    out = [p.data for net in (k["actor"], k["critic"], k["target"]) for p in net.parameters()] + [k["la"].data]
    for opt in (k["aopt"], k["copt"], k["lopt"]):
        for st in opt.state.values():
            out += [st["exp_avg"], st["exp_avg_sq"], st["step"].cpu()]
    if hasattr(k["buf"], "priorities"):
        out += [k["buf"].priorities, k["buf"].max_prio_dev]
    return out


class _Tee:
    def __init__(self, *stats):
        self.stats, self.inputs = stats, []

    def record(self, rows, tq, cu, au, lp, w, buf):
        for s in self.stats:
            s.record(rows, tq, cu, au, lp, w, buf)
        self.inputs.append([None if t is None else t.detach().cpu().numpy().copy() for t in (rows, au.q, tq, lp, w)])


def test_learning_stats_on_the_kernel_equals_the_torch_path():
    """5 recorded updates of a real sac_update into rings of 3 rows: the flushes cover a full ring
    and a wrapped one."""
    from pdenv.sac import LearningStats, sac_update
    k = _learner()
    dev = torch.device("cuda")
    on_kernel, on_torch = LearningStats(S_, A_, dev, capacity=3), LearningStats(S_, A_, dev, capacity=3, kernel=False)
    tee = _Tee(on_kernel, on_torch)
    for n in range(5):
        sac_update(k["buf"], k["td"], k["cu"], k["au"], B_, stats=tee)
        assert on_kernel.last_kernel is True and on_torch.last_kernel is False
        if n == 3:
            assert on_kernel._flushed == 3                     # the ring filled and flushed itself
    a, b = on_kernel.rows, on_torch.rows                       # (the rows 3, 4 come from slots 0, 1)
    assert a.shape == b.shape == (5, 37) and list(a[:, 0]) == [0, 1, 2, 3, 4]
    assert list(on_kernel.to_dict()) == M.NAMES
    for n, (rows, q, tq, lp, w) in enumerate(tee.inputs):
        scale = M.model_row(rows, q, tq, lp, S_, A_, weights=w, scales=True)[1]
        scale[M.ALPHA] = a[n, M.ALPHA]
        dev_rel = np.abs(a[n] - b[n]) / np.abs(scale)
        print(f"update {n}: largest |kernel - torch| / scale {np.nanmax(dev_rel):.3e}")
        assert M.same_number(a[n, M.MINMAX], b[n, M.MINMAX]) and M.same_bits(a[n, M.COPIED], b[n, M.COPIED])
        assert M.within(a[n, M.BOUNDED], b[n, M.BOUNDED], scale[M.BOUNDED], BOUND).all()
        assert abs(a[n, M.ALPHA] - b[n, M.ALPHA]) <= 2 * np.spacing(np.float32(a[n, M.ALPHA]))
    assert np.all(np.diff(a[:, 32]) > 0) and np.all(a[:, 34] >= 1.0)       # beta anneals; the max priority


@pytest.mark.parametrize("per", [True, False])
def test_sac_update_with_stats_leaves_the_learner_unchanged(per):
    from pdenv.sac import LearningStats, sac_update
    runs = []
    for with_stats in (False, True):
        k = _learner(per=per)
        stats = LearningStats(S_, A_, torch.device("cuda"), capacity=2) if with_stats else None
        torch.manual_seed(5)                                   # (the uniform buffer draws from torch's generator)
        for _ in range(3):
            if with_stats:
                sac_update(k["buf"], k["td"], k["cu"], k["au"], B_, stats=stats)
            else:
                sac_update(k["buf"], k["td"], k["cu"], k["au"], B_)
        runs.append([t.clone() for t in _state_tensors(k)])
        if with_stats:
            assert stats.last_kernel is True and len(stats) == 3
            assert list(stats.to_dict()) == (M.NAMES if per else M.NAMES[:32] + M.NAMES[35:])
    assert len(runs[0]) == len(runs[1]) > 40
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_agent_against_the_hand_wired_update():
    from pdenv.agent import SACPyTorch
    from pdenv.sac import KernelPrioritizedReplayBuffer, LearningStats, sac_update
    k = _learner(per=True, clip=True)
    stats = LearningStats(S_, A_, torch.device("cuda"), capacity=100)
    torch.manual_seed(0)
    agent = SACPyTorch(S_, A_, hidden_dim_actor=H_, hidden_dim_critic=H_, batch_size=B_, buffer_size=512, device="cuda",
                       use_per=True, clip_gradients=True)
    assert isinstance(agent.replay_buffer, KernelPrioritizedReplayBuffer)
    assert agent.td_target.kernel and agent.critic_update.kernel and agent.actor_update.kernel
    agent.update()
    assert agent.updates == 0                                  # an empty buffer: nothing happens
    agent.replay_buffer.add_batch(_slab(300))
    for _ in range(3):
        sac_update(k["buf"], k["td"], k["cu"], k["au"], B_, stats=stats)
        agent.update()
    assert agent.updates == 3 and agent.stats.last_kernel is True
    mine = dict(actor=agent.actor, critic=agent.critic, target=agent.critic_target, la=agent.log_alpha,
                aopt=agent.actor_optimizer, copt=agent.critic_optimizer, lopt=agent.alpha_optimizer, buf=agent.replay_buffer)
    for a, b in zip(_state_tensors(k), _state_tensors(mine)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert agent.stats.rows.tobytes() == stats.rows.tobytes()
    d = agent.learning_stats
    assert list(d) == M.NAMES and d["step"] == [0, 1, 2] and d == stats.to_dict()
    a = agent.select_action(np.array([0.3, -0.2]), deterministic=True)
    assert a.shape == (A_,) and a.dtype == np.float32
