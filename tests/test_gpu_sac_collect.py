"""GPU tests of the fused SAC collection (pd_collect_sac, PoweredDescentEnv.collect_sac,
SACCollector.collect): K collection steps of every env per call, the actor inside the step
kernel's fused-step loop, envs auto-resetting, every step's transition row in the replay ring
(sac_pytorch_powered_descent.py:160-183, sac_pytorch.py:27-35, 76-83).

The reference is the loop of K pd_step_sac_fused calls on a twin handle -- itself anchored to the
oracle and to torch (test_gpu_parity.py test_sac_ring_step_draws_rows_priorities,
test_gpu_sac_rollout.py) -- and every comparison is bit for bit.

1. equality with the per-step loop over whole episodes and in-kernel resets;
2. the ring's wrap and saturation;
3. guaranteed resets in a ragged tile, launch chaining (step_fuse) and call splitting;
4. slab mode;
5. refusals with nothing launched;
6. the facade, SACCollector.collect, and its per-step fallback.
"""
import pytest

from test_gpu_sac_rollout import LB, PT, WINDY, bits, landing_setup, make, make_actor, zero_action_actor

pytestmark = pytest.mark.gpu

MAX_PRIO = 2.5


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def make_buffer(env, capacity, position=0, size=0, sentinel=None):
    """A prioritized device ring for the handle with max priority 2.5, pre-positioned; sentinel:
    every row and priority filled with it first."""
    from pdenv.sac import DevicePrioritizedReplayBuffer
    buf = DevicePrioritizedReplayBuffer(capacity, env.obs_dim, env.action_dim, env.device)
    buf.max_priority = MAX_PRIO
    buf.max_prio_dev.fill_(MAX_PRIO)
    if sentinel is not None:
        buf.data.fill_(sentinel)
        buf.priorities.fill_(sentinel)
    buf.position, buf.size = position, size
    buf._sync_state_dev()
    return buf


def step_outputs(env, K):
    """The per-step outputs [K][N]...: eps (NaN-filled: a deterministic call writes none), reward,
    done, truncated, trunc_id."""
    import torch
    kw = dict(device=env.device)
    return dict(eps_out=torch.full((K, env.n, env.action_dim), float("nan"), dtype=torch.float32, **kw),
                reward=torch.full((K, env.n), float("nan"), dtype=env.dtype, **kw),
                done=torch.full((K, env.n), 9, dtype=torch.uint8, **kw),
                truncated=torch.full((K, env.n), 9, dtype=torch.uint8, **kw),
                trunc_id=torch.full((K, env.n), 99, dtype=torch.int8, **kw))


def ring_kw(buf):
    return dict(ring=buf.data, capacity=buf.capacity, ring_state=buf.state_dev, priorities=buf.priorities,
                max_priority=buf.max_prio_dev)


def per_step_loop(a, b, actor, K, deterministic, buf=None):
    """The comparator: handle `a` stepped by K pd_step_sac_fused calls (one launch per step, the
    actor in the kernel prologue on obs32) from its current state, its rows into `buf` (ring mode)
    or into a stacked [K, N, W] slab; the twin `b` (the same state) takes each step's float32
    action through pd_step for the reward, done, truncated and trunc_id in the handle's precision
    -- the same step bit for bit, tied to the first at every step by the replay row's reward and
    done and at the end by the state."""
    import torch
    from pdenv.sac import ActorKernel
    kern = ActorKernel(actor)
    N, S, A = a.n, a.obs_dim, a.action_dim
    obs = a.observe().float().contiguous()
    out = step_outputs(a, K)
    act = torch.empty(N, A, dtype=torch.float32, device=a.device)
    slabs = torch.empty(K, N, 2 * S + A + 2, dtype=torch.float32, device=a.device)
    mism = torch.zeros((), dtype=torch.int64, device=a.device)
    for t in range(K):
        start = buf.position if buf is not None else 0
        a.step_sac_fused(kern.S, kern.A, kern.H, kern.nl, kern.ptrs(), actor.log_std_min, actor.log_std_max,
                         actor.max_action, deterministic=deterministic, action=act, obs32=obs, eps_out=out["eps_out"][t],
                         **(ring_kw(buf) if buf is not None else dict(ring=slabs[t])))
        if buf is not None:
            buf.note_appended(N)
            slabs[t] = buf.rows(start, N)
        b.step_raw(act)
        out["reward"][t], out["done"][t] = b.reward_buf, b.done_buf
        out["truncated"][t], out["trunc_id"][t] = b.trunc_buf, b.trunc_id_buf
        mism += (slabs[t][:, S + A] != b.reward_buf.float()).sum() + (slabs[t][:, -1] != b.done_buf.float()).sum()
    assert int(mism) == 0, "the pd_step twin left the pd_step_sac_fused twin"
    assert torch.equal(bits(a.state), bits(b.state))
    out.update(obs32=obs, slabs=slabs)
    return out


def collect(env, actor, ks, deterministic, buf=None):
    """The calls under test: pd_collect_sac for each k of ks in turn (ring mode into buf, or slab
    mode), the per-step outputs and slabs of the calls concatenated.  obs32 starts as NaN: it is an
    output only."""
    import torch
    from pdenv.sac import ActorKernel
    kern = ActorKernel(actor)
    N, S, A = env.n, env.obs_dim, env.action_dim
    K = sum(ks)
    out = step_outputs(env, K)
    obs = torch.full((N, S), float("nan"), dtype=torch.float32, device=env.device)
    slabs = torch.full((K, N, 2 * S + A + 2), float("nan"), dtype=torch.float32, device=env.device)
    t = 0
    for k in ks:
        kw = {name: v[t:t + k] for name, v in out.items()}
        env.collect_sac(kern, k, deterministic=deterministic, obs32=obs,
                        **(ring_kw(buf) if buf is not None else dict(ring=slabs[t:t + k])), **kw)
        if buf is not None:
            start = buf.position
            buf.note_appended(k * N)
            if k:
                slabs[t:t + k] = buf.rows(start, k * N).reshape(k, N, -1)
        t += k
    out.update(obs32=obs, slabs=slabs)
    return out


def checkpoint(env):
    """The handle's checkpoint in a zeroed blob: pd_checkpoint_save writes the per-env buffers at
    16-byte aligned offsets and leaves the padding between them (261 envs: 11 bytes after the last
    byte-sized buffer) as it found it."""
    import ctypes as C
    import torch
    from pdenv import _lib as L
    blob = torch.zeros(int(env.lib.pd_checkpoint_size(env.h)), dtype=torch.uint8, device=env.device)
    L.check(env.lib.pd_checkpoint_save(env.h, C.c_void_p(blob.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)))
    return blob


def assert_same(got, want, names=None):
    import torch
    for name in names or want:
        x, y = got[name], want[name]
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert torch.equal(bits(x), bits(y)), f"{name}: {int((bits(x) != bits(y)).sum())} words differ"


def assert_same_handle_and_ring(env, a, buf=None, ref_buf=None):
    import torch
    assert torch.equal(checkpoint(env), checkpoint(a)), "handle checkpoint"
    for x, y in zip(env.episode_counters(), a.episode_counters()):
        assert torch.equal(x, y)
    if buf is not None:
        assert torch.equal(bits(buf.data), bits(ref_buf.data)), "ring rows"
        assert torch.equal(bits(buf.priorities), bits(ref_buf.priorities)), "priorities"
        assert buf.state_dev.tolist() == ref_buf.state_dev.tolist() == [ref_buf.position, ref_buf.size, 0]


@pytest.mark.parametrize("S,A,H,L,prec,windy,deterministic", [
    (2, 1, 256, 2, "f64", False, False),
    (2, 1, 128, 3, "f64", True, False),
    (5, 4, 256, 2, "f64", False, False),
    (2, 1, 256, 2, "f32", False, False),
    (2, 1, 256, 2, "f64", False, True),
    (5, 4, 128, 1, "f64", False, False),
])
def test_collect_equals_per_step_loop_bitwise(pd, S, A, H, L, prec, windy, deterministic):
    """pd_collect_sac(512) against 512 pd_step_sac_fused calls on a twin handle (same seed and
    config), 261 envs (16 full MLP tiles and one of 5): the whole ring, the priorities, the ring
    state, eps, the four per-step outputs, the final obs32, the handle checkpoint and the episode
    counters.  Every env crosses at least one in-kernel reset."""
    import torch
    N, K = 261, 512
    phase = PT if A == 1 else LB
    cfg = dict(precision=prec, seed=17, auto_reset=True, **(WINDY if windy else {}))
    actor = make_actor(S, A, H, L)
    a, b, env = (make(pd, N, phase, **cfg) for _ in range(3))
    for e in (a, b, env):
        e.reset()
    ref_buf, buf = make_buffer(a, K * N + 3), make_buffer(env, K * N + 3)
    ep0 = a.episode_counters()[0].clone()
    ref = per_step_loop(a, b, actor, K, deterministic, ref_buf)
    ep = a.episode_counters()[0]
    print("comparator episodes per env", int(ep.min()), int(ep.max()), "trunc ids",
          sorted(set(ref["trunc_id"].flatten().tolist())))
    # a condition on the inputs: every env crossed an in-kernel reset (its episode counter moved on
    # from the one the reset before the first step left)
    assert int(ep.min()) >= 1 and int((ep - ep0).min()) >= 1, \
        f"{int((ep - ep0 < 1).sum())} comparator envs never ended an episode in {K} steps"
    got = collect(env, actor, [K], deterministic, buf)
    assert_same(got, ref)
    assert_same_handle_and_ring(env, a, buf, ref_buf)
    assert bool(torch.isnan(got["eps_out"]).all()) == deterministic
    assert env.counters()["nan_events"] == 0 and a.counters()["nan_events"] == 0


def test_ring_wrap_and_saturation(pd):
    """A full ring pre-positioned 3 N + 2 rows before its end, K N + 5 rows in all: the K N rows of
    one call land modulo the capacity exactly as the per-step twin's, the size stays at the
    capacity, and only the written rows get a priority -- the other five keep the sentinel."""
    import torch
    N, K = 37, 40
    cap = K * N + 5
    pos = cap - 3 * N - 2
    actor = make_actor(2, 1)
    cfg = dict(seed=23, auto_reset=True)
    a, b, env = (make(pd, N, **cfg) for _ in range(3))
    for e in (a, b, env):
        e.reset()
    ref_buf, buf = (make_buffer(e, cap, pos, cap, sentinel=-7.0) for e in (a, env))
    ref = per_step_loop(a, b, actor, K, False, ref_buf)
    got = collect(env, actor, [K], False, buf)
    assert_same(got, ref)
    assert_same_handle_and_ring(env, a, buf, ref_buf)
    assert buf.state_dev.tolist() == [(pos + K * N) % cap, cap, 0]
    written = torch.zeros(cap, dtype=torch.bool, device=env.device)
    written[(pos + torch.arange(K * N, device=env.device)) % cap] = True
    assert int((~written).sum()) == 5
    assert bool((buf.priorities[written] == MAX_PRIO).all()) and bool((buf.priorities[~written] == -7.0).all())
    assert bool((buf.data[~written] == -7.0).all()) and bool((buf.data[written][:, -1] != -7.0).all())
    # step t's row of env i is row (position + t N + i) mod capacity
    rows = buf.data[(pos + torch.arange(K * N, device=env.device)) % cap].reshape(K, N, -1)
    assert torch.equal(bits(rows), bits(ref["slabs"]))


def test_resets_in_a_ragged_tile_chaining_and_splitting(pd):
    """48 envs whose first 8 land at their first step under the zero-action actor (deterministic),
    auto_reset on: the landing rows, the reset observation in the rows after them, the episode
    counters; then launches of 7 steps against 128, and two calls of 13 and 7 steps against one
    of 20 (deterministic and stochastic); a call of 0 steps changes nothing."""
    import torch
    N, K = 48, 20
    actor = zero_action_actor()
    env, blob = landing_setup(pd, N, auto_reset=True)
    S, A = env.obs_dim, env.action_dim
    start = checkpoint(env)
    fresh = env.observe()[8].float()
    ep0 = int(env.episode_counters()[0][0])

    def run(ks, deterministic, ring=True):
        env.restore(blob)
        buf = make_buffer(env, K * N + 9, 5, 5, sentinel=-7.0) if ring else None
        out = collect(env, actor, ks, deterministic, buf)
        out.update(blob=checkpoint(env), ep=env.episode_counters()[0])
        if ring:
            out.update(ring=buf.data, prio=buf.priorities, ring_state=buf.state_dev)
        return out

    one = run([1], True)
    assert bool((one["done"][0, :8] == 1).all()) and bool((one["done"][0, 8:] == 0).all())
    assert one["ep"].tolist() == [ep0 + 1] * 8 + [ep0] * 40, "the landed envs are in their next episode after the first step"
    assert torch.equal(one["obs32"][:8], fresh.expand(8, S)) and torch.equal(one["obs32"][8:], one["slabs"][0, 8:, S + A + 1:-1])
    full = run([K], True)
    sl = full["slabs"]
    assert bool((sl[0, :8, -1] == 1).all()) and bool((full["done"][0, :8] == 1).all()) and bool((sl[0, 8:, -1] == 0).all())
    # the landed envs' next rows start from the reset observation, the others' from their next_state
    assert torch.equal(sl[1, :8, :S], fresh.expand(8, S)) and not torch.equal(sl[0, :8, S + A + 1:-1], fresh.expand(8, S))
    assert torch.equal(sl[1, 8:, :S], sl[0, 8:, S + A + 1:-1])
    assert bool((sl[:, :, S:S + A] == 0).all())
    assert_same(one, {k: v[:1] for k, v in full.items() if k in ("slabs", "reward", "done", "truncated", "trunc_id")})
    assert env.tuning()["step_fuse"] == 128
    for deterministic in (True, False):
        want = full if deterministic else run([K], False)
        env.set_tuning(step_fuse=7)
        assert_same(run([K], deterministic), want)
        env.set_tuning(step_fuse=128)
        assert_same(run([13, 7], deterministic), want)
        assert_same(run([0, K, 0], deterministic), want)
        assert_same(run([K], deterministic, ring=False), want, [k for k in want if k not in ("ring", "prio", "ring_state")])
    assert not bool(torch.isnan(want["eps_out"]).any()) and bool((want["slabs"][:, :, S:S + A] != 0).any())
    zero = run([0], True)
    assert torch.equal(zero["blob"], start) and zero["ring_state"].tolist() == [5, 5, 0]
    assert bool((zero["ring"] == -7.0).all()) and bool(torch.isnan(zero["obs32"]).all())
    assert env.counters()["nan_events"] == 0


def test_slab_mode(pd):
    """ring_state NULL: the [K, N, W] slab equals the stacked per-step slabs; capacity and
    priorities are ignored (a priorities tensor given keeps its sentinel)."""
    import torch
    from pdenv.sac import ActorKernel
    N, K = 37, 9
    actor = make_actor(5, 4, H=128)
    cfg = dict(seed=31, auto_reset=True)
    a, b, env = (make(pd, N, LB, **cfg) for _ in range(3))
    for e in (a, b, env):
        e.reset()
    ref = per_step_loop(a, b, actor, K, False)
    got = collect(env, actor, [K], False)
    assert_same(got, ref)
    assert_same_handle_and_ring(env, a)
    # the raw call with a priorities tensor and no ring state
    env2 = make(pd, N, LB, **cfg)
    env2.reset()
    slab = torch.empty_like(got["slabs"])
    prio = torch.full((K * N,), -7.0, dtype=torch.float32, device=env.device)
    env2.collect_sac(ActorKernel(actor), K, ring=slab, capacity=0, priorities=prio,
                     max_priority=torch.full((1,), MAX_PRIO, device=env.device))
    assert torch.equal(bits(slab), bits(ref["slabs"])) and bool((prio == -7.0).all())


def test_refusals_launch_nothing(pd):
    """UNSUPPORTED for a handle that does not step 16 lanes per env and for hidden 512, INVALID for
    n_steps N > capacity and n_steps < 0 -- the cause in pd_last_error, episode counters, handle
    and ring state untouched."""
    import torch
    from pdenv import _lib as L
    from pdenv.sac import ActorKernel
    N = 37
    small, wide = make_actor(2, 1), make_actor(2, 1, H=512)
    cases = ((dict(lanes_per_env=2), small, 4, 4 * N, L.PD_ERR_UNSUPPORTED, b"16 lanes per env"),
             (dict(), wide, 4, 4 * N, L.PD_ERR_UNSUPPORTED, b"512"),
             (dict(), small, 4, 4 * N - 1, L.PD_ERR_INVALID, b"capacity"),
             (dict(), small, -1, 4 * N, L.PD_ERR_INVALID, b"n_steps"))
    for kw, actor, k, cap, status, cause in cases:
        env = make(pd, N, seed=5, **kw)
        env.reset()
        kern = ActorKernel(actor)
        buf = make_buffer(env, cap, 3, 7, sentinel=-7.0)
        before, blob = [x.clone() for x in env.episode_counters()], checkpoint(env)
        obs = torch.full((N, 2), float("nan"), dtype=torch.float32, device=env.device)
        st = env.lib.pd_collect_sac(env.h, kern.S, kern.A, kern.H, kern.nl, kern.ptrs(), 0, -20.0, 2.0, 1.0, k,
                                    buf.data.data_ptr(), cap, buf.state_dev.data_ptr(), buf.priorities.data_ptr(),
                                    buf.max_prio_dev.data_ptr(), obs.data_ptr(), None, None, None, None, None, None)
        assert st == status and cause in env.lib.pd_last_error(), (st, env.lib.pd_last_error())
        with pytest.raises(L.PdError) as err:
            env.collect_sac(kern, k, obs32=obs, **ring_kw(buf))
        assert err.value.status == status
        assert all(torch.equal(x, y) for x, y in zip(before, env.episode_counters())), "nothing was launched"
        assert torch.equal(blob, checkpoint(env)) and buf.state_dev.tolist() == [3, 7, 0]
        assert bool((buf.data == -7.0).all()) and bool(torch.isnan(obs).all())
    # zero steps: PD_OK with nothing looked at but the actor and the handle (ring and outputs NULL)
    env, kern = make(pd, N, seed=5), ActorKernel(small)
    env.reset()
    blob = checkpoint(env)
    assert env.lib.pd_collect_sac(env.h, kern.S, kern.A, kern.H, kern.nl, kern.ptrs(), 0, -20.0, 2.0, 1.0, 0, None, 0,
                                  None, None, None, None, None, None, None, None, None, None) == L.PD_OK
    assert torch.equal(blob, checkpoint(env))


def collector_state(c):
    b = c.buffer
    return dict(data=b.data, prio=b.priorities, ring_state=b.state_dev, obs=c.obs,
                host=__import__("torch").tensor([b.position, b.size, c.steps]), blob=checkpoint(c.env))


def test_collector_facade_and_fallback(pd):
    """SACCollector.collect(24) against 24 step() calls on a twin collector: buffer rows,
    priorities, host and device position and size, obs and the returned rows; a step() after it
    continues identically.  A handle at 2 lanes per env and a hidden-512 actor take the per-step
    fallback: the same bits again, with the logged per-step outputs tied to the rows."""
    import torch
    from pdenv.sac import SACCollector
    N, K = 37, 24

    def pair(actor, **kw):
        cs = []
        for _ in range(2):
            env = make(pd, N, seed=13, auto_reset=True, **kw)
            cs.append(SACCollector(env, actor, make_buffer(env, 3 * K * N + 11, 8, 8, sentinel=-7.0)))
        return cs

    for actor, kw, fused in ((make_actor(2, 1), dict(), True), (make_actor(2, 1), dict(lanes_per_env=2), False),
                             (make_actor(2, 1, H=512), dict(), False)):
        c, ref = pair(actor, **kw)
        launches = []
        real = c.env.collect_sac
        c.env.collect_sac = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        out = step_outputs(c.env, K)
        rows = c.collect(K, rewards=out["reward"], done=out["done"], truncated=out["truncated"], trunc_id=out["trunc_id"])
        want = torch.cat([ref.step().clone() for _ in range(K)])
        assert rows.shape == (K * N, c.buffer.width) and torch.equal(bits(rows), bits(want))
        assert_same(collector_state(c), collector_state(ref))
        assert c.buffer.position == 8 + K * N and c.buffer.size == 8 + K * N and c.steps == K
        assert (rows.data_ptr() == c.buffer.data[8].data_ptr()) == fused, "a view of the ring's rows in ring mode"
        assert launches, "the library was asked (and answered PD_ERR_UNSUPPORTED for the two fallbacks)"
        S, A = c.env.obs_dim, c.env.action_dim
        r3 = rows.reshape(K, N, -1)
        assert torch.equal(r3[:, :, S + A], out["reward"].float()) and torch.equal(r3[:, :, -1], out["done"].float())
        assert bool((out["truncated"] <= 1).all()) and bool(((out["trunc_id"] != 0) == (out["truncated"] != 0)).all())
        # step() and collect() alternate
        assert torch.equal(bits(c.step()), bits(ref.step()))
        r2 = c.collect(3)
        assert torch.equal(bits(r2), bits(torch.cat([ref.step().clone() for _ in range(3)])))
        assert_same(collector_state(c), collector_state(ref))
        assert c.collect(0).shape == (0, c.buffer.width)
        assert_same(collector_state(c), collector_state(ref))
    # no buffer on this rank: the rows of a local slab, a fresh tensor
    actor = make_actor(2, 1)
    c, ref = (SACCollector(make(pd, N, seed=13, auto_reset=True), actor) for _ in range(2))
    rows = c.collect(5)
    assert rows.shape == (5 * N, 7) and torch.equal(bits(rows), bits(torch.cat([ref.step().clone() for _ in range(5)])))
    assert torch.equal(bits(c.obs), bits(ref.obs)) and torch.equal(checkpoint(c.env), checkpoint(ref.env))
    # k N beyond the capacity: the per-step loop, the ring wrapping as step() wraps it
    actor = make_actor(2, 1)
    c, ref = (SACCollector(e, actor, make_buffer(e, 2 * N + 5)) for e in (make(pd, N, seed=13), make(pd, N, seed=13)))
    rows = c.collect(5)
    assert torch.equal(bits(rows), bits(torch.cat([ref.step().clone() for _ in range(5)])))
    assert_same(collector_state(c), collector_state(ref))
