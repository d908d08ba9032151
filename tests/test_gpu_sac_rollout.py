"""GPU tests of the fused SAC evaluation rollouts (pd_rollout_sac, PoweredDescentEnv.rollout_sac,
pdenv.sac.evaluate_agent): whole actor-driven episodes in the step kernel, the driver's
evaluate_agent / visualize_trajectory loops (sac_pytorch_powered_descent.py:234-251, :354-376).

1. bit-for-bit equality with the per-step loop of pd_step_sac_fused (a twin handle);
2. the reference anchor, shadowed (tests/shadow.py: the env is chaotic, so every step is
   teacher-forced from the device's own snapshot) plus the torch Actor on the snapshot's
   observation;
3. mixed episode lengths in one tile, the landing (done) path, the step cap and its
   continuation, launch chaining (step_fuse invariance), repeatability;
4. refusals (lanes per env != 16, hidden 512) and evaluate_agent's per-step fallback;
5. the facade's summary numbers.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

PT, LB = "landing_burn_pure_throttle", "landing_burn"
WINDY = dict(enable_wind=True, stochastic_wind=True, wind_percentile=None, tilt_sigma_rad=0.05)


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def make(pd, n, phase=PT, **kw):
    kw.setdefault("lanes_per_env", 16)
    return pd.PoweredDescentEnv(n, flight_phase=phase, mode="rl", **kw)


def make_actor(S, A, H=256, L=2, seed=3):
    import torch
    from pdenv.sac import Actor
    torch.manual_seed(seed)
    return Actor(S, A, hidden_dim=H, n_hidden_layers=L).cuda()


def bits(t):
    """The tensor's bit pattern (NaN rows compare equal to the NaN they were filled with)."""
    import torch
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.int8}[t.element_size()])


def traces(env, T):
    import torch
    a = torch.full((T, env.n, env.action_dim), float("nan"), dtype=torch.float32, device=env.device)
    r = torch.full((T, env.n), float("nan"), dtype=env.dtype, device=env.device)
    return a, r


def per_step_loop(pd, actor, N, T, deterministic, phase, cfg):
    """The comparator: a twin handle stepped by the EXISTING pd_step_sac_fused loop (actor in the
    kernel prologue on obs32, one launch per step), each env's first episode booked here.  The SAC
    step calls return the reward only as the replay row's float32, so a second twin takes the same
    float32 actions through pd_step for the reward / done / truncated / trunc_id in the handle's
    precision (the same step bit for bit: tests/test_gpu_parity.py
    test_sac_ring_step_draws_rows_priorities); it is tied to the first at every step (replay-row
    reward and done) and by the final state."""
    import torch
    from pdenv.sac import ActorKernel
    a, b = make(pd, N, phase, **cfg), make(pd, N, phase, **cfg)
    kern = ActorKernel(actor)
    S, A = a.obs_dim, a.action_dim
    obs = a.reset().float().contiguous()
    b.reset()
    dev = a.device
    act = torch.empty(N, A, dtype=torch.float32, device=dev)
    slab = torch.empty(N, 2 * S + A + 2, dtype=torch.float32, device=dev)
    live = torch.ones(N, dtype=torch.bool, device=dev)
    ret = torch.zeros(N, dtype=a.dtype, device=dev)
    steps = torch.zeros(N, dtype=torch.int32, device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    tid = torch.zeros(N, dtype=torch.int8, device=dev)
    acts, rews = traces(a, T)
    mism = torch.zeros((), dtype=torch.int64, device=dev)
    for t in range(T):
        a.step_sac_fused(kern.S, kern.A, kern.H, kern.nl, kern.ptrs(), actor.log_std_min, actor.log_std_max,
                         actor.max_action, deterministic=deterministic, ring=slab, action=act, obs32=obs)
        b.step_raw(act)
        r = b.reward_buf
        mism += (slab[:, S + A] != r.float()).sum() + (slab[:, -1] != b.done_buf.float()).sum()
        ret = torch.where(live, ret + r, ret)              # step order, handle precision
        steps += live
        acts[t] = torch.where(live[:, None], act, acts[t])
        rews[t] = torch.where(live, r, rews[t])
        ended = live & ((b.done_buf | b.trunc_buf) != 0)
        done = torch.where(ended, b.done_buf, done)
        tid = torch.where(live, b.trunc_id_buf, tid)
        live = live & ~ended
    assert int(mism) == 0, "the pd_step twin left the pd_step_sac_fused twin"
    assert torch.equal(bits(a.state), bits(b.state))
    # a condition on the inputs: every comparator episode ended within the cap
    assert not bool(live.any()), f"{int(live.sum())} comparator episodes did not end in {T} steps"
    return ret, steps, done, tid, acts, rews


@pytest.mark.parametrize("S,A,H,L,prec,windy,deterministic", [
    (2, 1, 256, 2, "f64", False, True),
    (2, 1, 128, 3, "f64", True, True),
    (5, 4, 256, 2, "f64", False, True),
    (2, 1, 256, 2, "f32", False, True),
    (2, 1, 256, 2, "f64", False, False),
    (5, 4, 128, 1, "f64", False, True),
])
def test_rollout_equals_per_step_loop_bitwise(pd, S, A, H, L, prec, windy, deterministic):
    """pd_rollout_sac against a loop of pd_step_sac_fused calls on a twin handle (same seed and
    config): steps, done, trunc_id, returns and both traces up to each env's length, bit for bit;
    trace rows past an env's length keep the NaN they were filled with.  261 envs: 16 full MLP
    tiles and one of 5; auto_reset is ON in the config, and the rollout must ignore it."""
    import torch
    from pdenv.sac import ActorKernel
    N, T = 261, 512
    phase = PT if A == 1 else LB
    cfg = dict(precision=prec, seed=17, auto_reset=True, **(WINDY if windy else {}))
    actor = make_actor(S, A, H, L)
    ref = per_step_loop(pd, actor, N, T, deterministic, phase, cfg)
    env = make(pd, N, phase, **cfg)
    acts, rews = traces(env, T)
    out = env.rollout_sac(ActorKernel(actor), deterministic=deterministic, reset=True, max_steps=T,
                          actions_out=acts, rewards_out=rews)
    names = ("returns", "steps", "done", "trunc_id", "actions", "rewards")
    print("episode lengths", int(ref[1].min()), int(ref[1].max()), "trunc ids", sorted(set(ref[3].tolist())))
    for name, got, want in zip(names, out + (acts, rews), ref):
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert torch.equal(bits(got), bits(want)), f"{name}: {int((bits(got) != bits(want)).sum())} words differ"
    # rows past an env's length: still the NaN fill; rows before it: written
    t = torch.arange(T, device=env.device)[:, None]
    past = t >= out[1][None, :]
    assert bool(torch.isnan(rews[past]).all()) and bool(torch.isfinite(rews[~past]).all())
    assert bool(torch.isnan(acts[past]).all()) and bool(torch.isfinite(acts[~past]).all())
    assert env.counters()["nan_events"] == 0


# ---------------------------------------------------------------------------------- shadowing
def rollout_records(env, kern, blob, K, it, reset, deterministic=True):
    """rollout_sac(max_steps=k) for k = 0..K from the same start (the handle is put back to `blob`
    first: with reset=True that rewinds the episode counter, so every k resets into the same
    episode -- same tilt, sigmas, percentile and gust draws).  Per k: the sampled envs' complete
    state (shadow.snapshot), their float32 observation, the call's outputs and traces."""
    import torch
    from shadow import snapshot
    recs = []
    for k in range(K + 1):
        env.restore(blob)
        acts, rews = traces(env, k)
        ret, steps, done, tid = env.rollout_sac(kern, deterministic=deterministic, reset=reset, max_steps=k,
                                                actions_out=acts, rewards_out=rews)
        recs.append(dict(snap=snapshot(env, it), obs=env.observe()[it].float().cpu(), ret=ret[it].cpu().numpy(),
                         steps=steps[it].cpu().numpy(), done=done[it].cpu().numpy(), tid=tid[it].cpu().numpy(),
                         acts=acts[:, it].cpu().numpy(), rews=rews[:, it].cpu().numpy()))
    return recs


def shadow_rollout(oracle_mod, recs, idx, phase, seed, tilt, wind, actor=None):
    """Teacher-forced parity of the rollout on envs `idx`: for every step k -> k + 1 (k + 1 below
    the longest call's cap) an env takes, the oracle loads the device's complete state after k
    steps (shadow._load), takes one env step with the action the kernel recorded in
    actions_out[k], and must give the device's state after k + 1 steps, rewards_out[k], the
    flags and ids at the tolerances of shadow.check_stats; the returns add the recorded rewards
    exactly; an env that ended stays frozen bit for bit.  actor: the torch Actor on snapshot k's
    float32 observation gives tanh(mean) max_action within 2e-5 + 1e-4 |mean| of actions_out[k]
    (the head bound of test_sac_actor_kernel_vs_torch; tanh is 1-Lipschitz)."""
    import torch
    from shadow import _load
    L, P = oracle_mod.lib(), oracle_mod.params()
    o, E = oracle_mod.OrcOut(), oracle_mod.OrcEnv()
    fin = recs[-1]
    K = len(recs) - 2
    st = dict(steps=0, ended=0, frozen=0, done=0, max_err=np.zeros(11), max_rew=0.0, max_obs=0.0, max_filt=0.0,
              max_act=0.0, trunc_ids=set())
    for j, g in enumerate(idx):
        for k in range(K):
            a, b = recs[k], recs[k + 1]
            ctx = f"env {g} step {k}"
            if int(fin["steps"][j]) <= k:          # ended before this step: frozen, nothing written
                for key in a["snap"]:
                    assert np.array_equal(a["snap"][key][j], b["snap"][key][j]), (ctx, key)
                assert a["ret"][j] == b["ret"][j] and a["steps"][j] == b["steps"][j] == fin["steps"][j], ctx
                assert a["done"][j] == b["done"][j] and a["tid"][j] == b["tid"][j], ctx
                assert np.isnan(fin["rews"][k, j]) and np.isnan(fin["acts"][k, j]).all(), ctx
                st["frozen"] += 1
                continue
            _load(L, P, E, a["snap"], j, phase, seed, g, -1, tilt)
            if not wind:
                E.wind_on, E.wind_stoch = 0, 0
            act = fin["acts"][k, j]
            assert np.array_equal(act, b["acts"][k, j]), ctx            # every call records the same action
            if actor is not None:
                with torch.no_grad():
                    mean = actor(a["obs"][j:j + 1].cuda())[0][0].cpu().numpy()
                d = np.abs(np.tanh(mean) * actor.max_action - act)
                assert (d <= 2e-5 + 1e-4 * np.abs(mean)).all(), (ctx, d, mean)
                st["max_act"] = max(st["max_act"], float(d.max()))
            u = (C.c_double * 4)(*(list(act.astype(np.float64)) + [0.0] * (4 - len(act))))
            L.orc_step(C.byref(P), C.byref(E), phase, 0, u, 1, None, C.byref(o))
            so = np.array(E.s[:])
            st["max_err"] = np.maximum(st["max_err"], np.abs(b["snap"]["s"][j] - so) / np.maximum(np.abs(so), 1e-3))
            rew = float(fin["rews"][k, j])
            st["max_rew"] = max(st["max_rew"], abs(rew - o.reward))
            assert b["ret"][j] == a["ret"][j] + fin["rews"][k, j], ctx    # the return: rewards in step order
            fo = np.array([E.fu[0], E.fu[1], E.fv[0], E.fv[1]])
            st["max_filt"] = max(st["max_filt"], float(np.abs(b["snap"]["filt"][j] - fo).max()))
            assert int(b["snap"]["ts"][j]) == int(a["snap"]["ts"][j]) + 1 and int(b["steps"][j]) == k + 1, ctx
            assert int(b["snap"]["ep"][j]) == int(a["snap"]["ep"][j]), ctx   # never auto-reset
            assert int(b["snap"]["tid"][j]) == o.trunc_id and int(b["tid"][j]) == o.trunc_id, ctx
            ended = bool(o.done or o.trunc)
            assert (int(fin["steps"][j]) == k + 1) == ended, (ctx, int(fin["steps"][j]), ended)
            assert int(b["done"][j]) == (int(o.done) if ended else 0), ctx
            st["steps"] += 1
            if ended:
                assert int(fin["done"][j]) == int(o.done) and int(fin["tid"][j]) == o.trunc_id, ctx
                st["ended"] += 1
                st["done"] += int(o.done)
                st["trunc_ids"].add(o.trunc_id)
    return st


@pytest.mark.parametrize("phase,S,A,windy,K", [(PT, 2, 1, True, 40), (LB, 5, 4, False, 20)])
def test_rollout_shadowed_against_oracle(pd, oracle_mod, phase, S, A, windy, K):
    """The reference anchor: 37 envs (two full tiles and a ragged one of 5), 8 sampled envs with
    one of the ragged tile, every step of the first K teacher-forced against the oracle from the
    device's own snapshots, and the torch Actor against the recorded actions."""
    import torch
    from shadow import check_stats
    from pdenv.sac import ActorKernel
    N, seed = 37, 29
    tilt = WINDY["tilt_sigma_rad"] if windy else 0.0
    env = make(pd, N, phase, seed=seed, **(WINDY if windy else {}))
    actor = make_actor(S, A)
    idx = np.array([0, 5, 15, 16, 23, 31, 32, 36])
    recs = rollout_records(env, ActorKernel(actor), env.checkpoint(), K + 1, torch.as_tensor(idx, device=env.device),
                           reset=True)
    st = shadow_rollout(oracle_mod, recs, idx, 0 if phase == PT else 1, seed, tilt, windy, actor=actor)
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in st.items()})
    check_stats(st)
    assert st["steps"] + st["frozen"] == K * len(idx) and st["steps"] >= K * len(idx) // 2
    if windy:   # the tilt took: the sampled envs start from different pitch angles
        assert len({float(v) for v in recs[0]["snap"]["s"][:, 4]}) == len(idx)
    assert env.counters()["nan_events"] == 0


def zero_action_actor():
    """An actor whose action is exactly 0.0 whatever the MLP sums: mean head zeroed."""
    import torch
    actor = make_actor(2, 1)
    with torch.no_grad():
        actor.mean.weight.zero_()
        actor.mean.bias.zero_()
    return actor


def landing_setup(pd, N=48, **kw):
    """48 fresh pure-throttle envs, the first 8 moved to row 1279 of the recorded landing (y about
    1.01 m, vy about -1.41 m/s: one step of action 0 lands them) with a consistent g-load history
    (|v| of that row, an empty window).  Returns the handle and a checkpoint of this start."""
    import torch
    env = make(pd, N, PT, seed=41, **kw)
    env.reset()
    row = torch.tensor(golden("recorded_reference_trajectory.npz")["state"][1279], dtype=env.dtype, device=env.device)
    s = env.state
    s[:8] = row
    env.set_state(s)
    vp, ring, ln, _ = env.gload_window()
    vp[:8] = torch.sqrt(row[2] * row[2] + row[3] * row[3])
    ring[:8] = 0
    ln[:8] = 0
    env.set_gload_window(vp, ring, ln)
    return env, env.checkpoint()


def run_from(env, blob, kern, T, **kw):
    import torch
    env.restore(blob)
    acts, rews = traces(env, T)
    out = env.rollout_sac(kern, reset=False, max_steps=T, actions_out=acts, rewards_out=rews, **kw)
    return out + (acts, rews, env.state)


def test_mixed_lengths_landing_cap_and_chaining(pd, oracle_mod):
    """One tile with envs that land at their first step next to fresh ones (about 131 steps under
    action 0): the done path, per-env freezing, and then launch chaining (step_fuse 7 against 128),
    a capped call continued by a second one, and repeatability.  Expected values come from the
    oracle, teacher-forced on the device's snapshots and free-running for the fresh envs' length."""
    import torch
    from shadow import check_stats
    from pdenv.sac import ActorKernel
    N, T = 48, 512
    actor = zero_action_actor()
    kern = ActorKernel(actor)
    env, blob = landing_setup(pd, N)
    # -- the oracle on the device's snapshots: the landing step, the frozen envs, the fresh ones
    idx = np.array([0, 3, 7, 8, 15, 20, 47])
    recs = rollout_records(env, kern, blob, 5, torch.as_tensor(idx, device=env.device), reset=False)
    st = shadow_rollout(oracle_mod, recs, idx, 0, 41, 0.0, False, actor=actor)
    check_stats(st)
    assert st["done"] == 3 and st["ended"] == 3 and st["frozen"] == 3 * 3, st   # envs 0, 3, 7 land at step 0
    # -- the full rollout
    ret, steps, done, tid, acts, rews, state = run_from(env, blob, kern, T)
    assert int(done.sum()) >= 1 and bool((done[:8] == 1).all()) and bool((steps[:8] == 1).all())
    assert len(set(steps[:16].tolist())) >= 2, "one tile, mixed lengths"
    assert bool((acts[~torch.isnan(acts)] == 0).all())
    o = oracle_mod.Oracle(phase=oracle_mod.PURE_THROTTLE, rtd=oracle_mod.RTD_RL)
    for n_orc in range(1, T + 1):
        _, _, d, tr, id_orc, _, _ = o.step(np.zeros(1, dtype=np.float32), f32=True)
        if d or tr:
            break
    print("fresh envs:", sorted(set(steps[8:].tolist())), "oracle", n_orc, id_orc)
    assert bool(((steps[8:] - n_orc).abs() <= 1).all()) and bool((tid[8:] == id_orc).all()) and bool((done[8:] == 0).all())
    assert bool((steps < T).all())
    full = (ret, steps, done, tid, acts, rews, state)
    # -- step_fuse invariance: launches of 7 steps against 128
    assert env.tuning()["step_fuse"] == 128
    env.set_tuning(step_fuse=7)
    for name, x, y in zip("ret steps done tid acts rews state".split(), run_from(env, blob, kern, T), full):
        assert torch.equal(bits(x), bits(y)), f"step_fuse 7: {name}"
    env.set_tuning(step_fuse=128)
    # -- a capped call, then its continuation
    r1, s1, d1, t1, a1, w1, _ = run_from(env, blob, kern, 50)
    assert bool((s1[8:] == 50).all()) and bool((d1[8:] == 0).all()) and bool((s1[:8] == 1).all())
    a2, w2 = traces(env, T)
    r2, s2, d2, t2 = env.rollout_sac(kern, reset=False, max_steps=T, actions_out=a2, rewards_out=w2)
    assert torch.equal((s1 + s2)[8:], steps[8:]) and torch.equal(t2[8:], tid[8:]) and torch.equal(d2[8:], done[8:])
    assert torch.equal(bits(torch.cat([w1, w2])[:T, 8:]), bits(rews[:, 8:])), "concatenated reward traces"
    assert torch.equal(bits(torch.cat([a1, a2])[:T, 8:]), bits(acts[:, 8:]))
    assert torch.equal(bits(env.state[8:]), bits(state[8:])), "final state after the continued call"
    # -- repeat: reset=True twice gives identical outputs
    env.restore(blob)
    reps = []
    for _ in range(2):
        a3, w3 = traces(env, T)
        reps.append(env.rollout_sac(kern, reset=True, max_steps=T, actions_out=a3, rewards_out=w3) + (a3, w3))
    for x, y in zip(*reps):
        assert torch.equal(bits(x), bits(y))
    assert bool((reps[0][1] == steps[8]).all()), "after a reset every env is a fresh one"
    assert env.counters()["nan_events"] == 0


def test_refusals_and_per_step_fallback(pd):
    """pd_rollout_sac refuses a handle that does not step 16 lanes per env and a hidden-512 actor
    (PD_ERR_UNSUPPORTED, the cause in pd_last_error, nothing launched); evaluate_agent then runs
    the per-step path; on a supported handle both of its paths give the same bits."""
    import torch
    from pdenv import _lib as L
    from pdenv.sac import ActorKernel, evaluate_agent
    N, T = 37, 512
    small, wide = make_actor(2, 1), make_actor(2, 1, H=512)
    for env, actor, cause in ((make(pd, N, lanes_per_env=2, seed=5), small, b"16 lanes per env"),
                              (make(pd, N, seed=5), wide, b"512")):
        k = ActorKernel(actor)
        before = [x.clone() for x in env.episode_counters()]
        st = env.lib.pd_rollout_sac(env.h, k.S, k.A, k.H, k.nl, k.ptrs(), 1, -20.0, 2.0, 1.0, 1, T, None, None, None,
                                    None, None, None, None)
        assert st == L.PD_ERR_UNSUPPORTED and cause in env.lib.pd_last_error(), env.lib.pd_last_error()
        with pytest.raises(L.PdError):
            env.rollout_sac(k, max_steps=T)
        assert all(torch.equal(x, y) for x, y in zip(before, env.episode_counters())), "nothing was launched"
        res = evaluate_agent(actor, env, max_steps=T)
        assert not res.fused
        assert bool((res.steps > 0).all()) and bool((res.steps < T).all()) and sum(res.trunc_hist.values()) == N
    a, b = make(pd, N, seed=9), make(pd, N, seed=9)
    fused = evaluate_agent(small, a, max_steps=T, deterministic=False, fused=True, traces=True)
    plain = evaluate_agent(small, b, max_steps=T, deterministic=False, fused=False, traces=True)
    assert fused.fused and not plain.fused
    assert fused[:2] == plain[:2] and fused.trunc_hist == plain.trunc_hist
    for name in ("returns", "steps", "done", "trunc_id", "actions", "rewards"):
        x, y = getattr(fused, name), getattr(plain, name)
        assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), name


def test_evaluate_agent_facade(pd):
    """eval_reward, success_rate = evaluate_agent(...)[:2] reads like the driver: the mean of the
    returns and the share of episodes whose terminal step had done; the trunc_id histogram covers
    every episode.  (The sums run in binary64 on the host in another order than numpy's: 1e-12.)"""
    from pdenv.sac import evaluate_agent
    actor = zero_action_actor()
    env = make(pd, 37, seed=2)
    res = evaluate_agent(actor, env, max_steps=512)
    eval_reward, success_rate = res[:2]
    assert res.fused and res.actions is None and res.rewards is None
    r = res.returns.cpu().numpy().astype(np.float64)
    assert math.isclose(eval_reward, r.mean(), rel_tol=1e-12) and eval_reward == res.mean_reward
    assert success_rate == float((res.done.cpu().numpy() != 0).mean()) == res.success_rate
    assert sum(res.trunc_hist.values()) == 37
    assert res.trunc_hist == {int(k): int(v) for k, v in zip(*np.unique(res.trunc_id.cpu().numpy(), return_counts=True))}
