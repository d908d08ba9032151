"""The 512-thread step kernels: binary64, pure throttle, wind, two lanes per env
-- the c3 kernel and its counting instantiation -- with one workgroup per CU, the coarse atmosphere
table and the wind profiles' slopes in LDS.

Sizes: N = 257 (a full 256-env workgroup and one env more: a second workgroup with 510 lanes past
the end) and N = 600 (a partial last workgroup); T = 24 steps of test_gpu_c3.py's 3:1 action mix;
wind with a percentile drawn per reset, gusts, tilt, auto-reset, lanes_per_env = 2.

  1. parity: every env teacher-forced against the oracle at every step (tests/shadow.py) at
     test_gpu_c3.py's tolerances, flags and auto-resets exact;
  2. pd_step_n at 7 and at 16 fused steps against a pd_step loop: equal bits in every output, in
     the final state and in the checkpoint;
  3. with PD_TABLES_NO_ATM_LDS (no coarse table: the closed form) every output and the final
     checkpoint equal, bit for bit, what the parent commit's library gave for the same seed and
     actions (tests/golden/wg512_parent_n600.npz, N = 600): the workgroup size and the tabulated
     wind slopes change no bit.  The fixture holds the rewards, flags, truncation ids, the last
     observation and the final state in full, and SHA-256 digests of each step's observations and
     of the final checkpoint's buffers (the full arrays would be 0.5 MB).
"""
import hashlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, SEED, ASEED = 24, 1234, 7


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def wg_env(pd, n, **kw):
    args = dict(flight_phase="landing_burn_pure_throttle", mode="rl", enable_wind=True, stochastic_wind=True,
                wind_percentile=None, auto_reset=True, tilt_sigma_rad=math.radians(1.0), seed=SEED, lanes_per_env=2)
    args.update(kw)
    return pd.PoweredDescentEnv(n, **args)


def wg_actions(n):
    """test_gpu_c3.py's mix: U(-1, 1) on every 4th env, U(0.5, 1) elsewhere."""
    import torch
    g = torch.Generator().manual_seed(ASEED)
    u = torch.rand(T, n, 1, generator=g)
    hi = torch.arange(n) % 4 != 0
    return torch.where(hi.view(1, n, 1), 0.5 + 0.5 * u, 2 * u - 1).contiguous()


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def ckpt_fields(env):
    """The checkpoint blob's per-env buffers (pd_checkpoint_save: each 16-byte aligned in the blob)
    without the alignment padding between them, which no call writes: N here is no multiple of 16."""
    blob, n = env.checkpoint(), env.n
    sizes = [11 * n * 8, n * 8, 10 * n * 8, 3 * n * 8, 6 * n * 8, n, n, n, 2 * n * 8, 2 * n * 4, n, n * 4, n * 4, n]
    assert sum((b + 15) & ~15 for b in sizes) == blob.numel()
    out, off = [], 0
    for b in sizes:
        out.append(blob[off:off + b])
        off += (b + 15) & ~15
    import torch
    return torch.cat(out)


def trace(pd, n, table_flags):
    """What case 3 compares (and what recorded the fixture, from the parent commit's library with
    table_flags 0): one pd_step_n call over the T steps."""
    env = wg_env(pd, n, table_flags=table_flags)
    obs, rew, dn, tr, tid = env.step_n(wg_actions(n).cuda())
    return dict(rew=rew.cpu().numpy(), done=dn.cpu().numpy(), trunc=tr.cpu().numpy(), tid=tid.cpu().numpy(),
                obs_last=obs[-1].cpu().numpy(), obs_sha=np.array([_sha(obs[t]) for t in range(T)]),
                state=env.state.cpu().numpy(), ckpt_sha=np.array(_sha(ckpt_fields(env))))


@pytest.mark.parametrize("n", [257, 600])
def test_wg512_shadowed(pd, oracle_mod, n):
    from shadow import shadow_run, check_stats
    env = wg_env(pd, n)
    st = shadow_run(oracle_mod, env, wg_actions(n).cuda(), np.arange(n), 0, 0, SEED, math.radians(1.0))
    print("wg512 shadow:", n, dict(max_err=st["max_err"].tolist(), rew=st["max_rew"], obs=st["max_obs"],
                                   filt=st["max_filt"], resets=st["resets"], gust_steps=st["gust_steps"]))
    check_stats(st)
    assert st["steps"] == n * T
    assert env.counters()["nan_events"] == 0


@pytest.mark.parametrize("n", [257, 600])
def test_wg512_fused_equals_per_step(pd, n):
    import torch
    A = wg_actions(n).cuda()
    ref = wg_env(pd, n)
    outs = [ref.step(A[t]) for t in range(T)]
    r_obs, r_rew = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    r_dn, r_tr = torch.stack([o[2] for o in outs]), torch.stack([o[3] for o in outs])
    r_tid = torch.stack([o[4]["trunc_id"] for o in outs])
    for fuse in (7, 16):
        env = wg_env(pd, n)
        env.set_tuning(step_fuse=fuse)
        obs, rew, dn, tr, tid = env.step_n(A)
        assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew), fuse
        assert torch.equal(dn, r_dn) and torch.equal(tr, r_tr) and torch.equal(tid, r_tid), fuse
        assert torch.equal(env.state, ref.state), fuse
        assert torch.equal(ckpt_fields(env), ckpt_fields(ref)), fuse


def test_wg512_no_table_keeps_parent_bits(pd):
    from conftest import golden
    from pdenv import _lib as L
    want = golden("wg512_parent_n600.npz")
    got = trace(pd, 600, L.TABLES_NO_ATM_LDS)
    assert set(got) == set(want.files)
    for k in sorted(got):
        assert np.array_equal(got[k], want[k]), k
