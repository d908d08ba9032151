"""Pacing of the two waves of a SIMD in the 512-thread step kernels (PD_PACE): the
waves change their issue priority by their progress against their SIMD partner's, which may move
no bit of any result.  Every case compares a default handle with one created with
PD_TABLES_NO_PACE (every wave stays at priority 0), on test_gpu_wg512.py's handle, action mix and
T = 24 steps.

Sizes: N = 257 (a full workgroup of four paced pairs per SIMD set, and a second workgroup with one
live env: its other waves only run private copies past the end) and N = 600 (a partial last
workgroup: waves with lanes past the end and waves with no live env at all, whose partners must
not stay raised).

  1. pd_step_n over the 24 steps at once, at 7 fused steps, and a pd_step loop: every output, the
     final state and the checkpoint equal in bits with pacing on and off;
  2. the miss solve under pacing: tables cut to 4 keys (payload sums only, as
     test_gpu_parity.py::test_device_solve_bit_identical), N = 600: the waves take the miss solve
     and its lock with pacing on, the results equal the PD_TABLES_NO_PACE handle's in bits, and the
     solved-miss counter is above zero.
"""
import pytest

from test_gpu_wg512 import T, ckpt_fields, wg_actions, wg_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def run(env, A, how):
    """The T steps by `how`: 0 one pd_step_n launch, k > 0 launches of k fused steps, -1 a pd_step loop."""
    import torch
    if how < 0:
        outs = [env.step(A[t]) for t in range(T)]
        res = (torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs]),
               torch.stack([o[3] for o in outs]), torch.stack([o[4]["trunc_id"] for o in outs]))
    else:
        env.set_tuning(step_fuse=how if how else T)
        res = env.step_n(A)
    return tuple(r.clone() for r in res) + (env.state.clone(), ckpt_fields(env))


NAMES = ("obs", "reward", "done", "trunc", "trunc_id", "state", "checkpoint")


@pytest.mark.parametrize("how", [0, 7, -1], ids=["step_n_24", "fused_7", "step_loop"])
@pytest.mark.parametrize("n", [257, 600])
def test_pace_changes_no_bit(pd, n, how):
    import torch
    from pdenv import _lib as L
    A = wg_actions(n).cuda()
    on = run(wg_env(pd, n), A, how)
    off = run(wg_env(pd, n, table_flags=L.TABLES_NO_PACE), A, how)
    for name, a, b in zip(NAMES, on, off):
        assert torch.equal(a, b), name


def test_pace_miss_solve_completes(pd):
    import torch
    from pdenv import _lib as L
    n = 600
    A = wg_actions(n).cuda()
    kw = dict(params=pd.Params().restrict_keys(4, 4))
    e_on = wg_env(pd, n, table_flags=L.TABLES_NO_CELL_PIECES, **kw)
    e_off = wg_env(pd, n, table_flags=L.TABLES_NO_CELL_PIECES | L.TABLES_NO_PACE, **kw)
    on, off = run(e_on, A, 0), run(e_off, A, 0)
    for name, a, b in zip(NAMES, on, off):
        assert torch.equal(a, b), name
    m_on, m_off = e_on.counters()["rbf_misses"], e_off.counters()["rbf_misses"]
    print("pace miss solve: solved misses", m_on, "(paced)", m_off, "(PD_TABLES_NO_PACE)")
    assert m_on > 0 and m_off > 0
