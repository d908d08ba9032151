"""CPU checks of the fused SAC collection's surface (pd_collect_sac, SACCollector.collect): the
additive export (ABI still 11), its argument checks before any launch, and the step-major order in
which several ranks' collection slabs are appended."""
import ctypes as C


def test_pd_collect_sac_is_an_additive_export():
    import pdenv
    from pdenv import _lib
    L = pdenv.load()
    assert hasattr(L, "pd_collect_sac") and "pd_collect_sac" in _lib.EXPORTS
    assert L.pd_abi_version() == _lib.ABI_VERSION == 11


def test_null_handle_is_refused_before_any_launch():
    import pdenv
    from pdenv import _lib
    L = pdenv.load()
    vp = C.c_void_p
    params = (vp * 8)(*([0x10000] * 8))          # (never dereferenced)
    st = L.pd_collect_sac(None, 2, 1, 256, 2, params, 0, -20.0, 2.0, 1.0, 4, vp(0x10000), 1 << 20, vp(0x10000),
                          vp(0x10000), vp(0x10000), vp(0x10000), None, None, None, None, None, None)
    assert st == _lib.PD_ERR_INVALID and b"pd_collect_sac" in L.pd_last_error()
    try:
        _lib.check(st)
    except _lib.PdError as err:
        assert err.status == _lib.PD_ERR_INVALID
    else:
        raise AssertionError("check() did not raise")


def test_step_major_equals_per_step_gathers():
    """World 3, k 4, N 5: the all-gathered per-rank [k, N, W] slabs, reordered, are the rows that k
    per-step gathers (every rank's [N, W] slab of the step, in rank order) append one after
    another."""
    import torch
    from pdenv.sac import step_major
    world, k, n, w = 3, 4, 5, 7
    slabs = [torch.arange(k * n * w, dtype=torch.float32).reshape(k, n, w) + 1000.0 * r for r in range(world)]
    gathered = torch.stack(slabs)                               # what all_gather_into_tensor leaves
    want = torch.cat([torch.cat([slabs[r][t] for r in range(world)]) for t in range(k)])
    got = step_major(gathered)
    assert got.shape == (k * world * n, w) and torch.equal(got, want)
    assert not torch.equal(gathered.reshape(-1, w), want), "rank-major order is another order"
