"""CPU checks of the SAC evaluation rollout's surface: the additive export (ABI still 11), its
argument checks before any launch, and the summary arithmetic of evaluate_agent."""
import ctypes as C


def test_pd_rollout_sac_is_an_additive_export():
    import pdenv
    from pdenv import _lib
    L = pdenv.load()
    assert hasattr(L, "pd_rollout_sac") and "pd_rollout_sac" in _lib.EXPORTS
    assert L.pd_abi_version() == _lib.ABI_VERSION == 11


def test_null_handle_is_refused_before_any_launch():
    import pdenv
    from pdenv import _lib
    L = pdenv.load()
    vp = C.c_void_p
    params = (vp * 8)(*([0x10000] * 8))          # (never dereferenced)
    st = L.pd_rollout_sac(None, 2, 1, 256, 2, params, 1, -20.0, 2.0, 1.0, 1, 100, None, None, None, None, None, None,
                          None)
    assert st == _lib.PD_ERR_INVALID and b"pd_rollout_sac" in L.pd_last_error()
    # the status reaches Python callers that fall back on PD_ERR_UNSUPPORTED only
    try:
        _lib.check(st)
    except _lib.PdError as err:
        assert err.status == _lib.PD_ERR_INVALID
    else:
        raise AssertionError("check() did not raise")


def test_summary_on_cpu_tensors():
    """mean of the returns, share of episodes whose terminal step had done, {trunc_id: count}; an
    episode with done AND a truncation id counts as a success (the driver counts `done`) and in
    its id's bin."""
    import torch
    from pdenv.sac import EvalResult, summarize_rollout
    returns = torch.tensor([1.5, -2.0, 4.0, 0.5, 8.0], dtype=torch.float64)
    done = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8)
    tid = torch.tensor([0, 4, 7, 4, 0], dtype=torch.int8)     # env 2: done and truncated (id 7)
    mean, rate, hist = summarize_rollout(returns, done, tid)
    assert mean == 12.0 / 5 and rate == 2 / 5
    assert hist == {0: 2, 4: 2, 7: 1} and sum(hist.values()) == 5
    mean32, _, _ = summarize_rollout(returns.float(), done.bool(), tid)
    assert mean32 == mean
    res = EvalResult(mean, rate, returns, torch.ones(5, dtype=torch.int32), done, tid, hist)
    eval_reward, success_rate = res[:2]
    assert (eval_reward, success_rate) == (mean, rate) == (res.mean_reward, res.success_rate)
    assert res.trunc_hist is hist and res.actions is None and res.rewards is None and res.returns is returns
