"""CPU checks of the inputs of tests/test_gpu_sac_actor.py: the integer nets of sac_nets.py are
exact in binary32 (no GPU involved), over the whole list of shapes the GPU test runs."""
import numpy as np
import pytest

import sac_nets as sn


@pytest.mark.parametrize("S,A,H,L", sn.SHAPES)
def test_integer_net_is_exact_in_f32_on_the_cpu(S, A, H, L):
    """The conditions on the inputs hold (every partial sum below 2**24, a live share in
    [0.2, 0.8] after the last hidden layer, at least 8 distinct head values: int_case asserts
    them), and torch's float32 forward on the CPU through pdenv.sac.Actor, an independent
    summation order, equals the int64 reference exactly."""
    import torch
    from pdenv.sac import Actor
    params, obs, ref = sn.int_case(S, A, H, L)
    assert len(params) == 2 * (L + 2) and all(p.dtype == np.float32 for p in params)
    assert params[0].shape == (H, S) and params[2 * L].shape == (A, H) and obs.shape == (sn.N_EXACT, S)
    for p in params + [obs]:
        assert np.array_equal(p, np.rint(p))
    if L > 3:
        assert all((params[2 * l] != 0).sum(1).tolist() == [4] * H for l in range(1, L))
    actor = sn.load_actor(Actor(S, A, hidden_dim=H, n_hidden_layers=L), params)
    with torch.no_grad():
        f = actor.shared_net(torch.from_numpy(obs))
        got = torch.cat([actor.mean(f), actor.log_std(f)], dim=1)
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.from_numpy(ref))
    # the prefixes the batch-size cases use are the same rows
    ref5, _, _ = sn.forward(params, obs[:5])
    assert np.array_equal(ref5.astype(np.float32), ref[:5])
