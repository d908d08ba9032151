"""CPU anchors of the SAC TD-target tests: the binary64 NumPy model the GPU tests compare the
kernels with (tests/sac_td_nets.py) agrees with torch's own float64 evaluation of Actor.sample,
Critic and the four lines of SACPyTorch.update's no_grad block (sac_pytorch.py:439-443) on the same
eps; Critic takes the reference's state dict; the integer critic cases meet their conditions; the
torch restatement of the kernel's eps draws agrees with the NumPy one."""
import copy

import numpy as np
import pytest

import sac_nets as sn
import sac_td_nets as td


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_model_agrees_with_torch_float64(S, A, H, L):
    import torch
    case = td.td_case(S, A, H, L, n=64)
    actor, critic = copy.deepcopy(case["actor"]).double(), copy.deepcopy(case["critic"]).double()
    rows = torch.from_numpy(case["rows"]).double()
    ns = rows[:, S + A + 1:2 * S + A + 1]
    # Actor.sample draws eps = torch.randn(mean.shape, generator): the same generator state gives it here
    g = torch.Generator().manual_seed(5)
    eps = torch.randn((64, A), dtype=torch.float64, generator=g)
    g.manual_seed(5)
    with torch.no_grad():
        next_actions, next_log_probs = actor.sample(ns, generator=g)
        q1, q2 = critic(ns, next_actions)
        alpha = case["log_alpha"].double().exp()
        next_q = torch.min(q1, q2) - alpha * next_log_probs
        gamma = float(np.float32(case["gamma"]))
        target_q = rows[:, S + A:S + A + 1] + (1 - rows[:, -1:]) * gamma * next_q
    c, heads, q = td.full(case, eps=eps.numpy())
    # (torch's constants are binary64 here, the model's the float32 constants of the f32 expression:
    # log(sqrt(2 pi)) and 1e-6 differ by 3e-8 and 2e-14, times A = 4 at most)
    np.testing.assert_allclose(c["next_actions"], next_actions.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(q, torch.cat([q1, q2], dim=1).numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(c["next_log_prob"], next_log_probs.numpy()[:, 0], rtol=0, atol=4 * 4e-8)
    np.testing.assert_allclose(c["target_q"], target_q.numpy()[:, 0], rtol=0, atol=4 * 4e-8)
    # the written-out block of the GPU tests is the same computation
    t2, a2, lp2, _, _ = td.torch_block(actor, critic, rows, eps, case["log_alpha"].double(), gamma, S, A)
    assert torch.equal(a2, next_actions)
    np.testing.assert_allclose(lp2.numpy(), next_log_probs.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(t2.numpy(), target_q.numpy(), rtol=0, atol=1e-12)
    # done rows: the reward's bits
    done = case["rows"][:, -1] == 1
    assert done.sum() >= 5 and (~done).sum() >= 5
    assert np.array_equal(c["target_q"][done], case["rows"][done, S + A].astype(np.float64))


def test_chain_bound_is_positive_and_small():
    """The a-priori bound is a few ulp for well-conditioned rows, finite everywhere."""
    case = td.td_case(2, 1, 256, 2, n=64)
    c, _, _ = td.full(case)
    for b, v in zip(td.chain_bound(c), (c["next_actions"], c["next_log_prob"], c["target_q"])):
        assert b.shape == v.shape and np.isfinite(b).all() and (b > 0).all()


def test_critic_loads_reference_state_dict():
    """The reference's Critic registers q1 / q2 nn.Sequential members (sac_pytorch.py:181-213): its
    state dict has the keys q1.<2 l>.weight / .bias; one with those names loads, strictly."""
    import torch
    from pdenv.sac import Critic
    S, A, H, L = 5, 4, 128, 3
    keys = [f"q{n}.{2 * l}.{w}" for n in (1, 2) for l in range(L + 1) for w in ("weight", "bias")]
    critic = Critic(S, A, hidden_dim=H, n_hidden_layers=L)
    assert list(critic.state_dict().keys()) == keys
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.rand(v.shape, generator=g) for k, v in critic.state_dict().items()}
    assert sd["q1.0.weight"].shape == (H, S + A) and sd[f"q2.{2 * L}.weight"].shape == (1, H)
    critic.load_state_dict(sd, strict=True)
    s, a = torch.rand(3, S, generator=g), torch.rand(3, A, generator=g)
    q1, q2 = critic(s, a)
    assert q1.shape == (3, 1) and q2.shape == (3, 1)
    p1, p2 = td.critic_params(critic)
    x = torch.cat([s, a], dim=1).numpy()
    np.testing.assert_allclose(td.q_forward(p1, x, dtype=np.float64)[0], q1.detach().numpy()[:, 0], rtol=1e-5)
    np.testing.assert_allclose(td.q_forward(p2, x, dtype=np.float64)[0], q2.detach().numpy()[:, 0], rtol=1e-5)


@pytest.mark.parametrize("S,A,H,L", td.SHAPES)
def test_integer_critic_cases_meet_their_conditions(S, A, H, L):
    p1, p2, states, actions, ref = td.int_critic_case(S, A, H, L)
    assert states.shape == (sn.N_EXACT, S) and actions.shape == (sn.N_EXACT, A) and ref.shape == (sn.N_EXACT, 2)
    assert len(p1) == len(p2) == 2 * (L + 1) and p1[-2].shape == (1, H)


def test_torch_eps_restatement_agrees_with_numpy():
    """pdenv.sac.td_eps (the fallback's eps source) against td.np_eps: the same Philox blocks, so the
    binary64 normals agree to a few ulp and the float32 casts to one float32 ulp."""
    import torch
    from pdenv.sac import td_eps
    seed, draw = 0x123456789ABCDEF, (7 << 32) | 3
    for A in (1, 4, 7):
        got = td_eps(seed, draw, 33, A, torch.device("cpu")).numpy()
        ref = td.np_eps(seed, draw, 33, A)
        assert got.shape == (33, A) and got.dtype == np.float32
        assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
