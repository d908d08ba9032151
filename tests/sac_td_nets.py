"""Inputs and NumPy models for the tests of pd_sac_critic and pd_sac_td_target (plain NumPy; no
GPU, no torch at import).  Builds on sac_nets.py: a Q net is an actor net with S + A inputs and
one output whose mean head is kept as the Q head.

The binary64 model of the update's no_grad block (sac_pytorch.py:439-443) is `chain` (steps 3, 4
and 6 of pd_sac_td_target's contract: sampling, log-probability, backup, from given heads, eps and
twin Q) and `full` (the nets as well).  `chain_bound` is the a-priori float32 error bound of the
chain, evaluated on the model's own values."""
import numpy as np

import sac_nets as sn

# (S, A, H, L) of the critic's exact tests; also the shapes of the TD-target tests
SHAPES = [
    (2, 1, 256, 2),     # the driver's default
    (8, 2, 128, 1),     # no hidden layer
    (5, 4, 256, 3),
    (12, 4, 512, 2),    # the S + A = 16 corner
    (1, 1, 128, 8),     # L = 8
]
SHAPES_N = [(8, 2, 128, 1), (2, 1, 256, 2), (12, 4, 512, 2)]     # one per H, for the batch sizes
LOG_STD_MIN, LOG_STD_MAX = -5.0, -1.0
LOG_SQRT_2PI = float(np.float32(0.9189385332046727))   # the float32 constant of the f32 expression
TANH_EPS = float(np.float32(1e-6))
EPS32 = 2.0 ** -24                                      # the relative error of one float32 rounding


def q_params(S, A, H, L, seed):
    """An integer Q net in pd_sac_critic's order -- W1 [H][S + A], b1, (W [H][H], b) x (L - 1),
    W [1][H], b [1] -- from sn.int_actor(S + A, 1, H, L, seed) without its log_std head."""
    return sn.int_actor(S + A, 1, H, L, seed)[:2 * (L + 1)]


def q_forward(params, x, dtype=np.int64):
    """(q [n], abs_sum, live) of one Q net: sn.forward on the net with its output head doubled."""
    ps = list(params) + list(params[-2:])
    out, abs_sum, live = sn.forward(ps, x, dtype=dtype)
    return out[:, 0], abs_sum, live


def int_critic_case(S, A, H, L, n=sn.N_EXACT):
    """(params_q1, params_q2, states [n][S], actions [n][A], q [n][2] float32) of an integer twin
    critic (seeds 0 and 1), with sn.int_case's conditions asserted on each net: every partial sum
    below 2**24, a live share in [0.2, 0.8], at least 8 distinct outputs; and Q1 != Q2 somewhere."""
    sa = sn.int_obs(n, S + A)
    cols, ps = [], []
    for seed in (0, 1):
        p = q_params(S, A, H, L, seed)
        q, abs_sum, live = q_forward(p, sa)
        assert abs_sum < sn.EXACT_LIMIT, (abs_sum, sn.EXACT_LIMIT)
        assert 0.2 <= live <= 0.8, live
        assert len(np.unique(q)) >= 8, np.unique(q)
        assert np.array_equal(q.astype(np.float32).astype(np.int64), q)
        cols.append(q)
        ps.append(p)
    ref = np.stack(cols, axis=1).astype(np.float32)
    assert (ref[:, 0] != ref[:, 1]).any()
    return ps[0], ps[1], np.ascontiguousarray(sa[:, :S]), np.ascontiguousarray(sa[:, S:]), ref


def q_linears(net):
    import torch.nn as nn
    return [m for m in net if isinstance(m, nn.Linear)]


def load_critic(critic, p1, p2):
    """Copy two parameter lists (pd_sac_critic's order) into a pdenv.sac.Critic, in place."""
    import torch
    with torch.no_grad():
        for net, params in ((critic.q1, p1), (critic.q2, p2)):
            lins = q_linears(net)
            assert len(params) == 2 * len(lins)
            for k, m in enumerate(lins):
                for t, p in ((m.weight, params[2 * k]), (m.bias, params[2 * k + 1])):
                    assert tuple(t.shape) == p.shape, (k, tuple(t.shape), p.shape)
                    t.copy_(torch.from_numpy(np.asarray(p)))
    return critic


def critic_params(critic):
    """(params_q1, params_q2) of a Critic as float32 NumPy arrays, pd_sac_critic's order."""
    return tuple([t.detach().cpu().numpy() for m in q_linears(net) for t in (m.weight, m.bias)]
                 for net in (critic.q1, critic.q2))


def real_critic(S, A, H, L, seed=0, gain=sn.REAL_GAIN):
    """A Critic on the CPU with sn.real_case's init: every weight matrix U(-1, 1) / sqrt(fan_in)
    times gain, biases U(-0.5, 0.5)."""
    import torch
    from pdenv.sac import Critic
    g = torch.Generator().manual_seed(7000 + 1000 * seed + 97 * S + 13 * A + H + L)
    critic = Critic(S, A, hidden_dim=H, n_hidden_layers=L)
    with torch.no_grad():
        for name, p in critic.named_parameters():
            if name.endswith("weight"):
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (gain / np.sqrt(p.shape[1])))
            else:
                p.copy_(torch.rand(p.shape, generator=g) - 0.5)
    return critic


def td_case(S, A, H, L, n=sn.N_REAL, log_alpha=-1.0, gamma=0.99):
    """The real-valued case of a shape: dict with the actor (sn.real_case seed 0, log_std clamp
    (-5, -1), max_action 1) and the critic on the CPU, rows [n][W] float32 (state, action and reward
    random, next_state the case's observations, done = 1 on every fifth row), a fixed eps [n][A],
    log_alpha and gamma."""
    import torch
    actor, obs, _, _ = sn.real_case(S, A, H, L, n=n)
    actor.log_std_min, actor.log_std_max = LOG_STD_MIN, LOG_STD_MAX
    rng = np.random.default_rng([S, A, H, L, 11])
    rows = np.empty((n, 2 * S + A + 2), dtype=np.float32)
    rows[:, :S] = rng.uniform(-2, 2, (n, S))
    rows[:, S:S + A] = rng.uniform(-1, 1, (n, A))
    rows[:, S + A] = rng.uniform(-2, 2, n)
    rows[:, S + A + 1:2 * S + A + 1] = obs.numpy()
    rows[:, -1] = (np.arange(n) % 5 == 3)
    eps = rng.standard_normal((n, A)).astype(np.float32)
    return dict(S=S, A=A, H=H, L=L, n=n, actor=actor, critic=real_critic(S, A, H, L), rows=rows, eps=eps,
                log_alpha=torch.full((1,), log_alpha, dtype=torch.float32), gamma=gamma)


def chain(heads, eps, q, rows, S, A, lo, hi, max_action, log_alpha, gamma):
    """Steps 3, 4 and 6 in binary64 from float32 inputs: dict of next_actions [n][A], next_log_prob
    [n], target_q [n] and the intermediate values chain_bound reads.  log_alpha and gamma enter as the
    float32 numbers the kernel receives, the constants as the float32 constants of the expression."""
    heads, eps, q, rows = (np.asarray(x, dtype=np.float64) for x in (heads, eps, q, rows))
    m = heads[:, :A]
    ls = np.clip(heads[:, A:], float(np.float32(lo)), float(np.float32(hi)))
    sd = np.exp(ls)
    p = sd * eps
    x = m + p
    a = np.tanh(x)
    d = x - m
    t1 = d * d / (2 * sd * sd)
    w = 1 - a * a + TANH_EPS
    lg = np.log(w)
    lpk = -t1 - ls - LOG_SQRT_2PI - lg
    lp = lpk.sum(axis=1)
    alpha = np.exp(float(np.float32(log_alpha)))
    nq = np.minimum(q[:, 0], q[:, 1]) - alpha * lp
    r, done = rows[:, S + A], rows[:, -1]
    f = (1 - done) * float(np.float32(gamma))
    return dict(next_actions=a * float(np.float32(max_action)), next_log_prob=lp, target_q=r + f * nq, m=m, ls=ls,
                sd=sd, eps=eps, p=p, x=x, a=a, d=d, t1=t1, w=w, lg=lg, lpk=lpk, alpha=alpha, nq=nq, f=f, r=r, done=done,
                gamma=float(np.float32(gamma)), max_action=float(np.float32(max_action)))


# ulp errors of the device library's expf, logf and tanhf: the OpenCL full-profile bounds its math
# library (OCML) is built to (exp <= 3, log <= 3, tanh <= 5 ulp); an error of k ulp is at most
# 2 k EPS32 relative
ULP_EXP, ULP_LOG, ULP_TANH = 3, 3, 5
SECOND_ORDER = 1.01          # the first-order terms below, plus 1 % for the products of errors


def chain_bound(c):
    """Absolute float32 error bounds (next_actions [n][A], next_log_prob [n], target_q [n]) of the
    chain on the model's values c = chain(...): see tests/test_gpu_sac_td.py, test 3."""
    e = EPS32
    ab = np.abs
    E_sd = 2 * ULP_EXP * e * c["sd"]
    E_p = ab(c["eps"]) * E_sd + e * ab(c["p"])
    E_x = E_p + e * ab(c["x"])
    E_a = (1 - c["a"] ** 2) * E_x + 2 * ULP_TANH * e * ab(c["a"])
    E_act = c["max_action"] * E_a + e * ab(c["a"] * c["max_action"])
    E_d = E_x + e * ab(c["d"])
    d2, s2 = c["d"] ** 2, c["sd"] ** 2
    E_d2 = 2 * ab(c["d"]) * E_d + e * d2
    E_den = 2 * (2 * c["sd"] * E_sd + e * s2)
    den = 2 * s2
    E_t1 = E_d2 / den + d2 * E_den / den ** 2 + e * c["t1"]
    g = c["a"] ** 2
    E_g = 2 * ab(c["a"]) * E_a + e * g
    E_h = E_g + e * ab(1 - g)
    E_w = E_h + e * c["w"]
    E_lg = E_w / c["w"] + 2 * ULP_LOG * e * ab(c["lg"])     # the amplification 1 / (1 - a^2 + 1e-6)
    s1 = -c["t1"] - c["ls"]
    s2_ = s1 - LOG_SQRT_2PI
    E_lpk = E_t1 + E_lg + e * (ab(s1) + ab(s2_) + ab(c["lpk"]))
    partial = np.cumsum(c["lpk"], axis=1)
    E_lp = E_lpk.sum(axis=1) + e * ab(partial[:, 1:]).sum(axis=1)
    lp = c["lpk"].sum(axis=1)
    E_alpha = 2 * ULP_EXP * e * c["alpha"]
    prod = c["alpha"] * lp
    E_prod = ab(lp) * E_alpha + c["alpha"] * E_lp + e * ab(prod)
    E_nq = E_prod + e * ab(c["nq"])
    E_f = e * ab(c["f"]) + e * ab(1 - c["done"]) * c["gamma"]
    fn = c["f"] * c["nq"]
    E_tq = ab(c["nq"]) * E_f + ab(c["f"]) * E_nq + e * ab(fn) + e * ab(c["r"] + fn)
    return SECOND_ORDER * E_act, SECOND_ORDER * E_lp, SECOND_ORDER * E_tq


def full(case, eps=None, log_alpha=None, actor_params=None, critic_params_=None):
    """The whole block in binary64 on the case's float32 parameters: (chain dict, heads [n][2A], q
    [n][2]), the critics on the model's own binary64 next_actions."""
    S, A = case["S"], case["A"]
    rows = case["rows"].astype(np.float64)
    ns = rows[:, S + A + 1:2 * S + A + 1]
    heads, _, _ = sn.forward(actor_params or sn.actor_params(case["actor"]), ns, dtype=np.float64)
    eps = case["eps"] if eps is None else eps
    la = float(case["log_alpha"][0]) if log_alpha is None else log_alpha
    actor = case["actor"]
    zero_q = np.zeros((rows.shape[0], 2))
    c = chain(heads, eps, zero_q, rows, S, A, actor.log_std_min, actor.log_std_max, actor.max_action, la, case["gamma"])
    sa = np.concatenate([ns, c["next_actions"]], axis=1)
    p1, p2 = critic_params_ or critic_params(case["critic"])
    q = np.stack([q_forward(p1, sa, dtype=np.float64)[0], q_forward(p2, sa, dtype=np.float64)[0]], axis=1)
    c = chain(heads, eps, q, rows, S, A, actor.log_std_min, actor.log_std_max, actor.max_action, la, case["gamma"])
    return c, heads, q


def torch_block(actor, critic, rows, eps, log_alpha, gamma, S, A):
    """The four reference lines (sac_pytorch.py:439-443) with Actor.sample written out on a given
    eps, in the tensors' dtype and on their device: (target_q [n, 1], next_actions, next_log_prob
    [n, 1], q1, q2)."""
    import torch
    with torch.no_grad():
        reward, ns, done = rows[:, S + A:S + A + 1], rows[:, S + A + 1:2 * S + A + 1], rows[:, 2 * S + A + 1:]
        mean, log_std = actor(ns)
        std = log_std.exp()
        x = mean + std * eps
        action = torch.tanh(x)
        log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727
                    - torch.log(1 - action.pow(2) + 1e-6)).sum(-1, keepdim=True)
        next_actions = action * actor.max_action
        q1, q2 = critic(ns, next_actions)
        next_q = torch.min(q1, q2) - log_alpha.exp() * log_prob
        target = reward + (1 - done) * gamma * next_q
    return target, next_actions, log_prob, q1, q2


def np_eps(seed, draw, n, A):
    """pd_sac_td_target's eps draws [n][A] in NumPy: Philox4x32-10 (philox_np), counter (row, draw
    lo, draw hi, 64 + k // 2), Box-Muller in binary64 with np.log, cast to float32."""
    import philox_np as ph
    pairs = (A + 1) // 2
    i = np.repeat(np.arange(n, dtype=np.uint64), pairs)
    tag = np.tile(64 + np.arange(pairs, dtype=np.uint64), n)
    d0 = np.full_like(i, draw & 0xFFFFFFFF)
    d1 = np.full_like(i, (draw >> 32) & 0xFFFFFFFF)
    x, y, z, w = ph.philox(i, d0, d1, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1, u2 = 1.0 - ph.u01(x, y), ph.u01(z, w)
    rho = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    zz = np.stack([rho * np.cos(ang), rho * np.sin(ang)], axis=1).reshape(n, 2 * pairs)
    return zz[:, :A]         # binary64: the caller casts
