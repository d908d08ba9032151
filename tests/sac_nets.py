"""Inputs for the SAC actor kernel's tests (plain NumPy; no GPU, no torch at import).

Integer nets: weights, biases and observations are small integers chosen so that every partial
sum of every dot product of the forward pass is an integer below 2**24.  Every such integer is a
binary32 number, so any f32 evaluation -- any summation order, fused multiply-add or not, MFMA or
VALU -- gives the bits of integer arithmetic, and a wrong index, a stale weight block, a missed
term or a misplaced row gives a wrong integer.  The int64 forward pass is the reference.

Real nets: the reference Actor's default init with every weight matrix scaled and the biases
drawn from U(-0.5, 0.5), so that the heads are of order 1 and about half the units are live."""
import copy

import numpy as np

# (S, A, H, L) and what of sac_mlp_tile each shape reaches (pd_sac_mlp.h).  Layer 1: S = 2 and
# S = 5 have their own instantiations, every other S the generic one.  Heads: held in registers
# from the start ("early") when 2 A <= 512 / H, else read where they are used ("late").
SHAPES = [
    (1, 1, 128, 1),     # S = 1 (generic layer 1), no hidden layer, early heads partly filled
    (3, 2, 128, 4),     # early heads with every register in use (four outputs of 8 floats)
    (16, 8, 128, 2),    # late heads at H = 128; S = 16 (all 256 threads stage observations), A = 8
    (2, 1, 256, 8),     # S = 2 layer 1; L = 8 (20 parameter pointers, seven ping-pong swaps)
    (5, 4, 256, 3),     # S = 5 layer 1; late heads at H = 256
    (8, 3, 256, 2),     # generic layer 1; late heads, odd A
    (16, 1, 256, 1),    # early heads at H = 256 (two outputs of 16 floats), no hidden layer
    (2, 1, 512, 2),     # H = 512 with A = 1: late heads (2 A > 1), two columns per thread in layer 1
    (5, 4, 512, 3),     # H = 512, S = 5
    (9, 8, 512, 1),     # H = 512 heads straight from layer 1, A = 8
    (16, 8, 512, 8),    # the corner: every maximum at once
]
SHAPES_N = [(3, 2, 128, 4), (8, 3, 256, 2), (5, 4, 512, 3)]    # one per H, for the batch sizes
N_EXACT = 37            # two full 16-env tiles and one of five rows
EXACT_LIMIT = 2 ** 24


def int_actor(S, A, H, L, seed=0):
    """The integer net's parameters in pd_sac_actor's order -- W1 [H][S], b1, (W [H][H], b) x
    (L - 1), mean W [A][H], b, log_std W [A][H], b -- as float32 arrays.  Layer 1 and the heads:
    dense integers in [-2, 2]; hidden layers: entries of {-2, -1, 1, 2}, dense for L <= 3, else 4
    per row at random columns; biases: integers in [-3, 3]."""
    rng = np.random.default_rng([seed, S, A, H, L])
    vals = np.array([-2, -1, 1, 2])
    ps = [rng.integers(-2, 3, (H, S)), rng.integers(-3, 4, H)]
    for _ in range(L - 1):
        if L <= 3:
            W = vals[rng.integers(0, 4, (H, H))]
        else:
            W = np.zeros((H, H), dtype=np.int64)
            for j in range(H):
                W[j, rng.choice(H, 4, replace=False)] = vals[rng.integers(0, 4, 4)]
        ps += [W, rng.integers(-3, 4, H)]
    for _ in range(2):
        ps += [rng.integers(-2, 3, (A, H)), rng.integers(-3, 4, A)]
    return [np.ascontiguousarray(p, dtype=np.float32) for p in ps]


def int_obs(n, S, seed=0):
    """[n][S] integer observations in [-4, 4], float32."""
    return np.random.default_rng([seed, n, S, 77]).integers(-4, 5, (n, S)).astype(np.float32)


def forward(params, obs, dtype=np.int64):
    """The Actor's forward pass in `dtype` (int64 for the integer nets, float64 for the real
    ones): heads [n][2A] (mean | log_std, unclamped), and
      abs_sum: max over every layer and head of |h| |W|^T + |b|, the bound on every partial sum;
      live:    the share of positive units after the last hidden layer."""
    ps = [np.asarray(p).astype(dtype) for p in params]
    L = len(ps) // 2 - 2
    h = np.asarray(obs).astype(dtype)
    abs_sum = 0
    for l in range(L):
        W, b = ps[2 * l], ps[2 * l + 1]
        abs_sum = max(abs_sum, (np.abs(h) @ np.abs(W).T + np.abs(b)).max())
        h = np.maximum(h @ W.T + b, 0)
    live = float((h > 0).mean())
    out = []
    for W, b in ((ps[2 * L], ps[2 * L + 1]), (ps[2 * L + 2], ps[2 * L + 3])):
        abs_sum = max(abs_sum, (np.abs(h) @ np.abs(W).T + np.abs(b)).max())
        out.append(h @ W.T + b)
    return np.concatenate(out, axis=1), abs_sum, live


def int_case(S, A, H, L, n=N_EXACT, seed=0):
    """(params, obs [n][S], heads [n][2A] as float32) of an integer case, with the conditions on
    the inputs asserted: every partial sum below 2**24, between 0.2 and 0.8 of the units live
    after the last hidden layer, at least 8 distinct head values.  (Conditions, not measurements:
    a shape that misses one needs another seed or density, not another bound.)"""
    params, obs = int_actor(S, A, H, L, seed), int_obs(n, S, seed)
    ref, abs_sum, live = forward(params, obs)
    assert abs_sum < EXACT_LIMIT, (abs_sum, EXACT_LIMIT)
    assert 0.2 <= live <= 0.8, live
    assert len(np.unique(ref)) >= 8, np.unique(ref)
    assert np.array_equal(ref.astype(np.float32).astype(np.int64), ref)
    return params, obs, ref.astype(np.float32)


def load_actor(actor, params):
    """Copy `params` (pd_sac_actor's order) into a pdenv.sac.Actor, in place."""
    import torch
    import torch.nn as nn
    lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)] + [actor.mean, actor.log_std]
    assert len(params) == 2 * len(lins)
    with torch.no_grad():
        for k, m in enumerate(lins):
            for t, p in ((m.weight, params[2 * k]), (m.bias, params[2 * k + 1])):
                assert tuple(t.shape) == p.shape, (k, tuple(t.shape), p.shape)
                t.copy_(torch.from_numpy(np.asarray(p)))
    return actor


def actor_params(actor):
    """The Actor's parameters in pd_sac_actor's order as float32 NumPy arrays."""
    import torch.nn as nn
    lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)] + [actor.mean, actor.log_std]
    return [t.detach().cpu().numpy() for m in lins for t in (m.weight, m.bias)]


N_REAL = 261            # 16 full tiles and one of five rows
REAL_GAIN = 2.0         # see real_case


def real_case(S, A, H, L, n=N_REAL, seed=0, gain=REAL_GAIN):
    """(actor on the CPU, obs [n][S] float32, float64 heads of the same float32 parameters, live
    share): Actor default init, U(-1/sqrt(fan_in), 1/sqrt(fan_in)), every weight matrix times
    `gain`, biases U(-0.5, 0.5), observations U(-2, 2).  The default init alone shrinks the
    activations' variance by 6 per ReLU layer (weight variance 1 / (3 fan_in), half the units
    live); gain 2 brings that to 2/3 per layer and the biases refill it, so the heads stay of
    order 1 down to L = 8 without growing.  The caller asserts max |head| in [0.1, 1e3] and a live
    share in [0.2, 0.8]."""
    import torch
    from pdenv.sac import Actor
    g = torch.Generator().manual_seed(1000 * seed + 97 * S + 13 * A + H + L)
    actor = Actor(S, A, hidden_dim=H, n_hidden_layers=L)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                bound = 1.0 / np.sqrt(p.shape[1])
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (bound * gain))
            else:
                p.copy_(torch.rand(p.shape, generator=g) - 0.5)
    obs = (torch.rand(n, S, generator=g) * 4 - 2).contiguous()
    _, _, live = forward(actor_params(actor), obs.numpy(), dtype=np.float64)
    with torch.no_grad():
        a64 = copy.deepcopy(actor).double()
        f = a64.shared_net(obs.double())
        ref = torch.cat([a64.mean(f), a64.log_std(f)], dim=1)
    return actor, obs, ref, live
