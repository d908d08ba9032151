"""pd_per_sample / pd_per_update on the GPU against the NumPy model (tests/per_ref.py), and the
KernelPrioritizedReplayBuffer facade.

Every pd_per_sample call of this file goes through `run`, which carves the outputs and the scratch
out of larger sentinel-filled tensors and checks that nothing outside them changed (the scratch past
scratch_bytes included) and that the overflow flag info[2] is 0.

Bounds.  Keys: 32 ulp of binary64 relative (7.1e-15) against the model -- the device library's
documented bounds for double are log 3 ulp and pow 16 ulp, the division adds 0.5, NumPy's own log,
power and division about 2.5; rounded up.  Weights: 1 float32 ulp of the model's binary64 formula
cast to float32 (the binary64 error, about 1e-15, can only move the cast at a rounding boundary).
The selection is checked exactly against the kernel's own keys, and against the model's wherever
the model's first B + 1 sorted keys are further apart than 1e-9 relative (1e5 times the key bound),
which the test asserts first.  The largest key error seen is printed (tools/per_sample_time.py
records it in profiles/per_sample.json)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import per_ref

pytestmark = pytest.mark.gpu

SEED, ALPHA, BETA, WIDTH = 12345, 0.6, 0.4, 7
DRAWS = (0, 1, 2 ** 32 + 5)
SHAPES = [(1, 1), (2, 1), (5, 2), (63, 63), (64, 32), (65, 64), (257, 255), (1000, 256), (4097, 1024), (300_007, 512)]
PATTERNS = ("equal", "loguniform", "dirty")
GUARD = 64                      # sentinel elements (bytes for the scratch) on either side of an output
KEY_ERR = {"max": 0.0}


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def priorities(size, pattern, seed=5):
    """equal: a freshly filled ring (every row at the max priority); loguniform: 1e-6 .. 1e3; dirty:
    loguniform with zeros (every fifth item), one NaN and one negative value."""
    rng = np.random.default_rng(seed + size)
    if pattern == "equal":
        return np.ones(size, dtype=np.float32)
    p = (10.0 ** rng.uniform(-6, 3, size)).astype(np.float32)
    if pattern == "dirty":
        p[3::5] = 0.0
        if size > 1:
            p[1] = np.nan
        if size > 2:
            p[2] = -abs(p[2])
    return p


def ring_rows(size, seed=11):
    """[size, WIDTH] float32 rows of arbitrary bit patterns (finite or not: the gather is bitwise)."""
    rng = np.random.default_rng(seed + size)
    return rng.integers(-2 ** 31, 2 ** 31, (size, WIDTH), dtype=np.int64).astype(np.int32).view(np.float32)


class Carved:
    """A [n] region inside a sentinel-filled tensor of n + 2 GUARD elements."""

    def __init__(self, n, dtype, sentinel, device="cuda"):
        import torch
        self.full = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=device)
        self.ref = self.full.clone()
        self.view = self.full[GUARD:GUARD + n]
        self.n = n

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def guards_intact(self):
        import torch
        a, b = self.full.view(torch.uint8), self.ref.view(torch.uint8)
        k = GUARD * self.full.element_size()
        return bool(torch.equal(a[:k], b[:k]) and torch.equal(a[-k:], b[-k:]))


class Outputs:
    def __init__(self, L, size, batch, width, keys=True, scratch=None, scratch_for=None):
        import torch
        self.idx = Carved(batch, torch.int64, -7777)
        self.w = Carved(batch, torch.float32, 12345.0)
        self.rows = Carved(batch * width, torch.float32, 54321.0) if width else None
        self.keys = Carved(size, torch.float64, -9.0) if keys else None
        self.info = Carved(4, torch.int32, 99)
        self.scratch_bytes = int(L.pd_per_sample_scratch_bytes(*(scratch_for or (size, batch))))
        self.scratch = scratch if scratch is not None else Carved(self.scratch_bytes, torch.uint8, 0xA5)
        self.all = [c for c in (self.idx, self.w, self.rows, self.keys, self.info, self.scratch) if c is not None]


def run(pd, pri, batch, draw, data=None, alpha=ALPHA, beta=BETA, seed=SEED, keys=True, scratch=None, scratch_for=None):
    """One pd_per_sample call on device tensors `pri` [size] and `data` [size, W] (or None); returns
    the outputs as NumPy arrays (indices, weights, rows, keys, info) after the guard and overflow
    checks."""
    import torch
    L = pd.load()
    size = pri.numel()
    width = data.shape[1] if data is not None else 0
    o = Outputs(L, size, batch, width, keys=keys, scratch=scratch, scratch_for=scratch_for)
    st = L.pd_per_sample(C.c_void_p(pri.data_ptr()), size, batch, alpha, beta, seed, draw,
                         C.c_void_p(data.data_ptr()) if data is not None else None, width, o.idx.ptr(), o.w.ptr(),
                         o.rows.ptr() if o.rows else None, o.keys.ptr() if o.keys else None, o.info.ptr(),
                         o.scratch.ptr(), o.scratch_bytes, None)
    assert st == 0, L.pd_last_error()
    torch.cuda.synchronize()
    for c in o.all:
        assert c.guards_intact(), "a kernel wrote outside its output"
    info = o.info.view.cpu().numpy()
    assert info[2] == 0 and info[3] == 0
    rows = o.rows.view.cpu().numpy().reshape(batch, width) if o.rows else None
    return (o.idx.view.cpu().numpy(), o.w.view.cpu().numpy(), rows, o.keys.view.cpu().numpy() if o.keys else None, info)


def check_against_model(pri_np, data_np, batch, draw, out, beta=BETA):
    idx, w, rows, keys, info = out
    size = pri_np.size
    m_idx, m_w, m_keys, m_n, m_fin = per_ref.sample(pri_np, batch, ALPHA, beta, SEED, draw)
    # keys: +inf exactly where the model has it, the others within the bound
    assert np.array_equal(np.isinf(keys), np.isinf(m_keys)) and not np.isnan(keys).any() and (keys >= 0).all()
    fin = np.isfinite(m_keys)
    if fin.any():
        err = float(np.max(np.abs(keys[fin] - m_keys[fin]) / m_keys[fin]))
        KEY_ERR["max"] = max(KEY_ERR["max"], err)
        print(f"size {size} batch {batch} draw {draw}: key error {err / per_ref.ULP64:.2f} ulp "
              f"(largest so far {KEY_ERR['max'] / per_ref.ULP64:.2f}, bound 32)")
        assert err <= per_ref.KEY_BOUND
    assert info[0] == m_n and info[1] == m_fin
    # selection, exact against the kernel's own keys
    own, own_n = per_ref.select(keys, batch)
    assert own_n == m_n and np.array_equal(idx, own)
    # selection, independent: the model's, where its keys are well separated
    gap = per_ref.min_gap(m_keys, batch)
    assert gap > 1e-9, f"pick another draw for this shape: smallest relative key gap {gap:.2e}"
    assert np.array_equal(idx, m_idx)
    sel = idx[:m_n]
    assert len(set(sel.tolist())) == m_n and (sel >= 0).all() and (sel < size).all() and (idx[m_n:] == -1).all()
    # weights: 1 float32 ulp of the model, the largest exactly 1, 0 in the unfilled slots
    assert (np.abs(w.astype(np.float64) - m_w.astype(np.float64)) <= np.spacing(m_w).astype(np.float64)).all()
    if m_n:
        assert w.max() == np.float32(1.0)
    assert (w[m_n:] == 0).all()
    # rows: bit for bit, zeros in the unfilled slots
    if rows is not None:
        want = np.zeros((batch, data_np.shape[1]), dtype=np.float32)
        want[:m_n] = data_np[sel]
        assert np.array_equal(rows.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size,batch", SHAPES)
def test_sample_against_model(pd, size, batch, pattern):
    import torch
    draw = DRAWS[(SHAPES.index((size, batch)) + PATTERNS.index(pattern)) % 3]
    pri_np, data_np = priorities(size, pattern), ring_rows(size)
    pri, data = torch.from_numpy(pri_np).cuda(), torch.from_numpy(data_np).cuda()
    check_against_model(pri_np, data_np, batch, draw, run(pd, pri, batch, draw, data))


def test_unaligned_priorities_and_no_rows(pd):
    """A priority pointer that is only 4-byte aligned (no 16-byte loads) and a call without ring,
    rows and keys give the same indices and weights."""
    import torch
    size, batch = 1003, 128
    pri_np = priorities(size, "loguniform")
    base = torch.zeros(size + 1, dtype=torch.float32, device="cuda")
    base[1:] = torch.from_numpy(pri_np).cuda()
    a = run(pd, base[1:], batch, 1, keys=True)
    check_against_model(pri_np, None, batch, 1, a)
    b = run(pd, torch.from_numpy(pri_np).cuda(), batch, 1, keys=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_beta_range(pd):
    """beta 0 (every weight 1) and beta 1 against the model."""
    import torch
    pri_np, data_np = priorities(1000, "loguniform"), ring_rows(1000)
    pri, data = torch.from_numpy(pri_np).cuda(), torch.from_numpy(data_np).cuda()
    out = run(pd, pri, 256, 0, data, beta=0.0)
    assert (out[1] == 1.0).all()
    check_against_model(pri_np, data_np, 256, 0, run(pd, pri, 256, 0, data, beta=1.0), beta=1.0)


def test_shortfall(pd):
    """100 items, 7 of them positive, a batch of 16: 7 slots filled, the others index -1, weight 0
    and zero rows; the facade's check=True raises numpy's ValueError."""
    import torch
    from pdenv.sac import KernelPrioritizedReplayBuffer
    pri_np = np.zeros(100, dtype=np.float32)
    pri_np[[3, 10, 11, 50, 64, 98, 99]] = [0.5, 1.0, 2.0, 1e-6, 7.0, 3.0, 0.1]
    pri_np[20], pri_np[21] = np.nan, -1.0
    data_np = ring_rows(100)
    pri, data = torch.from_numpy(pri_np).cuda(), torch.from_numpy(data_np).cuda()
    out = run(pd, pri, 16, 2, data)
    idx, w, rows, keys, info = out
    assert info[0] == 7 and info[1] == 7
    assert (idx[7:] == -1).all() and (w[7:] == 0).all() and (rows[7:].view(np.int32) == 0).all()
    assert sorted(idx[:7].tolist()) == [3, 10, 11, 50, 64, 98, 99]
    check_against_model(pri_np, data_np, 16, 2, out)
    buf = KernelPrioritizedReplayBuffer(128, 2, 1, "cuda", seed=SEED)
    assert buf.width == WIDTH
    buf.add_batch(data)
    buf.priorities[:100] = pri
    assert buf.size == 100
    with pytest.raises(ValueError):
        buf.sample(16, check=True)
    s = buf.sample(16)                                        # unchecked: the short sample itself
    assert (s[6][7:] == -1).all() and (s[5][7:] == 0).all()
    assert len(buf.sample(7, check=True)) == 7
    with pytest.raises(ValueError):
        buf.sample(101)


def test_reproducible_and_scratch_hygiene(pd):
    """The same (seed, draw) gives equal bits in every output -- also on a scratch that a call of
    another size (300 007 items) left dirty in between; another draw gives another index set."""
    import torch
    L = pd.load()
    big_np, small_np = priorities(300_007, "loguniform"), priorities(4097, "loguniform")
    big, small = torch.from_numpy(big_np).cuda(), torch.from_numpy(small_np).cuda()
    data = torch.from_numpy(ring_rows(4097)).cuda()
    big_shape = (300_007, 1024)
    scratch = Carved(int(L.pd_per_sample_scratch_bytes(*big_shape)), torch.uint8, 0xA5)
    kw = dict(scratch=scratch, scratch_for=big_shape)
    a = run(pd, small, 512, 7, data, **kw)
    b = run(pd, small, 512, 7, data, **kw)
    run(pd, big, 1024, 3, **kw)
    c = run(pd, small, 512, 7, data, **kw)
    d = run(pd, small, 512, 7, data)                          # a fresh scratch of its own size
    for other in (b, c, d):
        for x, y in zip(a[:4], other[:4]):
            assert np.array_equal(x.view(np.int64 if x.itemsize == 8 else np.int32),
                                  y.view(np.int64 if y.itemsize == 8 else np.int32))
        assert np.array_equal(a[4], other[4])
    e = run(pd, small, 512, 8, data, **kw)
    assert set(e[0].tolist()) != set(a[0].tolist())
    f = run(pd, small, 512, 7, data, seed=SEED + 1, **kw)
    assert set(f[0].tolist()) != set(a[0].tolist())


def test_pair_probabilities_on_device(pd):
    """np.random.choice(5, 2, replace=False, p = prio**0.6)'s ordered pairs through the kernel: 20 000
    launches at size 5, frequencies within 5 sigma + 1e-3 of p_i p_j / (1 - p_i)
    (test_prioritized_buffer_on_device's bound)."""
    import torch
    L = pd.load()
    prio = (np.array([0.5, 1.0, 2.0, 4.0, 8.0]) + 1e-6).astype(np.float32)
    p = prio.astype(np.float64) ** 0.6
    p /= p.sum()
    T = 20000
    pri = torch.from_numpy(prio).cuda()
    idx = torch.full((T, 2), -5, dtype=torch.int64, device="cuda")
    w = torch.empty(T, 2, dtype=torch.float32, device="cuda")
    info = torch.full((T, 4), 9, dtype=torch.int32, device="cuda")
    nbytes = int(L.pd_per_sample_scratch_bytes(5, 2))
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    for t in range(T):
        st = L.pd_per_sample(C.c_void_p(pri.data_ptr()), 5, 2, 0.6, 0.4, 7, t, None, 0,
                             C.c_void_p(idx[t].data_ptr()), C.c_void_p(w[t].data_ptr()), None, None,
                             C.c_void_p(info[t].data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes, None)
        assert st == 0
    torch.cuda.synchronize()
    I = idx.cpu().numpy()
    assert (info.cpu().numpy() == np.array([2, 5, 0, 0])).all()
    # the kernel draws the model's pairs (the same seed and draws as test_per_cpu's model check)
    for t in (0, 1, T - 1):
        assert np.array_equal(I[t], per_ref.select(per_ref.keys(prio, 0.6, 7, t), 2)[0])
    for i, j in itertools.permutations(range(5), 2):
        e = p[i] * p[j] / (1 - p[i])
        f = np.mean((I[:, 0] == i) & (I[:, 1] == j))
        assert abs(f - e) < 5 * np.sqrt(e * (1 - e) / T) + 1e-3, (i, j, f, e)


def test_update(pd):
    """pd_per_update: the bits of td.abs().float() + eps at the indices, a sentinel everywhere else,
    the device maximum = max(old, p.max()) bitwise; a NaN td leaves the maximum alone; indices -1
    and `size` are skipped (their values do not count towards the maximum either)."""
    import torch
    L = pd.load()
    size, eps = 1000, 1e-6
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rng = np.random.default_rng(2)
    idx_np = rng.permutation(size)[:300].astype(np.int64)
    td_np = (rng.standard_normal(300) * 3).astype(np.float32)
    td_np[5], td_np[6] = 0.0, -0.0
    full = torch.full((size + 2 * GUARD,), -3.0, dtype=torch.float32, device="cuda")
    pri = full[GUARD:GUARD + size]
    idx, td = torch.from_numpy(idx_np).cuda(), torch.from_numpy(td_np).cuda()
    want = td.abs().float() + eps
    for old in (1.0, 100.0):
        full.fill_(-3.0)
        mx = torch.full((3,), old, dtype=torch.float32, device="cuda")
        assert L.pd_per_update(vp(pri), size, vp(idx), vp(td), 300, eps, vp(mx[1:]), None) == 0
        ref = torch.full_like(full, -3.0)
        ref[GUARD + idx] = want
        assert torch.equal(full.view(torch.int32), ref.view(torch.int32))
        new = max(old, float(want.max()))
        assert torch.equal(mx.view(torch.int32), torch.tensor([old, new, old], dtype=torch.float32).view(torch.int32).cuda())
    # a NaN and skipped indices: neither raises the maximum; the NaN priority itself is written
    idx2 = torch.tensor([4, -1, size, 7, 9, -2 ** 40, 2 ** 40], dtype=torch.int64, device="cuda")
    td2 = torch.tensor([float("nan"), 50.0, 60.0, -2.0, 0.5, 70.0, 80.0], dtype=torch.float32, device="cuda")
    full.fill_(-3.0)
    mx = torch.full((1,), 1.0, dtype=torch.float32, device="cuda")
    assert L.pd_per_update(vp(pri), size, vp(idx2), vp(td2), 7, eps, vp(mx), None) == 0
    got = full.cpu().numpy()
    assert got[GUARD + 7].view(np.int32) == (np.float32(2.0) + np.float32(eps)).view(np.int32)
    assert got[GUARD + 9].view(np.int32) == (np.float32(0.5) + np.float32(eps)).view(np.int32)
    assert np.isnan(got[GUARD + 4])
    keep = torch.ones_like(full, dtype=torch.bool)
    keep[[GUARD + 4, GUARD + 7, GUARD + 9]] = False
    assert bool((full[keep] == -3.0).all())
    assert float(mx) == float(np.float32(2.0) + np.float32(eps))
    mx.fill_(5.0)
    assert L.pd_per_update(vp(pri), size, vp(idx2[:1]), vp(td2[:1]), 1, eps, vp(mx), None) == 0
    assert float(mx) == 5.0


def test_facade(pd):
    """KernelPrioritizedReplayBuffer as a drop-in: the parent's 7-tuple (views of one [B, W] tensor),
    beta annealing, the draw counter, keys=True, max_priority on the device, add_batch's device fill,
    and the model's indices."""
    import torch
    from pdenv import KernelPrioritizedReplayBuffer
    from pdenv.sac import DevicePrioritizedReplayBuffer
    S, A = 2, 1
    buf = KernelPrioritizedReplayBuffer(600, S, A, "cuda", alpha=0.6, beta=0.4, beta_annealing_steps=10, seed=SEED)
    assert isinstance(buf, DevicePrioritizedReplayBuffer) and buf.sample(4) is None
    assert buf.max_priority == 1.0
    data_np = ring_rows(500)[:, :buf.width].copy()
    buf.add_batch(torch.from_numpy(data_np).cuda())
    assert buf.size == 500 and torch.equal(buf.priorities[:500].cpu(), torch.ones(500)) and float(buf.priorities[500]) == 0
    pri_np = priorities(500, "loguniform")
    buf.update_priorities(torch.arange(500, device="cuda"), torch.from_numpy(pri_np).cuda().double())
    want = torch.from_numpy(pri_np).cuda().abs().float() + 1e-6
    assert torch.equal(buf.priorities[:500].view(torch.int32), want.view(torch.int32))
    assert buf.max_priority == float(want.max())
    pri_np = buf.priorities[:500].cpu().numpy()
    out = buf.sample(64, keys=True)
    assert len(out) == 8 and buf.beta == pytest.approx(0.46) and buf.draws == 1
    s, a, r, s2, d, w, idx, keys = out
    assert [t.shape[1] for t in (s, a, r, s2, d, w)] == [S, A, 1, S, 1, 1] and idx.shape == (64,)
    assert len({t.untyped_storage().data_ptr() for t in (s, a, r, s2, d)}) == 1
    m_idx, m_w, m_keys, _, _ = per_ref.sample(pri_np, 64, 0.6, 0.4, SEED, 0)
    assert np.array_equal(idx.cpu().numpy(), m_idx)
    assert np.array_equal(torch.cat([s, a, r, s2, d], dim=1).cpu().numpy().view(np.int32), data_np[m_idx].view(np.int32))
    assert (np.abs(w.cpu().numpy().ravel().astype(np.float64) - m_w) <= np.spacing(m_w)).all()
    assert keys.shape == (500,) and np.allclose(keys.cpu().numpy(), m_keys, rtol=per_ref.KEY_BOUND, atol=0)
    first = idx.clone()
    out2 = buf.sample(64, check=True)                         # draw 1, beta 0.46
    assert len(out2) == 7 and buf.draws == 2 and out2[6].data_ptr() == idx.data_ptr()
    assert np.array_equal(out2[6].cpu().numpy(), per_ref.sample(pri_np, 64, 0.6, 0.46, SEED, 1)[0])
    again = buf.sample(64, draw=0)[6]                         # an explicit draw leaves the counter alone
    assert torch.equal(again, first) and buf.draws == 2
    # the setter fills the device value; new rows enter at it, filled on the device
    buf.max_priority = 3.5
    assert float(buf.max_prio_dev) == 3.5
    buf.add_batch(torch.zeros(150, buf.width, device="cuda"))   # wraps: 100 at the tail, 50 at the head
    assert (buf.priorities[500:] == 3.5).all() and (buf.priorities[:50] == 3.5).all() and buf.size == 600
    assert torch.equal(buf.priorities[50:500].cpu(), torch.from_numpy(pri_np[50:]))


def test_round_trip_with_the_collector(pd):
    """64 envs, capacity 512: collect(4), sample(32), update_priorities(idx, linspace(0, 5, 32)), one
    step(): the 64 new rows carry the bits of float32(5) + float32(1e-6), set by the step kernel from
    the device maximum with no host fill in between, and max_priority reads that value."""
    import torch
    from pdenv.sac import Actor, KernelPrioritizedReplayBuffer, SACCollector
    torch.manual_seed(3)
    env = pd.PoweredDescentEnv(64, flight_phase="landing_burn_pure_throttle", mode="rl", auto_reset=True, seed=8,
                               lanes_per_env=16)
    actor = Actor(env.obs_dim, env.action_dim).cuda()
    buf = KernelPrioritizedReplayBuffer(512, env.obs_dim, env.action_dim, "cuda", seed=1)
    col = SACCollector(env, actor, buf)
    assert col.ring
    col.collect(4)
    assert buf.size == 256 and (buf.priorities[:256] == 1.0).all() and (buf.priorities[256:] == 0).all()
    out = buf.sample(32, check=True)
    idx = out[6].clone()
    assert len(set(idx.tolist())) == 32 and int(idx.max()) < 256
    assert torch.equal(torch.cat(out[:5], dim=1).view(torch.int32), buf.data[idx].view(torch.int32))
    buf.update_priorities(idx, torch.linspace(0, 5, 32, device="cuda"))
    col.step()
    top = np.float32(5.0) + np.float32(1e-6)
    new = buf.priorities[256:320].cpu().numpy()
    assert buf.size == 320 and (new.view(np.int32) == top.view(np.int32)).all()
    assert buf.max_priority == float(top)
    assert (buf.priorities[320:] == 0).all()
