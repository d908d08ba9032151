"""GPU: the work the 2-lane binary64 step kernels share inside a sub-step (PD_MERGE):
the sub-step's seven true divisions as four division sequences over an env's lane pair (Mach with
inertia's x_prop, x_wet with the gravity ratio, F_x / m with F_y / m, M_z / I alone).  It may not
change a bit.  The same cases also anchor tools/experiments/merge_pieces.patch (one evaluator for a
wave's Taylor-piece and cell-piece queries; measured slower and not in the product), which is why
they are built around the composition of a wave.

The counting instantiation (count_work(True)) keeps the five division sequences (and, under the
patch, the split evaluators): a second, independently compiled implementation on the same device.
Every case compares the default kernel with a counting handle with torch.equal on every output of
every step and on the final state, reads the counting handle's counters to show that the waves
held what the case claims, and teacher-forces the default handle against the oracle at the c3
tolerances (tests/shadow.py), so that the anchor is the reference and not the code under test.

Crafted waves: one env-step (four sub-steps), n = 64 (two full waves of 32 envs) and n = 33 (a
full wave and a wave of one env with 62 idle lanes).  Both tables clamp at the same
|alpha_eff| = radians(10) / rad2deg = 10 / rad2deg^2 ~ 0.003046 rad, so an env is on a clamped
line with both of its lanes or interior with both.  alpha_eff = gamma - theta - pi on a descending
vehicle: "line" envs have +-0.05 rad, "interior" envs +-0.0015 rad (gamma turns by ~5e-4 rad in
the 0.1 s of a step), so every env keeps its kind through the four sub-steps and the number of mixed
wave sub-steps is four times the number of waves holding both kinds.
"""
import math

import numpy as np
import pytest

from test_gpu_carry import C3, assert_same, make, mixed_actions, run_launches

pytestmark = pytest.mark.gpu

SEED = 41
TILT = C3["tilt_sigma_rad"]
LINE, INNER = 0.05, 0.0015


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


@pytest.fixture(scope="module")
def nominal(pd):
    """The nominal initial state of the pure-throttle landing burn (no tilt)."""
    return make(pd, 1, tilt_sigma_rad=0.0).state.cpu().numpy()[0].copy()


def _alpha_eff(ga, th):
    """The kernel's alpha_effective of a descending vehicle, in its order of operations."""
    return (np.float64(ga) - np.float64(th)) - np.float64(math.pi)


def _clamped(ae):
    """cd_query's clamp test, in its order of operations."""
    r10 = np.float64(10.0 * (math.pi / 180.0))
    return abs(np.float64(ae) * np.float64(180.0 / math.pi)) > r10


def _theta_at_clamp(ga, sign, steps):
    """theta with alpha_eff `steps` values of the subtraction's result grid (4.4e-16 rad: theta and
    gamma are ~ 1.4 and ~ 4.5) past the clamp (steps > 0: clamped, on the line; steps <= 0:
    |steps| + 1 values inside it), on the positive (sign = 1) or negative side."""
    t0 = np.float64(10.0 * (math.pi / 180.0)) / np.float64(180.0 / math.pi)
    lo, hi = np.float64(ga - math.pi - sign * (t0 - 1e-9)), np.float64(ga - math.pi - sign * (t0 + 1e-9))
    assert not _clamped(_alpha_eff(ga, lo)) and _clamped(_alpha_eff(ga, hi))
    while True:                                   # bisection over theta down to adjacent doubles
        mid = np.float64(0.5) * (lo + hi)
        if mid == lo or mid == hi:
            break
        if _clamped(_alpha_eff(ga, mid)):
            hi = mid
        else:
            lo = mid
    th = hi if steps > 0 else lo                  # the first clamped / the last interior theta
    out = np.inf if (hi > lo) == (steps > 0) else -np.inf   # (away from the clamp, on theta's own grid)
    for _ in range(abs(steps) - (1 if steps > 0 else 0)):
        th = np.nextafter(th, out)
    assert _clamped(_alpha_eff(ga, th)) == (steps > 0)
    return float(th)


def crafted(s0, kinds, speed=None, y=None, theta=None, mp=None):
    """States [n, 11]: env i has alpha_eff = kinds[i] (or the given theta), the nominal velocity's
    direction at 0.5 .. 1.0 of its speed (another Mach per env), the nominal altitude unless given."""
    n = len(kinds)
    S = np.tile(s0, (n, 1))
    for i in range(n):
        f = (0.5 + 0.5 * i / max(n - 1, 1)) if speed is None else speed[i]
        S[i, 2:4] = s0[2:4] * f
        assert S[i, 3] < 0
        g = math.atan2(S[i, 3], S[i, 2])
        S[i, 6] = g + 2 * math.pi if g < 0 else g              # gamma as the integrator leaves it
        S[i, 4] = S[i, 6] - math.pi - kinds[i] if theta is None or theta[i] is None else theta[i]
        S[i, 5] = 0.0
        S[i, 7] = S[i, 4] - S[i, 6]
        if y is not None and y[i] is not None:
            S[i, 1] = y[i]
        if mp is not None and mp[i] is not None:
            S[i, 8] += mp[i] - S[i, 9]
            S[i, 9] = mp[i]
    return S


def on_line(S):
    return np.array([_clamped(_alpha_eff(S[i, 6], S[i, 4])) for i in range(len(S))])


def mixed_waves(line, free=()):
    """Waves (32 envs) that hold both kinds, whatever the envs in `free` (near the clamp) do."""
    m = 0
    for w0 in range(0, len(line), 32):
        k = [line[i] for i in range(w0, min(w0 + 32, len(line))) if i not in free]
        m += int(any(k) and not all(k))
    return m


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def one_step_case(pd, oracle_mod, S, A, shadow_idx, bitwise=False):
    """One env-step from states S with actions A [1, n, 1]: the default handle (teacher-forced
    against the oracle on shadow_idx) and a counting handle; every output and the final state
    equal.  Returns the counting handle's counters and both handles."""
    import torch
    from shadow import check_stats, shadow_run
    n = len(S)
    kw = dict(C3, seed=SEED)
    dflt, cnt = make(pd, n, **kw), make(pd, n, **kw)
    St = torch.tensor(S, device="cuda")
    dflt.set_state(St)
    cnt.set_state(St)
    cnt.count_work(True)
    At = torch.tensor(A, device="cuda")
    st = shadow_run(oracle_mod, dflt, At, np.asarray(shadow_idx), 0, 0, SEED, TILT)
    check_stats(st)
    assert st["steps"] == len(shadow_idx)
    obs, rew, dn, tr, ex = cnt.step(At[0])
    o = st["outs"]
    eq = (lambda x, y: torch.equal(_bits(x), _bits(y))) if bitwise else torch.equal
    assert eq(o["obs"][0], obs) and eq(o["rew"][0], rew)
    assert torch.equal(o["done"][0], dn) and torch.equal(o["trunc"][0], tr) and torch.equal(o["tid"][0], ex["trunc_id"])
    assert eq(dflt.state, cnt.state)
    return cnt.stats(), dflt, cnt


def check_counts(c, n, mixed, what):
    """The counting handle's record of one env-step of n envs: 8 n queries (2 lanes, 4 sub-steps),
    `mixed` mixed wave sub-steps, and the piece paths carrying at least 99 % of the queries."""
    q = 8 * n
    print(what, n, {k: c[k] for k in ("q_line", "q_taylor", "q_cell", "q_verified", "q_balanced", "q_miss",
                                      "wave_substeps_mixed")})
    assert c["wave_substeps_mixed"] == mixed, (what, c)
    assert c["q_taylor"] + c["q_cell"] + c["q_balanced"] + c["q_miss"] == q, (what, c)
    assert 100 * c["q_verified"] <= q and 100 * (c["q_balanced"] + c["q_miss"]) <= q, (what, c)
    if mixed:
        assert c["q_taylor"] > 0 and c["q_cell"] > 0, (what, c)


def _kinds(name, n):
    sg = [1.0 if (i // 2) % 2 == 0 else -1.0 for i in range(n)]    # both lines, both halves of the cells
    if name == "all_line":
        return [sg[i] * LINE for i in range(n)]
    if name == "all_interior":
        return [sg[i] * INNER for i in range(n)]
    if name == "alternating":
        return [sg[i] * (LINE if i % 2 == 0 else INNER) for i in range(n)]
    if name == "one_interior":
        return [sg[i] * (INNER if i == 5 else LINE) for i in range(n)]
    if name == "one_line":
        return [sg[i] * (LINE if i == 5 else INNER) for i in range(n)]
    raise KeyError(name)


def _actions(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (1, n, 1)).astype(np.float32)


@pytest.mark.parametrize("n", [64, 33])
@pytest.mark.parametrize("name", ["all_line", "all_interior", "alternating", "one_interior", "one_line"])
def test_merge_crafted_waves(pd, oracle_mod, nominal, name, n):
    """Waves of one kind, alternating kinds, and one env of the other kind in a wave."""
    S = crafted(nominal, _kinds(name, n))
    line = on_line(S)
    c, _, _ = one_step_case(pd, oracle_mod, S, _actions(n, 3), np.arange(n))
    check_counts(c, n, 4 * mixed_waves(line), name)
    if name == "all_line":
        assert c["q_cell"] == 0 and c["q_line"] == 8 * n
    if name == "all_interior":
        assert c["q_taylor"] == 0 and c["q_line"] == 0


@pytest.mark.parametrize("n", [64, 33])
def test_merge_at_the_clamp(pd, oracle_mod, nominal, n):
    """alpha_eff within a few values of the clamp on either side, on both signs (envs 2, 6, 10, 38),
    among line envs (i % 4 == 0) and interior envs (odd i): every full wave is mixed whatever the
    envs at the clamp do after their first sub-step.  (An env just inside the clamp lies within the
    grid's rounding margin of its edge and is verified: at most two such envs in 64, one in 33.)"""
    kinds = [(LINE if i % 4 == 0 else (INNER if i % 2 else -LINE)) for i in range(n)]
    S = crafted(nominal, kinds)
    near = {2: (1.0, 2), 6: (1.0, -1), 10: (-1.0, 1), 38: (-1.0, -2)}
    near = {i: v for i, v in near.items() if i < n}
    for i, (sign, steps) in near.items():
        S[i, 4] = _theta_at_clamp(S[i, 6], sign, steps)
        S[i, 7] = S[i, 4] - S[i, 6]
    line = on_line(S)
    assert all(line[i] == (near[i][1] > 0) for i in near)
    c, _, _ = one_step_case(pd, oracle_mod, S, _actions(n, 5), np.arange(n))
    check_counts(c, n, 4 * mixed_waves(line, free=set(near)), "clamp")


@pytest.mark.parametrize("n", [64, 33])
def test_merge_unused_queries(pd, oracle_mod, nominal, n):
    """Queries whose value is discarded, between line and interior envs: |deg(deg(alpha_eff))| < 1e-6
    (C_L exactly 0; i % 4 == 2) and altitudes above 81 km (speed of sound 0, Mach 0, neither
    coefficient used; i % 4 == 3, on either line: an interior query at Mach exactly 0 lies on the
    grid's edge and is verified, not a piece query)."""
    kinds = [[LINE, -INNER, 1e-10, (LINE if (i // 4) % 2 else -LINE)][i % 4] for i in range(n)]
    y = [85000.0 + 10.0 * i if i % 4 == 3 else None for i in range(n)]
    S = crafted(nominal, kinds, y=y)
    line = on_line(S)
    c, _, _ = one_step_case(pd, oracle_mod, S, _actions(n, 7), np.arange(n))
    check_counts(c, n, 4 * mixed_waves(line), "unused")


def test_merge_divisions(pd, oracle_mod, nominal):
    """The paired divisions' special operands in one step: speed of sound 0 (above 81 km: the
    Mach lane's quotient is not used), fuel consumed 0 (a full tank: the 1e-6 substitute enters
    x_prop), and a NaN force (a NaN action: the NaN guard zeroes the control force and counts the
    event; that env's outputs are NaN and compared by their bits, and it is not shadowed.  One such
    env: its mass is NaN after the first sub-step, its speed after the second, so its four queries
    of sub-steps 3 and 4 are NaN queries, verified -- under 1 % of the 512)."""
    from pdenv import params as PR
    n = 64
    m_prop0 = float(PR.load_pack()["sizing"]["m_prop0"])
    kinds = _kinds("alternating", n)
    y = [None] * n
    mp = [None] * n
    for i in (2, 4, 34):                          # (line envs: see test_merge_unused_queries)
        y[i] = 85000.0 + i
    for i in (5, 8, 36):
        mp[i] = m_prop0
    S = crafted(nominal, kinds, y=y, mp=mp)
    A = _actions(n, 9)
    nan_envs = (7,)
    for i in nan_envs:
        A[0, i, 0] = np.nan
    idx = np.array([i for i in range(n) if i not in nan_envs])
    c, dflt, cnt = one_step_case(pd, oracle_mod, S, A, idx, bitwise=True)
    check_counts(c, n, 4 * mixed_waves(on_line(S)), "divisions")
    nd, nc = dflt.counters()["nan_events"], cnt.counters()["nan_events"]
    assert nd == nc and nd >= len(nan_envs), (nd, nc)


FREE = [
    ("c3", 512, "landing_burn_pure_throttle", "rl", 0, 0, 13),
    ("landing_burn_pso", 256, "landing_burn", "pso", 1, 1, 17),
]


@pytest.mark.parametrize("name,n,phase,mode,oph,ortd,seed", FREE, ids=[c[0] for c in FREE])
def test_merge_free_running(pd, oracle_mod, name, n, phase, mode, oph, ortd, seed):
    """160 free-running steps (test_gpu_carry.py's c3 settings, 3:1 action mix, auto-reset) as
    launches of 64 + 64 + 32, as 160 one-step launches and on a counting handle: equal in every
    output of every step and in the final state; a fourth handle stepped by pd_step is
    teacher-forced against the oracle on every 16th env and equal to them too."""
    import torch
    from shadow import check_stats, shadow_run
    launches = (64, 64, 32)
    kw = dict(C3, seed=seed)
    fused = make(pd, n, phase, mode, **kw)
    acts = mixed_actions(sum(launches), n, fused.action_dim, 31)
    o1 = run_launches(fused, acts, launches)
    cnt = make(pd, n, phase, mode, **kw)
    cnt.count_work(True)
    o3 = run_launches(cnt, acts, launches)
    assert_same(o1, o3, name + " counting")
    assert torch.equal(fused.state, cnt.state)
    whole = [torch.cat([o[j] for o in o1]) for j in range(5)]
    single = make(pd, n, phase, mode, **kw)
    o2 = run_launches(single, acts, (1,) * sum(launches))
    for j in range(5):
        assert torch.equal(torch.cat([o[j] for o in o2]), whole[j]), (name, "one-step launches", j)
    assert torch.equal(fused.state, single.state)
    shadowed = make(pd, n, phase, mode, **kw)
    st = shadow_run(oracle_mod, shadowed, acts, np.arange(0, n, 16), oph, ortd, seed, TILT)
    check_stats(st)
    for j, k in enumerate(("obs", "rew", "done", "trunc", "tid")):
        assert torch.equal(st["outs"][k], whole[j]), (name, "pd_step", k)
    assert torch.equal(fused.state, shadowed.state)
    c = cnt.stats()
    print(name, {k: c[k] for k in ("q_taylor", "q_cell", "q_refined", "q_bisect", "wave_substeps_mixed", "resets")})
    for k in ("q_taylor", "q_cell", "q_refined", "q_bisect", "wave_substeps_mixed", "resets"):
        assert c[k] > 0, (name, k, c)
