"""GPU: the search intervals the step kernel carries across sub-steps (wind profile knots, grid-fin
C_a knots: a guess checked by the search's own postcondition, the search itself as the fallback;
the clamped-line breakpoint search takes none: with one the c3 kernel measured 2-4 % slower, the
"not kept" entry of DESIGN.md s6, tools/experiments/line_carry.patch) and the action row it
requests one step ahead.  Neither may change a bit:
every case compares a default handle with one created with PD_TABLES_NO_CARRY (every guess fails)
or with per-step launches, with torch.equal."""
import numpy as np
import pytest

from pdenv import _lib as L

pytestmark = pytest.mark.gpu

ST = ["x", "y", "vx", "vy", "theta", "theta_dot", "gamma", "alpha", "mass", "mass_propellant", "time"]
C3 = dict(lanes_per_env=2, enable_wind=True, stochastic_wind=True, wind_percentile=None, auto_reset=True,
          tilt_sigma_rad=0.02)


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def make(pd, n, phase="landing_burn_pure_throttle", mode="rl", **kw):
    return pd.PoweredDescentEnv(n, flight_phase=phase, mode=mode, **kw)


def mixed_actions(T, N, A, seed):
    """U(-1, 1) actions, the first 3/4 of the envs at high throttle (test_fine_index_bit_identical's
    3:1 mix; the throttle is component 1 where there are several)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.rand(T, N, A, device="cuda", generator=g) * 2 - 1
    c = min(1, A - 1)
    a[:, : 3 * N // 4, c] = a[:, : 3 * N // 4, c] * 0.25 + 0.75
    return a.contiguous()


def run_launches(env, acts, launches):
    """step_n over consecutive launches of the given lengths (each one fused launch); every output."""
    outs, t0 = [], 0
    env.set_tuning(step_fuse=max(launches))
    for n in launches:
        outs.append(env.step_n(acts[t0:t0 + n].contiguous()))
        t0 += n
    return outs


def assert_same(o1, o2, what):
    import torch
    assert len(o1) == len(o2)
    for k, (l1, l2) in enumerate(zip(o1, o2)):
        for j, (x, y) in enumerate(zip(l1, l2)):
            assert torch.equal(x, y), (what, "launch", k, "output", j)


CASES = [
    # name, env count, phase, mode, handle settings, the searches the configuration has counters for
    ("c3", 512, "landing_burn_pure_throttle", "rl", dict(C3, seed=13), ("wind", "fin")),
    ("landing_burn_pso", 256, "landing_burn", "pso", dict(C3, seed=17), ("wind", "fin")),
    # (16 lanes per env, windless: the c2 / c5 path; the counting kernel exists at 2 lanes only)
    ("lpe16_windless", 64, "landing_burn_pure_throttle", "rl",
     dict(lanes_per_env=16, auto_reset=True, tilt_sigma_rad=0.02, seed=19), ()),
]


@pytest.mark.parametrize("name,n,phase,mode,kw,searches", CASES, ids=[c[0] for c in CASES])
def test_carry_bit_identical(pd, name, n, phase, mode, kw, searches):
    """160 steps as launches of 64 + 64 + 32, carry against PD_TABLES_NO_CARRY: every output of
    every step and the final state are equal.  Not vacuous: a third handle runs the same launches
    with counting on (the counting instantiation; equal too) and must report, for each search,
    wave sub-steps in which every guess held and wave sub-steps in which the search ran, and
    resets.  (The carried word starts empty in every launch, so each launch's first sub-step
    searches; later searches are the lanes whose interval changed.)"""
    import torch
    launches = (64, 64, 32)
    carry = make(pd, n, phase, mode, **kw)
    plain = make(pd, n, phase, mode, table_flags=L.TABLES_NO_CARRY, **kw)
    acts = mixed_actions(sum(launches), n, carry.action_dim, 31)
    o1 = run_launches(carry, acts, launches)
    o2 = run_launches(plain, acts, launches)
    assert_same(o1, o2, name)
    assert torch.equal(carry.state, plain.state)
    if searches:
        cnt = make(pd, n, phase, mode, **kw)
        cnt.count_work(True)
        o3 = run_launches(cnt, acts, launches)
        assert_same(o1, o3, name + " counting")
        st = cnt.stats()
        print(name, {k: v for k, v in st.items() if k.startswith("carry_") or k == "resets"})
        assert st["resets"] > 0, st
        for s in searches:
            assert st[f"carry_{s}_hit"] > 0 and st[f"carry_{s}_search"] > 0, (s, st)
        # the flag turns every guess off
        off = make(pd, n, phase, mode, table_flags=L.TABLES_NO_CARRY, **kw)
        off.count_work(True)
        off.set_tuning(step_fuse=8)
        off.step_n(acts[:8].contiguous())
        so = off.stats()
        assert all(so[f"carry_{s}_hit"] == 0 and so[f"carry_{s}_search"] > 0 for s in searches), so


def _exact_quotient(target, denom):
    """A double y with y / denom == target exactly (searched over the neighbouring doubles of
    target * denom), or the nearest one."""
    y = np.float64(target) * denom
    for c in [y] + [f(y, k) for k in range(1, 9) for f in (lambda v, k: _ulps(v, k), lambda v, k: _ulps(v, -k))]:
        if c / denom == target:
            return float(c)
    return float(y)


def _ulps(v, k):
    v = np.float64(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def test_carry_boundaries(pd, oracle_mod):
    """One launch of 2 steps from states on the searches' boundaries: Mach on a dense sweep of
    [0.05, 9.95] on a clamped line (alpha_eff 0.05 rad clamps both tables), so that many envs cross
    line breakpoints and grid-fin knots between sub-steps (at 40 km, where Mach 10 is inside the
    flight envelope -- q = rho (M a)^2 / 2 ~ 2e4 Pa, under the 65 kPa truncation limit -- as the
    states of the teacher-forced fixture are: the rounding differences between the device and the
    oracle scale with the forces, and the tolerance is the fixture's); altitudes with y / 1000 exactly on the
    wind profile's knots, one ulp either side, below the first and at / above the last knot, and
    a few metres above each knot (crossed during the 8 sub-steps); Mach just below and at the
    grid-fin table's first knot (ca_min_mach).  Carry and PD_TABLES_NO_CARRY are bit-identical and
    both within test_gpu_parity's teacher-forced tolerance of the oracle (1e-10 relative per
    channel, theta_dot 1e-8, floor 1e-3)."""
    import torch
    probe = make(pd, 1)
    s0 = probe.state.cpu().numpy()[0]
    from pdenv import params as PR
    pk = PR.load_pack()
    assert pk["wind_profiles"][0]["percentile"] == 50
    knots = np.array(pk["wind_profiles"][0]["alt_km"], dtype=np.float64)
    ca_min = float(np.array(pk["grid_fin_ca"]["min_mach"]).ravel()[0])

    def sound(y):
        return float(probe.atmosphere(torch.tensor([y], dtype=torch.float64, device="cuda"))[2][0])

    rows = []

    # the velocity keeps the direction of the nominal initial state (vx ~ 0.2 vy: a vertical fall
    # would leave vx the difference of cancelling forces, with no scale for a relative tolerance)
    d0 = s0[2:4] / np.hypot(s0[2], s0[3])

    def add(y, mach=None, vel=None):
        s = s0.copy()
        s[1] = y
        s[2:4] = mach * sound(y) * d0 if vel is None else vel
        g = np.arctan2(s[3], s[2])
        s[6] = g + 2 * np.pi if g < 0 else g                    # gamma as the integrator leaves it
        s[4] = s[6] - np.pi - 0.05                              # alpha_eff = gamma - theta - pi = 0.05 rad
        s[7] = s[4] - s[6]
        rows.append(s)

    for m in np.arange(0.05, 9.951, 0.025):                     # the Mach sweep at 40 km
        add(40000.0, mach=float(m))
    for kx in knots:
        for t in (kx, _ulps(kx, 1), _ulps(kx, -1)):             # on the knot, one ulp either side
            add(_exact_quotient(t, 1000.0), mach=0.9)
        for d in (3.0, 10.0, 20.0, 40.0):                       # crossed within the launch (~7 m per sub-step)
            if kx * 1000.0 + d < 80000.0:
                add(float(kx) * 1000.0 + d, mach=0.9)
    add(float(knots[0]) * 1000.0 - 200.0, mach=0.5)             # below the first knot
    add(float(knots[-1]) * 1000.0 + 500.0, mach=0.9)            # above the last
    for y in (12000.0, 3000.0):                                 # Mach at and just below ca_min_mach
        a = sound(y)
        vx, vy = ca_min * a * d0

        def mach_of(vyc):                                       # the kernel's operations, in its order
            return np.sqrt(vx * vx + vyc * vyc) / np.float64(a)
        hit = next((c for c in [_ulps(vy, k) for k in range(-64, 65)] if mach_of(c) == ca_min), np.float64(vy))
        for vv in (hit, _ulps(hit, 1), _ulps(hit, 8), _ulps(hit, -1), _ulps(hit, -8), hit * 1.002, hit * 0.998):
            add(y, vel=np.array([vx, float(vv)]))
    S = np.array(rows)
    n = len(S)
    rng = np.random.default_rng(7)
    A = rng.uniform(-1, 1, (2, n, 1)).astype(np.float32)
    kw = dict(lanes_per_env=2, enable_wind=True, stochastic_wind=False, wind_percentile=50, auto_reset=False)
    outs = []
    for flags in (0, L.TABLES_NO_CARRY):
        env = make(pd, n, table_flags=flags, **kw)
        env.set_state(torch.tensor(S, device="cuda"))
        env.set_tuning(step_fuse=2)
        o = env.step_n(torch.tensor(A, device="cuda"))
        outs.append((o, env.state.clone()))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert torch.equal(x, y)
    assert torch.equal(outs[0][1], outs[1][1])
    got = outs[0][1].cpu().numpy()
    ref = np.empty_like(got)
    o = oracle_mod.Oracle(phase=0, rtd=0, wind=True, stochastic=False, wind_percentile=50)
    for i in range(n):
        o.reset(S[i])
        for t in range(2):
            o.step(A[t, i], f32=True)
        ref[i] = o.state
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
    tol = np.full(11, 1e-10); tol[5] = 1e-8
    print("boundaries: max relative error per channel", {k: float(v) for k, v in zip(ST, err.max(0))},
          "worst env", int(err.max(1).argmax()), "y, vy", S[int(err.max(1).argmax()), [1, 3]])
    assert (err.max(0) < tol).all(), dict(zip(ST, err.max(0)))


def test_carry_launch_split(pd):
    """The carried word is not kept between launches: 64 launches of one step, one launch of 64
    and two of 32 give the same bits; step_n of one step equals step()."""
    import torch
    n, T = 512, 64
    kw = dict(C3, seed=23)
    acts = mixed_actions(T, n, 1, 5)
    ref = run_launches(make(pd, n, **kw), acts, (64,))
    whole = [torch.cat([o[j] for o in ref]) for j in range(5)]
    for launches in ((1,) * 64, (32, 32)):
        env = make(pd, n, **kw)
        got = run_launches(env, acts, launches)
        for j in range(5):
            assert torch.equal(torch.cat([o[j] for o in got]), whole[j]), (launches[0], j)
    e1, e2 = make(pd, n, **kw), make(pd, n, **kw)
    obs, r, dn, tr, ex = e1.step(acts[0])
    o2 = e2.step_n(acts[0:1].contiguous())
    assert torch.equal(obs, o2[0][0]) and torch.equal(r, o2[1][0]) and torch.equal(dn, o2[2][0])
    assert torch.equal(tr, o2[3][0]) and torch.equal(ex["trunc_id"], o2[4][0])
    assert torch.equal(e1.state, e2.state)


@pytest.mark.parametrize("nf", [1, 2, 5])
@pytest.mark.parametrize("f64", [False, True], ids=["act32", "act64"])
def test_action_rows_one_step_ahead(pd, f64, nf):
    """The fused launch requests row f + 1 of the actions during step f and nothing past row
    nf - 1: with an action tensor of exactly [nf, N, A] (its own allocation), binary32 and binary64
    rows, the outputs equal those of nf one-step launches."""
    import torch
    n = 512
    kw = dict(C3, seed=29, action_f64=f64)
    g = torch.Generator(device="cuda").manual_seed(100 + nf)
    acts = (torch.rand(nf, n, 1, device="cuda", generator=g, dtype=torch.float64 if f64 else torch.float32) * 2 - 1)
    acts = acts.clone().contiguous()
    assert tuple(acts.shape) == (nf, n, 1) and acts.untyped_storage().nbytes() == acts.numel() * acts.element_size()
    fused, single = make(pd, n, **kw), make(pd, n, **kw)
    fused.set_tuning(step_fuse=8)
    of = fused.step_n(acts)
    for t in range(nf):
        obs, r, dn, tr, ex = single.step(acts[t])
        assert torch.equal(of[0][t], obs) and torch.equal(of[1][t], r), t
        assert torch.equal(of[2][t], dn) and torch.equal(of[3][t], tr) and torch.equal(of[4][t], ex["trunc_id"]), t
    assert torch.equal(fused.state, single.state)
