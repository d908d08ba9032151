"""GPU parity WITH WIND for the flight phases besides the two landing burns
(landing_burn_pure_throttle_Pcontrol, ballistic_arc_descent, flip_over_boostbackburn, subsonic,
supersonic): the step kernel's one-physics-call-per-step family with the wind path compiled in, at
every lanes-per-env value.  The reference turns wind on by default for every phase
(base_environment.py:16-18); tests/test_gpu_phases.py is windless and the other windy GPU tests
cover only the two landing burns.

1. test_teacher_forced_wind_vs_reference: the reference's own numbers
   (tests/golden/ref_phases_wind.npz, made by make_golden.py phases_wind): per-env percentile,
   sigmas, non-zero filter pre-states and injected normals; next state, filter states, the info
   tap's gusts, wind forces and moment, mass flow.
   test_vertical_gust_force_and_moment_arm: the same rows with C_gust_y = 1 (the reference's
   is 0.0, which hides F_wind_y and M_wind_z), the moment arm against the reference's d_cp_cg.
2. test_free_running_wind_shadowed: Philox gust draws, per-reset sigmas/percentile/tilt and
   auto-reset, every env teacher-forced against the oracle at every step (tests/shadow.py; the
   oracle's wind path is pinned to the reference by tests/test_oracle_phases_wind.py).
3. test_env_shards_equal_single_handle_wind: two handles over env shards give one handle's bits.

Tolerances (f64 handle): teacher-forced step <= 1e-10 relative per channel with a 1e-3 floor,
theta_dot 1e-9 (tests/test_gpu_phases.py); gust filters <= 1e-12 absolute; info tap <= 1e-9 *
max(1, |ref|) (test_gpu_c3.py::test_info_tap_vs_oracle); mass flow <= 1e-15 of the largest;
shadowed runs: shadow.check_stats as it stands.

The in-band start of the free-running tests (BAND_Y, BAND_V): the initial states of pc, ba and
fl lie at 30, 50 and 34 km, above the 15 km gust ceiling, so before the first step the even envs
of these phases are put at 10 000 m.  At the initial speeds (1 046 and 1 045 m/s) that altitude
alone ends every such pc and ba episode at its first step (dynamic pressure: rtd_rl.py's q > 65 kPa
of pc, q > 8 kPa with a large effective angle of attack of ba; oracle alone: 35 resets of the 35
even envs at step 0, at 8, 10 and 12 km alike), after which the env is back above the band; so the
velocity of these envs is scaled as well, by 0.25 (pc) and 0.15 (ba), direction kept.  With the
oracle alone (orc_reset_philox + orc_step, the same seeds and actions, 70 envs x 48 steps) the
even envs then stay within pc 8 692..9 975 m, ba 10 013..10 505 m, fl 10 090..14 411 m (from
12 km the flip-over envs leave the band: 16 412 m), none of them resets, and the gust-step counts
are pc 1680, ba 1680, fl 1680, sub 3360, sup 3360 of 3360 env-steps; resets sub 1608 (the random-action
subsonic episodes end after two steps), sup 21; profiles seen sub 49, sup 45.

Measured on an MI355X (the tests print these at every run).  Teacher-forced against the
reference, largest over the five lanes-per-env values: state pc 4.7e-12, ba 2.8e-12, fl 7.1e-15,
sub 7.4e-13, sup 5.6e-12 (theta_dot everywhere but fl; every other channel <= 1.3e-12); filters
<= 4.4e-16; gusts, wind forces and moment <= 4.3e-15 of max(1, |ref|).  With C_gust_y = 1 against
the oracle: state <= 4.6e-12.  Shadowed: theta_dot pc 1.0e-10, ba 4.4e-12, fl 6.9e-15, sub
6.2e-15, sup 8.6e-13 (bound 1e-8), every other channel <= 2.3e-13, reward <= 1.8e-15, observation
and filters 0; gust steps pc 1680, ba 1680, fl 1680, sub 3360, sup 3360 of 3360; resets sub 1608,
sup 21; profiles pc 36, ba 36, fl 38, sub 49, sup 45: the oracle-only figures above.
"""
import math

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

ST = ["x", "y", "vx", "vy", "theta", "theta_dot", "gamma", "alpha", "mass", "mass_propellant", "time"]
TAGS = {"pc": "landing_burn_pure_throttle_Pcontrol", "ba": "ballistic_arc_descent", "fl": "flip_over_boostbackburn",
        "sub": "subsonic", "sup": "supersonic"}
ORC_PHASE = {"pc": 2, "ba": 3, "fl": 4, "sub": 5, "sup": 6}
BAND_Y = {"pc": 10000.0, "ba": 10000.0, "fl": 10000.0}
BAND_V = {"pc": 0.25, "ba": 0.15, "fl": 1.0}      # velocity scale of the in-band start (module docstring)
N_FREE, T_FREE, TILT = 70, 48, math.radians(1.0)


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


def rel_err(got, ref, floor=1e-3):
    return np.abs(got - ref) / np.maximum(np.abs(ref), floor)


def _teacher_forced_rows(pd, d, tag, lpe, rows, f32, stoch):
    """One physics-mode handle over `rows` of the fixture (all float32 or all float64 actions);
    returns the largest errors (state per channel, filters, info)."""
    import torch
    g = lambda k: d[f"{tag}_{k}"][rows]
    names = list(d["info_names"])
    env = pd.PoweredDescentEnv(len(rows), TAGS[tag], mode="physics", action_f64=not f32, lanes_per_env=lpe,
                               enable_wind=True, stochastic_wind=stoch)
    env.set_state(torch.tensor(g("state_in")))
    prev = g("prev").astype(np.float32).astype(np.float64) if f32 else g("prev")
    if tag == "fl":
        env.set_actuators(torch.tensor(np.stack([prev, 0 * prev, 0 * prev], 1)))
    env.set_wind_state(filters=g("filt_in"), sigmas=g("sigma"), percentile=g("percentile").astype(np.int64))
    a = torch.tensor(g("action"), dtype=torch.float32 if f32 else torch.float64)
    obs, r, dn, tr, ex = env.step(a, noise=torch.tensor(g("normals")), info=True)
    ctx = (tag, lpe, "f32" if f32 else "f64", "stochastic" if stoch else "profile only")
    SO = g("state_out")
    err = rel_err(env.state.cpu().numpy(), SO).max(0)
    tol = np.full(11, 1e-10); tol[5] = 1e-9
    assert (err < tol).all(), (ctx, dict(zip(ST, err)))
    filt, sig, pct = (v.cpu().numpy() for v in env.wind_state())
    e_filt = float(np.abs(filt - g("filt_out")).max())
    assert e_filt <= 1e-12, (ctx, e_filt)
    assert np.array_equal(sig, g("sigma")) and np.array_equal(pct, g("percentile").astype(np.int64)), ctx
    info = g("info")
    mass = SO[:, 8]       # rockets_physics.py:660-661 divide by the mass after its update (:642)
    refs = {"ug": g("gust")[:, 0], "vg": g("gust")[:, 1],
            "F_wind_x": info[:, names.index("acceleration_x_component_wind")] * mass,
            "F_wind_y": info[:, names.index("acceleration_y_component_wind")] * mass,
            "M_wind_z": info[:, names.index("M_wind_z")]}
    e_info = 0.0
    for k, ref in refs.items():
        e = np.abs(ex[k].cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))
        e_info = max(e_info, float(e.max()))
        assert e.max() <= 1e-9, (ctx, k, int(e.argmax()), e.max())
    md = ex["mass_flow"].cpu().numpy()
    ref_md = info[:, names.index("mass_flow")]
    assert np.abs(md - ref_md).max() <= 1e-15 * np.abs(ref_md).max(), (ctx, "mass flow")
    if tag == "fl":
        gd = env.actuators.cpu().numpy()[:, 0]
        assert np.array_equal(gd, info[:, names.index("gimbal_angle_deg")]), (ctx, "flip-over gimbal low-pass")
    assert not dn.any() and not tr.any() and float(r.abs().max()) == 0.0   # physics mode
    assert env.counters()["nan_events"] == 0
    return err, e_filt, e_info


@pytest.mark.parametrize("lpe", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("tag", list(TAGS))
def test_teacher_forced_wind_vs_reference(pd, tag, lpe):
    """compile_physics(0.1, phase) with a WindModel per row: the 50 float32-action rows and the 50
    float64-action rows of the fixture's stochastic-wind rows on two handles (50 envs: the last
    wave is ragged at every lanes-per-env value); at lanes_per_env = 2 also the 20 rows with the
    profile alone on stochastic_wind=False handles."""
    d = golden("ref_phases_wind.npz")
    F, stoch = d[f"{tag}_f32"], d[f"{tag}_stoch"]
    worst = [np.zeros(11), 0.0, 0.0]
    for st in ((True, False) if lpe == 2 else (True,)):
        for f32 in (True, False):
            rows = np.nonzero((F == f32) & (stoch == st))[0]
            assert len(rows) == (50 if st else 10)
            err, ef, ei = _teacher_forced_rows(pd, d, tag, lpe, rows, f32, st)
            worst = [np.maximum(worst[0], err), max(worst[1], ef), max(worst[2], ei)]
    print(f"wind teacher-forced {tag} lpe {lpe}: state {worst[0].max():.2e} (theta_dot {worst[0][5]:.2e}, others "
          f"{np.delete(worst[0], 5).max():.2e}), filters {worst[1]:.2e}, wind info {worst[2]:.2e}")


@pytest.mark.parametrize("lpe", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("tag", list(TAGS))
def test_vertical_gust_force_and_moment_arm(pd, oracle_mod, tag, lpe):
    """The reference's C_gust_y is 0.0 (size_gust_coefficients.py:21), so in every number of its
    own F_wind_y and M_wind_z vanish and the test above cannot see which centre of pressure the
    kernel puts into M_wind_z = -d_cp_cg * F_wind_y (rockets_physics.py:512), nor how F_wind_y
    joins the force sum.  Handles with C_gust_y = 1 on the fixture's in-band stochastic rows:
    the info tap's d_cp_cg against the reference's recorded one, F_wind_y against 0.5 rho vg^2 A
    of the recorded density and gust, M_wind_z against -(recorded d_cp_cg) * F_wind_y, and the
    next state against the oracle with the same C_gust_y (tests/test_oracle_phases_wind.py holds
    the oracle's arm to the same recorded d_cp_cg)."""
    import ctypes as C
    import torch
    O = oracle_mod
    d = golden("ref_phases_wind.npz")
    names = list(d["info_names"])
    prm = pd.Params()
    prm.struct.C_gust_y = 1.0
    o = O.Oracle(phase=ORC_PHASE[tag], rtd=O.RTD_NONE, wind=True, stochastic=True)
    o.slotted = 1
    o.P.C_gust_y = 1.0
    worst = np.zeros(11)
    for f32 in (True, False):
        rows = np.nonzero((d[f"{tag}_f32"] == f32) & d[f"{tag}_stoch"] & (d[f"{tag}_state_in"][:, 1] < 15000))[0]
        assert len(rows) >= 20
        g = lambda k: d[f"{tag}_{k}"][rows]
        env = pd.PoweredDescentEnv(len(rows), TAGS[tag], mode="physics", action_f64=not f32, lanes_per_env=lpe,
                                   enable_wind=True, stochastic_wind=True, params=prm)
        env.set_state(torch.tensor(g("state_in")))
        prev = g("prev").astype(np.float32).astype(np.float64) if f32 else g("prev")
        if tag == "fl":
            env.set_actuators(torch.tensor(np.stack([prev, 0 * prev, 0 * prev], 1)))
        env.set_wind_state(filters=g("filt_in"), sigmas=g("sigma"), percentile=g("percentile").astype(np.int64))
        a = torch.tensor(g("action"), dtype=torch.float32 if f32 else torch.float64)
        _, _, _, _, ex = env.step(a, noise=torch.tensor(g("normals")), info=True)
        ctx = (tag, lpe, "f32" if f32 else "f64")
        info = g("info")
        arm = info[:, names.index("d_cp_cg")]
        want_f = 0.5 * info[:, names.index("air_density")] * g("gust")[:, 1] ** 2 * prm.struct.frontal_area
        fwy = ex["F_wind_y"].cpu().numpy()
        assert (want_f > 0).all()
        for k, got, ref in (("d_cp_cg", ex["d_cp_cg"].cpu().numpy(), arm), ("F_wind_y", fwy, want_f),
                            ("M_wind_z", ex["M_wind_z"].cpu().numpy(), -arm * fwy)):
            e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
            assert e.max() <= 1e-9, (ctx, k, int(e.argmax()), e.max())
        S = env.state.cpu().numpy()
        for j, i in enumerate(rows):
            o.su, o.sv = (float(v) for v in g("sigma")[j])
            o.reset(g("state_in")[j])
            o.E.wind_prof = int(g("percentile")[j]) - 50
            o.E.fu[0], o.E.fu[1], o.E.fv[0], o.E.fv[1] = (float(v) for v in g("filt_in")[j])
            o.E.gimbal_prev = float(prev[j])
            av = g("action")[j].astype(np.float32).astype(np.float64) if f32 else g("action")[j]
            ua = (C.c_double * 4)(*list(av) + [0.0] * (4 - len(av)))
            nz = (C.c_double * 8)(*[float(v) for v in g("normals")[j]])
            O.lib().orc_physics(C.byref(o.P), C.byref(o.E), ORC_PHASE[tag], ua, int(f32), nz, None)
            worst = np.maximum(worst, rel_err(S[j], np.array(o.E.s[:])))
    tol = np.full(11, 1e-10); tol[5] = 1e-9
    assert (worst < tol).all(), (tag, lpe, dict(zip(ST, worst)))
    assert env.counters()["nan_events"] == 0
    print(f"wind C_gust_y=1 {tag} lpe {lpe}: state vs oracle {worst.max():.2e}")


def free_actions(tag, T, N):
    """Random float32 actions in the ranges of test_gpu_phases.py::test_batch_vs_oracle_rl."""
    rng = np.random.default_rng(40 + ORC_PHASE[tag])
    A = 2 if tag in ("sub", "sup") else 1
    acts = rng.uniform(-1, 1, (T, N, A))
    if tag == "pc":
        acts = rng.uniform(0, 1100, (T, N, A))
    if tag == "sub":
        acts[..., 1] = rng.uniform(0.5, 1, (T, N))
    return acts.astype(np.float32)


def free_env(pd, tag, n, seed, **kw):
    """The phase's free-running windy handle: wind profile of a percentile drawn per reset, von
    Karman gusts, tilt, auto-reset; the even (global) envs of pc, ba and fl start inside the gust
    band."""
    import torch
    env = pd.PoweredDescentEnv(n, TAGS[tag], mode="physics" if tag == "fl" else "rl", enable_wind=True,
                               stochastic_wind=True, wind_percentile=None, auto_reset=True, tilt_sigma_rad=TILT,
                               seed=seed, discount_factor=0.99, trajectory_length=100, **kw)
    if tag in BAND_Y:
        S = env.state
        even = (torch.arange(n, device=S.device) + int(kw.get("env_offset", 0))) % 2 == 0
        S[even, 1] = BAND_Y[tag]
        S[even, 2:4] *= BAND_V[tag]
        env.set_state(S)
        # the g-load history starts from the new speed (base_environment.py:137-141 takes |v| of
        # the previous state: the jump from the initial speed would read as 80 g and end pc)
        env.set_gload_window(torch.hypot(S[:, 2], S[:, 3]), torch.zeros(n, 10), torch.zeros(n))
    return env


@pytest.mark.parametrize("tag", list(TAGS))
def test_free_running_wind_shadowed(pd, oracle_mod, tag):
    """70 envs (16 lanes per env: a ragged last workgroup) x 48 steps with the device's own Philox
    draws, every env teacher-forced against the oracle at every step: state, reward, flags,
    observation, gust filters, and every auto-reset bit for bit (sigmas, percentile, tilt)."""
    import torch
    from shadow import shadow_run, check_stats
    N, T, seed = N_FREE, T_FREE, 300 + ORC_PHASE[tag]
    env = free_env(pd, tag, N, seed)
    A = torch.tensor(free_actions(tag, T, N)).cuda()
    st = shadow_run(oracle_mod, env, A, np.arange(N), ORC_PHASE[tag], 2 if tag == "fl" else 0, seed, TILT)
    print(f"wind shadow {tag}:", dict(max_err=[float(f"{v:.2e}") for v in st["max_err"]], rew=st["max_rew"],
                                      obs=st["max_obs"], filt=st["max_filt"], gust_steps=st["gust_steps"],
                                      resets=st["resets"], profiles=len(st["profiles"]),
                                      trunc_ids=sorted(st["trunc_ids"])))
    check_stats(st)
    assert st["steps"] == N * T
    assert st["gust_steps"] >= N * T // 4, st["gust_steps"]
    if tag in ("sub", "sup"):
        assert st["resets"] >= N // 4, st["resets"]
        assert len(st["profiles"]) >= 10, sorted(st["profiles"])
    if tag in BAND_Y:      # the even envs stayed inside the band, so their gust draws acted throughout
        y = env.state[0::2, 1].cpu().numpy()
        assert ((y > 0) & (y < 15000)).all(), y
    assert env.counters()["nan_events"] == 0


@pytest.mark.parametrize("tag", list(TAGS))
def test_env_shards_equal_single_handle_wind(pd, tag):
    """Two handles of 35 envs with env_offset 0 and 35 reproduce one handle of 70 bit for bit over
    16 windy steps (the Philox streams depend on the global env index only)."""
    import torch
    N, T, seed = N_FREE, 16, 500 + ORC_PHASE[tag]
    half = N // 2
    A = torch.tensor(free_actions(tag, T, N)).cuda()
    whole = free_env(pd, tag, N, seed)
    shards = [free_env(pd, tag, half, seed, env_offset=r * half) for r in range(2)]
    cat = lambda f: torch.cat([f(s) for s in shards], dim=0)
    assert torch.equal(whole.state, cat(lambda s: s.state))
    for t in range(T):
        o, r, dn, tr, ex = whole.step(A[t])
        parts = [s.step(A[t, k * half:(k + 1) * half]) for k, s in enumerate(shards)]
        for j, got in enumerate((o, r, dn, tr)):
            assert torch.equal(got, torch.cat([p[j] for p in parts])), (tag, t, j)
        assert torch.equal(ex["trunc_id"], torch.cat([p[4]["trunc_id"] for p in parts])), (tag, t)
        assert torch.equal(whole.state, cat(lambda s: s.state)), (tag, t)
    for k in range(3):
        assert torch.equal(whole.wind_state()[k], cat(lambda s: s.wind_state()[k])), (tag, k)
    f, sg, pr = whole.wind_state()
    assert bool((f != 0).any()) and len(set(pr.cpu().tolist())) >= 10     # gusts drawn, many profiles
