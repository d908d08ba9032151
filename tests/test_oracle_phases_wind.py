"""CPU oracle vs the reference WITH WIND for the flight phases besides the two landing burns:
landing_burn_pure_throttle_Pcontrol, ballistic_arc_descent, flip_over_boostbackburn, subsonic and
supersonic.  The reference turns wind on by default for every phase (base_environment.py:16-18);
tests/golden/ref_phases.npz is windless throughout and ref_wind_episodes.npz covers only the
landing burns.

Pinned by tests/golden/ref_phases_wind.npz (make_golden.py phases_wind, made by importing the
reference):
  * 120 teacher-forced compile_physics steps per phase with a fresh WindModel per row: half the
    rows inside the gust band (y < 15 km), at least 20 above it; rows 0..99 with stochastic wind
    (percentiles 50, 57.0, 75, 88.0, 99, injected sigmas, N(0, 1) filter pre-states, injected
    normals), rows 100..119 with the profile alone (vy_vk the int 0);
  * one windy rl_wrapped_env_pytorch episode for each phase the RL wrapper can step.

Bounds: those of tests/test_oracle_phases.py (state 1e-10 relative, theta_dot 1e-9, mass flow and
the atmosphere 1e-14, CL/CD 1e-9; episodes: state 1e-9, reward 1e-10 (1.0 floor), flags exact,
observation 1e-12); gust filters 1e-12 absolute (shadow.check_stats' tol_filt); the wind
accelerations, M_wind_z, ug and vg 1e-9 * max(1, |ref|) (test_gpu_c3.py::test_info_tap_vs_oracle).

Measured (this fixture): the state's largest relative error per phase is pc 2.6e-12, ba 5.0e-12,
fl 0 (bit-equal: the flip-over zeroes the aerodynamics, so no RBF solve enters), sub 2.3e-12,
sup 2.8e-11, theta_dot in every phase; every other channel <= 1.0e-12; filters <= 4.4e-16, wind
accelerations, M_wind_z, ug and vg <= 3.4e-16 of max(1, |ref|); the episodes consume 0 (pc, 163
steps; ba, 300 steps: neither comes below 15 km), 262 (sub) and 122 (sup) normals.

The reference's C_gust_y is 0.0 (size_gust_coefficients.py:21, "not used"): F_wind_y and M_wind_z
are 0 in every number the reference can produce, whatever the gust vg.  The fixture therefore
also records the reference's d_cp_cg, and test_wind_moment_arm_is_the_references holds the oracle's
M_wind_z to it with the oracle's own C_gust_y set to 1.

Sensitivity, each tried on a scratch copy of oracle/pd_oracle.c and committed nowhere:
  1. the promotion line of the binary32 force sum taken in its wind-off form,
     `fx = (double)(sx + (float)Fwx)`: test_teacher_forced_physics_wind fails for sub (largest
     state error 9.2e-7, on alpha; vx 2.3e-8 at the first row) and sup (1.7e-6, on alpha), and the
     sub and sup episodes fail at their first step (4.4e-8 and 2.3e-10 on vx); pc, ba and fl have
     no binary32 force sum and stay as above;
  2. M_wind_z with the descent centre of pressure in the ascent phases (`-(x_cog - P->cop) *
     Fwy`): against the reference's own numbers nothing changes (its F_wind_y is 0, above);
     test_wind_moment_arm_is_the_references fails for sub and sup (M_wind_z off by 1.7 of its
     value; with C_gust_y = 1 theta_dot moves by 6.2e-4 and 9.2e-5 relative).
"""
import os

import numpy as np
import pytest

import oracle as O
from test_oracle_phases import augment, rel

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "ref_phases_wind.npz"))
TAGS = {"pc": O.PCONTROL, "ba": O.BALLISTIC, "fl": O.FLIP, "sub": O.SUBSONIC, "sup": O.SUPERSONIC}
EP_TAGS = {k: v for k, v in TAGS.items() if k != "fl"}
INFO = list(Z["info_names"])


def test_fixture_covers_the_gust_band():
    """What make_golden.py asserts when it writes the fixture, on the committed file."""
    for tag in TAGS:
        y, st, n = Z[f"{tag}_state_in"][:, 1], Z[f"{tag}_stoch"], Z[f"{tag}_n_normals"]
        assert int((y < 14500).sum()) >= 60 and int((y > 15000).sum()) >= 20, tag
        assert (n[(y < 15000) & st] == 2).all(), tag      # one filter step of u and v per physics call
        assert (n[(y >= 15000) | ~st] == 0).all(), tag
        assert int(st.sum()) == 100 and len(st) == 120
        assert set(Z[f"{tag}_percentile"]) == {50.0, 57.0, 75.0, 88.0, 99.0}
    assert Z["ep_sub_n_normals_cum"][-1] > 0 and Z["ep_sup_n_normals_cum"][-1] > 0


@pytest.mark.parametrize("tag", list(TAGS))
def test_teacher_forced_physics_wind(tag):
    """compile_physics(0.1, phase) with the row's WindModel: next state, normals consumed, filter
    states, wind accelerations and moment, gusts, mass flow."""
    g = lambda k: Z[f"{tag}_{k}"]
    S, A, F, PV, SO = g("state_in"), g("action"), g("f32"), g("prev"), g("state_out")
    worst = dict(state=np.zeros(11), filt=0.0, wind=0.0)
    orcs = {}
    for i in range(len(S)):
        f32, stoch, pct = bool(F[i]), bool(g("stoch")[i]), int(g("percentile")[i])
        if (stoch, pct) not in orcs:
            orcs[stoch, pct] = O.Oracle(phase=TAGS[tag], rtd=O.RTD_NONE, wind=True, stochastic=stoch,
                                        wind_percentile=pct)
            orcs[stoch, pct].slotted = 1
        o = orcs[stoch, pct]
        o.su, o.sv = (float(v) for v in g("sigma")[i])
        o.reset(S[i])
        fi = g("filt_in")[i]
        o.E.fu[0], o.E.fu[1], o.E.fv[0], o.E.fv[1] = (float(v) for v in fi)
        prev = float(np.float32(PV[i])) if f32 else float(PV[i])
        o.E.gimbal_prev = prev
        a = A[i].astype(np.float32).astype(np.float64) if f32 else A[i]
        ua = (O.D * 4)(*list(a) + [0.0] * (4 - len(a)))
        nz = (O.D * 8)(*[float(v) for v in g("normals")[i]])
        info = (O.D * len(O.INFO_NAMES))()
        O.lib().orc_physics(O.C.byref(o.P), O.C.byref(o.E), TAGS[tag], ua, int(f32), nz, info)
        info = dict(zip(O.INFO_NAMES, info[:]), **O.wind_info())
        ctx = (tag, i)
        e = rel(np.array(o.E.s[:]), SO[i])
        worst["state"] = np.maximum(worst["state"], e)
        assert e[5] < 1e-9 and np.delete(e, 5).max() < 1e-10, (ctx, e)
        assert o.noise_used == int(g("n_normals")[i]), (ctx, o.noise_used)
        fo = np.array([o.E.fu[0], o.E.fu[1], o.E.fv[0], o.E.fv[1]])
        ef = float(np.abs(fo - g("filt_out")[i]).max())
        worst["filt"] = max(worst["filt"], ef)
        assert ef <= 1e-12, (ctx, ef)
        ref = dict(zip(INFO, g("info")[i]))
        ref["ug"], ref["vg"] = g("gust")[i]
        for k in ("acceleration_x_component_wind", "acceleration_y_component_wind", "M_wind_z", "ug", "vg"):
            ew = abs(info[k] - ref[k]) / max(1.0, abs(ref[k]))
            worst["wind"] = max(worst["wind"], ew)
            assert ew <= 1e-9, (ctx, k, info[k], ref[k])
        names = ["mass_flow", "air_density", "mach_number", "gimbal_angle_deg"]
        ei = rel(np.array([info[k] for k in names]), np.array([ref[k] for k in names]))
        assert ei.max() < 1e-14, (ctx, dict(zip(names, ei)))    # mass flow bit-level incl. f32 islands
        ec = rel(np.array([info["CL"], info["CD"]]), np.array([ref["CL"], ref["CD"]]))
        assert ec.max() < 1e-9, (ctx, "CL/CD", ec)               # RBF solve order
    print(f"wind teacher-forced {tag}: state {worst['state'].max():.2e} (theta_dot {worst['state'][5]:.2e}, "
          f"others {np.delete(worst['state'], 5).max():.2e}), filters {worst['filt']:.2e}, wind info {worst['wind']:.2e}")


@pytest.mark.parametrize("tag", list(TAGS))
def test_wind_moment_arm_is_the_references(tag):
    """The reference's C_gust_y is 0.0 (size_gust_coefficients.py:21, "not used"), so its F_wind_y
    and M_wind_z are 0 in every row above and no number of the reference's can tell which centre of
    pressure the oracle puts into M_wind_z = -d_cp_cg * F_wind_y (rockets_physics.py:512).  With
    the oracle's C_gust_y set to 1, on the in-band stochastic rows: M_wind_z must equal
    -(the reference's recorded d_cp_cg of the row) * (the oracle's own F_wind_y), and F_wind_y must
    equal 0.5 rho vg^2 A with the reference's recorded density and gust."""
    g = lambda k: Z[f"{tag}_{k}"]
    rows = np.nonzero(g("stoch") & (g("state_in")[:, 1] < 15000))[0]
    assert len(rows) >= 50
    o = O.Oracle(phase=TAGS[tag], rtd=O.RTD_NONE, wind=True, stochastic=True, wind_percentile=50)
    o.slotted = 1
    o.P.C_gust_y = 1.0
    worst = 0.0
    for i in rows:
        f32 = bool(g("f32")[i])
        o.su, o.sv = (float(v) for v in g("sigma")[i])
        o.reset(g("state_in")[i])
        o.E.fu[0], o.E.fu[1], o.E.fv[0], o.E.fv[1] = (float(v) for v in g("filt_in")[i])
        o.E.gimbal_prev = float(np.float32(g("prev")[i])) if f32 else float(g("prev")[i])
        a = g("action")[i].astype(np.float32).astype(np.float64) if f32 else g("action")[i]
        ua = (O.D * 4)(*list(a) + [0.0] * (4 - len(a)))
        nz = (O.D * 8)(*[float(v) for v in g("normals")[i]])
        info = (O.D * len(O.INFO_NAMES))()
        O.lib().orc_physics(O.C.byref(o.P), O.C.byref(o.E), TAGS[tag], ua, int(f32), nz, info)
        info = dict(zip(O.INFO_NAMES, info[:]), **O.wind_info())
        ref = dict(zip(INFO, g("info")[i]))
        fwy = info["acceleration_y_component_wind"] * o.E.s[8]
        want_f = 0.5 * ref["air_density"] * g("gust")[i, 1] ** 2 * o.P.A_front
        assert want_f > 0 and abs(fwy - want_f) <= 1e-9 * max(1.0, want_f), (tag, i, fwy, want_f)
        want_m = -ref["d_cp_cg"] * fwy
        e = abs(info["M_wind_z"] - want_m) / max(1.0, abs(want_m))
        worst = max(worst, e)
        assert e <= 1e-9, (tag, i, info["M_wind_z"], want_m)
    print(f"wind moment arm {tag}: {worst:.2e}")


@pytest.mark.parametrize("tag", list(EP_TAGS))
def test_teacher_forced_rl_episodes_wind(tag):
    """A windy rl_wrapped_env_pytorch episode (percentile 50, stochastic gusts with the recorded
    normal stream): each step starts from the reference's previous state and g-load window, the
    oracle's gust filters run free over the whole episode and take the stream's next normals;
    every step's state, reward, done/truncated/id, observation and running normal count."""
    p = f"ep_{tag}_"
    S, R, Dn, T, TI, OB, A, CUM = (Z[p + n] for n in ("state", "reward", "done", "trunc", "trunc_id", "obs", "actions",
                                                      "n_normals_cum"))
    su, sv = Z[p + "sigma"]
    o = O.Oracle(phase=EP_TAGS[tag], rtd=O.RTD_RL, wind=True, stochastic=True, sigma_u=su, sigma_v=sv,
                 wind_percentile=50, discount_factor=0.99, trajectory_length=100)
    normals = np.concatenate([Z[p + "normals"], np.zeros(8)])
    allS = np.vstack([np.array(o.P.state0_ph[EP_TAGS[tag]][:])[None], S])
    v = np.hypot(allS[:, 2], allS[:, 3])
    gl = np.abs(np.diff(v)) / 0.1 / 9.81
    k = 0
    for t in range(len(R)):
        o.E.s[:] = list(allS[t]); o.E.prev_s[:] = list(allS[t])
        win = gl[max(0, t - 9):t]
        for i, gv in enumerate(win):
            o.E.gwin[i] = gv
        o.E.gwin_len = len(win)
        u, f32 = augment(tag, A[t], o.P.speed0_pc)
        s, r, d, tr, tid, ob, info = o.step(u, f32=f32, noise=normals[k:k + 8])
        k += o.noise_used
        assert k == int(CUM[t]), (tag, t, k, int(CUM[t]))
        assert rel(s, S[t]).max() < 1e-9, (tag, t, rel(s, S[t]))
        assert abs(r - R[t]) <= 1e-10 * max(1.0, abs(R[t])), (tag, t, r, R[t])
        assert (d, tr, tid) == (bool(Dn[t]), bool(T[t]), int(TI[t])), (tag, t)
        assert np.abs(ob - OB[t]).max() < 1e-12, (tag, t, ob, OB[t])
    assert k == len(Z[p + "normals"])
