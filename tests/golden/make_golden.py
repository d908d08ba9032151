#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ (build container only).

Two kinds of fixtures, both plain data (npz):

1. recorded_*.npz -- columns lifted from the reference's OWN recorded runs
   (data/reference_trajectory, data/agent_saves/PyTorchSAC, data/pso_saves):
   the de-facto golden data of the reference.
2. ref_*.npz -- produced by importing the reference (/root/reference, read-only)
   and running its own functions on seeded inputs.  The reference needs two
   absent third-party packages; tests/golden/shims provides `ambiance` (ISA
   restated, pinned by the recorded atmosphere columns) and a `gymnasium`
   annotation stub.  `dill.load` is replaced BEFORE the reference is imported:
   the reference's rocket_functions.pkl is never unpickled.  Instead the closures
   are rebuilt from the reference's own stage_inertia / d_cg_thrusters / cop_func
   with the constants tools/make_param_pack.py read statically from the pickle.

Nothing here ships to the GPU box: only the .npz outputs are committed.
Run:  python tests/golden/make_golden.py
"""
import contextlib
import io
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PDENV_REFERENCE", "/root/reference")
PACK = os.path.join(REPO, "psso-sac-for-powered-descent_amd", "data", "param_pack.json")
STATE_COLS = ["x", "y", "vx", "vy", "theta", "theta_dot", "gamma", "alpha", "mass", "mass_propellant", "time"]


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"  {name}: " + ", ".join(f"{k}{tuple(np.shape(v))}" for k, v in arrays.items()), file=sys.stderr)


# --------------------------------------------------------------------------- recorded data
def recorded():
    import pandas as pd
    d = pd.read_csv(os.path.join(REF, "data/reference_trajectory/landing_burn_controls_pure_throttle/"
                                      "state_action_landing_burn_pure_throttle_control.csv"))
    cols = ["x[m]", "y[m]", "vx[m/s]", "vy[m/s]", "theta[rad]", "theta_dot[rad/s]", "gamma[rad]",
            "alpha[rad]", "mass[kg]", "masspropellant[kg]", "time[s]"]
    save("recorded_reference_trajectory.npz", state=d[cols].values, u0=d["u0"].values)

    root = os.path.join(REF, "data/agent_saves/PyTorchSAC/LandingBurnPureThrottle")
    runs = sorted(r for r in os.listdir(root) if os.path.exists(os.path.join(root, r, "trajectories/trajectory.csv")))
    keep = ["air_density", "atmospheric_pressure", "speed_of_sound", "CD", "CL", "mach_number",
            "mass_flow", "dynamic_pressure", "x_cog", "inertia", "d_thrust_cg", "alpha_effective",
            "g_load_1_sec_window", "control_force_parallel", "throttle"]
    out = {}
    for k, r in enumerate(runs[:4]):
        t = pd.read_csv(os.path.join(root, r, "trajectories/trajectory.csv"))
        out[f"run{k}_state"] = t[STATE_COLS].values
        out[f"run{k}_action"] = t["action"].values.astype(np.float64)
        out[f"run{k}_info"] = t[keep].values
    out["info_names"] = np.array(keep)
    out["runs"] = np.array(runs[:4])
    save("recorded_sac_trajectories.npz", **out)

    p = os.path.join(REF, "data/pso_saves/landing_burn_pure_throttle/Landed/trajectory_data")
    tr = pd.read_csv(os.path.join(p, "trajectory.csv"))
    ac = pd.read_csv(os.path.join(p, "actions.csv"))
    rw = pd.read_csv(os.path.join(p, "rewards.csv"))
    info = pd.read_csv(os.path.join(p, "info_data.csv"))
    cols2 = ["x[m]", "y[m]", "vx[m/s]", "vy[m/s]", "theta[rad]", "theta_dot[rad/s]", "gamma[rad]",
             "alpha[rad]", "mass[kg]", "mass_propellant[kg]", "time[s]"]
    save("recorded_pso_landed.npz", state=tr[cols2].values, action=ac.values[:, 0].astype(np.float64),
         reward=rw.values[:, 0], mass_flow=info["mass_flow"].values, air_density=info["air_density"].values,
         CD=info["CD"].values, CL=info["CL"].values)


# --------------------------------------------------------------------------- reference import
def import_reference():
    sys.path[:0] = [os.path.join(HERE, "shims"), REF]
    os.chdir(REF)
    pack = json.load(open(PACK))
    import dill

    def _no_unpickle(_f, *a, **k):
        from src.RocketSizing.functions.rocket_dimensions import stage_inertia, d_cg_thrusters, full_rocket_inertia
        from src.RocketSizing.functions.cop_estimation import cop_func
        c = pack["inertia"]
        inert = stage_inertia(h_ox=c["h_ox"], h_f=c["h_f"], m_ox=c["m_ox"], m_f=c["m_f"],
                              h_lower=c["h_lower"], m_dry=c["m_dry"], x_dry=c["x_dry"], I_dry=c["I_dry"])
        L = pack["sizing"]["stage_1_height"]
        fr = pack["phases"]["ascent_inertia"]
        full = full_rocket_inertia(m_s_1=np.float64(fr["m_s_1"]), x_dry_1=np.float64(fr["x_dry_1"]),
                                   I_dry_1=np.float64(fr["I_dry_1"]), m_2=np.float64(fr["m_2"]), m_pay=fr["m_pay"],
                                   x_wet_2_initial=np.float64(fr["x_wet_2_initial"]),
                                   I_wet_2_initial=np.float64(fr["I_wet_2_initial"]), h_1=np.float64(fr["h_1"]),
                                   h_1_ox=np.float64(fr["h_1_ox"]), h_1_f=np.float64(fr["h_1_f"]),
                                   m_1_ox=np.float64(fr["m_1_ox"]), m_1_f=np.float64(fr["m_1_f"]),
                                   h_lower_1=np.float64(fr["h_lower_1"]))
        L0 = pack["phases"]["cop_ascent"] / 0.25
        return {"x_cog_inertia_subrocket_2_lambda": inert,
                "d_cg_thrusters_subrocket_2_lambda": lambda x: d_cg_thrusters(x, c["engine_height"]),
                "cop_subrocket_2_lambda": lambda alpha, M: cop_func(L, alpha, M, d_0=0.75),
                "x_cog_inertia_subrocket_0_lambda": full,
                "d_cg_thrusters_subrocket_0_lambda": lambda x: d_cg_thrusters(x, c["engine_height"]),
                "cop_subrocket_0_lambda": lambda alpha, M: cop_func(L0, alpha, M, d_0=0.25),
                "cop_subrocket_1_lambda": None}

    dill.load = _no_unpickle
    with contextlib.redirect_stdout(io.StringIO()):
        import src.envs.rockets_physics as rp
        from src.envs.utils import acs_model, atmosphere_dynamics
        from src.envs.rl.env_wrapped_rl_pytorch import rl_wrapped_env_pytorch
        from src.envs.pso.env_wrapped_ea import pso_wrapper, pso_wrapped_env
    import_reference.pso_wrapped_env = pso_wrapped_env
    return rp, acs_model, atmosphere_dynamics, rl_wrapped_env_pytorch, pso_wrapper


def kats(rp, acs_model, atm):
    rng = np.random.default_rng(1234)
    # rocket_CD(M, aoa_deg): clamps at +-radians(10) in "degree" units
    M = np.concatenate([np.linspace(0.0, 10.0, 101), rng.uniform(0, 4, 400)])
    Acd = np.concatenate([np.linspace(-0.2, 0.2, 41), rng.uniform(-0.2, 0.2, 60)])
    cd_q = np.array([(m, a) for m in M[::5] for a in Acd[::4]] + [(m, a) for m, a in zip(rng.uniform(0, 4, 300), rng.uniform(-0.2, 0.2, 300))])
    cd_v = np.array([rp.rocket_CD(m, a) for m, a in cd_q])
    # rocket_CL(M, x): x is converted to degrees once more inside
    Xcl = np.concatenate([np.linspace(-0.25, 0.25, 51), rng.uniform(-0.2, 0.2, 80), np.radians([1e-7, 2.0, 10.0, 11.0])])
    cl_q = np.array([(m, x) for m in M[::5] for x in Xcl[::3]] + [(m, x) for m, x in zip(rng.uniform(0, 4, 300), rng.uniform(-0.2, 0.2, 300))])
    cl_v = np.array([rp.rocket_CL(m, x) for m, x in cl_q])
    ca_q = np.concatenate([np.linspace(0, 5, 201), rng.uniform(0, 4, 100)])
    ca_v = np.array([float(acs_model.Ca_func(m)) for m in ca_q])
    cn_q = np.stack([np.concatenate([np.linspace(0, 5, 101), rng.uniform(0, 4, 100)]),
                     rng.uniform(-0.3, 0.3, 201)], 1)
    cn_v = np.array([float(acs_model.Cn_func(m, a)) for m, a in cn_q])
    alt = np.concatenate([np.linspace(-100, 90000, 3000), [0, 11000, 20000, 32000, 47000, 51000, 71000, 80000, 81019.9, 81020]])
    isa = np.array([atm.endo_atmospheric_model(h) for h in alt])
    grav = np.array([atm.gravity_model_endo(h) for h in alt])
    save("ref_kat.npz", cd_q=cd_q, cd_v=cd_v, cl_q=cl_q, cl_v=cl_v, ca_q=ca_q, ca_v=ca_v,
         cn_q=cn_q, cn_v=cn_v, alt=alt, isa=isa, grav=grav)


def sample_states(rng, n):
    sac = np.load(os.path.join(HERE, "recorded_sac_trajectories.npz"))
    ref = np.load(os.path.join(HERE, "recorded_reference_trajectory.npz"))["state"]
    pool = np.concatenate([sac[f"run{k}_state"] for k in range(4)] + [ref])
    pool = pool[pool[:, 1] > 5.0]
    return pool[rng.choice(len(pool), n, replace=False)]


def teacher_forced(rp):
    rng = np.random.default_rng(99)
    step_pt = rp.compile_physics(0.1, "landing_burn_pure_throttle")
    step_lb = rp.compile_physics(0.1, "landing_burn")
    S = sample_states(rng, 600)
    out = {}
    for tag, fn, A in (("pt", step_pt, 1), ("lb", step_lb, 4)):
        acts = rng.uniform(-1, 1, (len(S), A)).astype(np.float32)
        prevs = np.stack([rng.uniform(-5, 5, len(S)), rng.uniform(-0.3, 0.3, len(S)), rng.uniform(-0.3, 0.3, len(S))], 1)
        res, info_keep = [], []
        for i in range(len(S)):
            st = [np.float64(v) for v in S[i]]
            with contextlib.redirect_stdout(io.StringIO()):
                if A == 1:
                    s2, info = fn(st, acts[i], wind_generator=None)
                else:
                    s2, info = fn(st, acts[i], prevs[i, 0], prevs[i, 1], prevs[i, 2], wind_generator=None)
            res.append([float(v) for v in s2])
            ai = info["action_info"]
            info_keep.append([info["air_density"], info["mach_number"], info["CL"], info["CD"],
                              float(info["mass_flow"]), info["dynamic_pressure"], info["x_cog"], info["inertia"],
                              float(ai.get("gimbal_angle_deg", 0.0)), float(ai.get("delta_command_left_rad", 0.0)),
                              float(ai.get("delta_command_right_rad", 0.0))])
        out[f"{tag}_state_in"] = S
        out[f"{tag}_action"] = acts
        out[f"{tag}_prevs"] = prevs
        out[f"{tag}_state_out"] = np.array(res)
        out[f"{tag}_info"] = np.array(info_keep)
    out["info_names"] = np.array(["air_density", "mach_number", "CL", "CD", "mass_flow", "dynamic_pressure",
                                  "x_cog", "inertia", "gimbal_angle_deg", "delta_command_left_rad",
                                  "delta_command_right_rad"])
    save("ref_teacher_forced.npz", **out)


def run_episode(env, actions, max_steps, obs_of_step):
    rec = {k: [] for k in ("state", "reward", "done", "trunc", "trunc_id", "obs")}
    with contextlib.redirect_stdout(io.StringIO()):
        env.reset()
        for k in range(max_steps):
            obs, r, d, tr, info = obs_of_step(env, actions[k])
            rec["state"].append([float(v) for v in info["state"]])
            rec["reward"].append(float(r)); rec["done"].append(bool(d)); rec["trunc"].append(bool(tr))
            rec["trunc_id"].append(int(env.truncation_id() if callable(getattr(env, "truncation_id", None)) else env.env.truncation_id))
            rec["obs"].append(np.asarray(obs, dtype=np.float64).ravel().tolist())
            if d or tr:
                break
    return {k: np.array(v) for k, v in rec.items()}


def episodes(rl_env_cls, pso_wrapper_cls):
    ref_u0 = np.load(os.path.join(HERE, "recorded_reference_trajectory.npz"))["u0"]
    out = {}
    # (a) SAC wrapper, pure throttle, the SAC driver's configuration (sac_pytorch_powered_descent.py:22-28)
    with contextlib.redirect_stdout(io.StringIO()):
        env = rl_env_cls(flight_phase="landing_burn_pure_throttle", enable_wind=False, stochastic_wind=False,
                         trajectory_length=1, discount_factor=0.99)
    sac_step = lambda e, a: e.step(a)
    seqs = {
        "rl_land": ref_u0.astype(np.float32)[:, None],              # the classical controller's throttle, as f32
        "rl_rand0": np.random.default_rng(7).uniform(-1, 1, (2200, 1)).astype(np.float32),
        "rl_rand1": np.random.default_rng(8).uniform(0.2, 1, (2200, 1)).astype(np.float32),
        "rl_hi": np.full((2200, 1), 0.95, np.float32),
    }
    for name, acts in seqs.items():
        ep = run_episode(env, acts, min(2200, len(acts)), sac_step)
        for k, v in ep.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_actions"] = acts[:len(ep["reward"])]
    # (b) PSO wrapper, pure throttle and landing_burn (env_wrapped_ea.py:77-134)
    import torch
    pso_step = lambda e, a: e.step(torch.tensor(a))
    with contextlib.redirect_stdout(io.StringIO()):
        pt = pso_wrapper_cls(flight_phase="landing_burn_pure_throttle", enable_wind=False, stochastic_wind=False,
                             horiontal_wind_percentile=50)
        lb = pso_wrapper_cls(flight_phase="landing_burn", enable_wind=False, stochastic_wind=False,
                             horiontal_wind_percentile=50)
    seqs = {
        ("pso_pt_land", pt): ref_u0.astype(np.float32)[:, None],
        ("pso_pt_rand", pt): np.random.default_rng(11).uniform(-1, 1, (2200, 1)).astype(np.float32),
        ("pso_lb_rand0", lb): np.random.default_rng(12).uniform(-1, 1, (2200, 4)).astype(np.float32),
        ("pso_lb_rand1", lb): np.concatenate([np.random.default_rng(13).uniform(-0.2, 0.2, (2200, 1)),
                                              np.random.default_rng(14).uniform(0.3, 1.0, (2200, 1)),
                                              np.random.default_rng(15).uniform(-0.3, 0.3, (2200, 2))], 1).astype(np.float32),
    }
    for (name, env), acts in seqs.items():
        ep = run_episode(env, acts, 2200, pso_step)
        for k, v in ep.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_actions"] = acts[:len(ep["reward"])]
    save("ref_episodes.npz", **out)


def wind_episodes(rl_env_cls):
    """Stochastic wind with an INJECTED noise stream: vonkarman.py draws np.random.randn()
    per filter step and random.uniform per reset; both are replaced by recorded streams."""
    out = {}
    ref_u0 = np.load(os.path.join(HERE, "recorded_reference_trajectory.npz"))["u0"]
    for ep_i, seed in enumerate((21, 22)):
        rng = np.random.default_rng(seed)
        normals = rng.standard_normal(2200 * 8)
        uniforms = [0.5 + (2.25 - 0.5) * rng.random(), 1.25 + (2.0 - 1.25) * rng.random()]
        state = {"n": 0, "u": 0}
        orig_randn, orig_uniform = np.random.randn, random.uniform

        def fake_randn(*a):
            v = normals[state["n"]]; state["n"] += 1
            return v

        def fake_uniform(a, b):
            if state["u"] < 2:
                v = uniforms[state["u"]]
            else:
                v = a + (b - a) * 0.5
            state["u"] += 1
            return v

        np.random.randn, random.uniform = fake_randn, fake_uniform
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                env = rl_env_cls(flight_phase="landing_burn_pure_throttle", enable_wind=True, stochastic_wind=True,
                                 horiontal_wind_percentile=50, trajectory_length=1, discount_factor=0.99)
                state["n"] = 0; state["u"] = 0
                # reset() draws the per-episode sigmas (VKDisturbanceGenerator._new_filters)
                acts = ref_u0.astype(np.float32)[:, None] if ep_i == 0 else np.full((2200, 1), 0.9, np.float32)
                ep = run_episode(env, acts, min(2200, len(acts)), lambda e, a: e.step(a))
                su = env.env.wind_generator.von_karman_generator_class.sigma_u
                sv = env.env.wind_generator.von_karman_generator_class.sigma_v
        finally:
            np.random.randn, random.uniform = orig_randn, orig_uniform
        for k, v in ep.items():
            out[f"w{ep_i}_{k}"] = v
        out[f"w{ep_i}_actions"] = acts[:len(ep["reward"])]
        out[f"w{ep_i}_normals"] = normals[:state["n"]]
        out[f"w{ep_i}_sigma"] = np.array([su, sv])
    save("ref_wind_episodes.npz", **out)


def pso_objective(pso_wrapped_env_cls):
    """pso_wrapped_env.objective_function (env_wrapped_ea.py:200-222) on seeded particles of both
    PSO phases: fitness, episode length, and per step the raw env state the actor saw and the
    float32 action it returned (teacher-forced check of the fused actor)."""
    import torch
    torch.manual_seed(0)
    out = {}
    for tag, phase in (("pt", "landing_burn_pure_throttle"), ("lb", "landing_burn")):
        with contextlib.redirect_stdout(io.StringIO()):
            model = pso_wrapped_env_cls(flight_phase=phase, enable_wind=False, stochastic_wind=False,
                                        horiontal_wind_percentile=50)
        D = len(model.bounds)
        rng = np.random.default_rng(11)
        inds = np.concatenate([rng.uniform(-1.5, 1.5, (4, D)), rng.uniform(-0.5, 0.5, (4, D))])
        base = model.env.env
        fits, lens, states, acts, owner = [], [], [], [], []
        for k, ind in enumerate(inds):
            rec_s, rec_a = [], []
            orig = model.env.step

            def step(action, _orig=orig, _rs=rec_s, _ra=rec_a):
                _rs.append(np.array(base.state, dtype=np.float64))
                _ra.append(action.detach().numpy().astype(np.float32).reshape(-1))
                return _orig(action)
            model.env.step = step
            with contextlib.redirect_stdout(io.StringIO()):
                f = model.objective_function(ind)
            model.env.step = orig
            fits.append(f); lens.append(len(rec_a))
            states += rec_s; acts += rec_a; owner += [k] * len(rec_a)
        out[f"{tag}_individuals"] = inds
        out[f"{tag}_fitness"] = np.array(fits)
        out[f"{tag}_length"] = np.array(lens)
        out[f"{tag}_states"] = np.array(states)
        out[f"{tag}_actions"] = np.array(acts)
        out[f"{tag}_owner"] = np.array(owner)
    save("ref_pso_objective.npz", **out)


PHASE_CSV = {   # recorded classical-controller runs of each phase (column names differ per file)
    "subsonic": "ascent_controls/subsonic_state_action_ascent_control.csv",
    "supersonic": "ascent_controls/supersonic_state_action_ascent_control.csv",
    "flip_over_boostbackburn": "flip_over_and_boostbackburn_controls/state_action_flip_over_and_boostbackburn_control.csv",
    "ballistic_arc_descent": "ballistic_arc_descent_controls/state_action_ballistic_arc_descent_control.csv",
    "landing_burn_pure_throttle_Pcontrol": "landing_burn_v_ref_control/state_action_landing_burn_pure_throttle_control.csv",
}
CSV_STATE = ["x[m]", "y[m]", "vx[m/s]", "vy[m/s]", "theta[rad]", "theta_dot[rad/s]", "gamma[rad]", "alpha[rad]",
             "mass[kg]", "mass_propellant[kg]", "time[s]"]


def phase_states(phase):
    import pandas as pd
    d = pd.read_csv(os.path.join(REF, "data/reference_trajectory", PHASE_CSV[phase]))
    d = d.rename(columns={"masspropellant[kg]": "mass_propellant[kg]"})
    return d[CSV_STATE].values, d


def recorded_phases():
    """The reference's recorded classical-controller runs of the flip-over and both ascent
    phases (data/reference_trajectory/*), replayed open-loop by the oracle test."""
    out = {}
    for tag, phase, ucols in (("fl", "flip_over_boostbackburn", ["u0"]), ("sub", "subsonic", ["u0", "u1"]),
                              ("sup", "supersonic", ["u0", "u1"])):
        S, d = phase_states(phase)
        out[f"{tag}_state"] = S
        out[f"{tag}_u"] = d[ucols].values
    save("recorded_phases.npz", **out)


def phases(rp, rl_env_cls):
    """The flight phases besides the two landing burns:
    teacher-forced compile_physics steps with float32 and float64 actions from states of the
    reference's recorded runs of each phase, RL-wrapper episodes, and the phase/type pairs the
    reference itself cannot step (recorded as the exception they raise)."""
    rng = np.random.default_rng(2024)
    out = {}
    for tag, phase, A in (("pc", "landing_burn_pure_throttle_Pcontrol", 1), ("ba", "ballistic_arc_descent", 1),
                          ("fl", "flip_over_boostbackburn", 1), ("sub", "subsonic", 2), ("sup", "supersonic", 2)):
        fn = rp.compile_physics(0.1, phase)
        pool, _ = phase_states(phase)
        S = pool[rng.choice(len(pool), 300, replace=len(pool) < 300)]
        if phase == "landing_burn_pure_throttle_Pcontrol":
            acts = rng.uniform(0, 1100, (len(S), A))
        else:
            acts = rng.uniform(-1, 1, (len(S), A))
        f32 = np.arange(len(S)) % 2 == 0            # even rows: float32 actions, odd: float64
        prev = rng.uniform(-10, 10, len(S))
        res, inf = [], []
        for i in range(len(S)):
            st = [np.float64(v) for v in S[i]]
            a = acts[i].astype(np.float32) if f32[i] else acts[i].astype(np.float64)
            with contextlib.redirect_stdout(io.StringIO()):
                if phase == "flip_over_boostbackburn":
                    g = np.array([prev[i]], dtype=np.float32 if f32[i] else np.float64)
                    s2, info = fn(st, a, g, wind_generator=None)
                else:
                    s2, info = fn(st, a, wind_generator=None)
            res.append([float(v) for v in s2])
            ai = info["action_info"]
            inf.append([info["air_density"], info["mach_number"], info["CL"], info["CD"], float(info["mass_flow"]),
                        info["dynamic_pressure"], info["x_cog"], info["inertia"],
                        float(np.asarray(ai.get("gimbal_angle_deg", 0.0)).ravel()[0])])
        out[f"{tag}_state_in"] = S
        out[f"{tag}_action"] = acts
        out[f"{tag}_f32"] = f32
        out[f"{tag}_prev"] = prev
        out[f"{tag}_state_out"] = np.array(res)
        out[f"{tag}_info"] = np.array(inf)
    out["info_names"] = np.array(["air_density", "mach_number", "CL", "CD", "mass_flow", "dynamic_pressure",
                                  "x_cog", "inertia", "gimbal_angle_deg"])
    # RL-wrapper episodes (float32 policy actions, env_wrapped_rl_pytorch.step)
    specs = [("lb", "landing_burn", 4, [(31, 0.3), (32, 0.05)]),
             ("pc", "landing_burn_pure_throttle_Pcontrol", 1, [(33, 1.0), (34, 0.2)]),
             ("ba", "ballistic_arc_descent", 1, [(35, 1.0), (36, 0.1)]),
             ("sub", "subsonic", 2, [(37, 1.0), (38, 0.05)]),
             ("sup", "supersonic", 2, [(39, 1.0), (40, 0.05)])]
    for tag, phase, A, seeds in specs:
        with contextlib.redirect_stdout(io.StringIO()):
            env = rl_env_cls(flight_phase=phase, enable_wind=False, stochastic_wind=False,
                             trajectory_length=100, discount_factor=0.99)
        for k, (seed, scale) in enumerate(seeds):
            r = np.random.default_rng(seed)
            acts = (r.uniform(-1, 1, (2500, A)) * scale).astype(np.float32)
            if phase == "landing_burn_pure_throttle_Pcontrol":
                acts = r.uniform(-1, 1, (2500, A)).astype(np.float32) * np.float32(scale)
            if phase == "subsonic":      # the ascent needs throttle to leave the pad
                acts[:, 1] = np.clip(acts[:, 1] + np.float32(0.9), -1, 1)
            ep = run_episode(env, acts, 2500, lambda e, a: e.step(a))
            for key, v in ep.items():
                out[f"ep_{tag}{k}_{key}"] = v
            out[f"ep_{tag}{k}_actions"] = acts[:len(ep["reward"])]
    # pairs the reference cannot step: record the exception type
    raised = []
    for phase, typ in (("landing_burn_ACS", "rl"), ("flip_over_boostbackburn", "rl")):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                env = rl_env_cls(flight_phase=phase, enable_wind=False, stochastic_wind=False,
                                 trajectory_length=100, discount_factor=0.99)
                env.reset()
                env.step(np.zeros(env.action_dim, dtype=np.float32))
            raised.append(f"{phase}/{typ}: none")
        except Exception as e:   # noqa: BLE001 (recording what the reference does)
            raised.append(f"{phase}/{typ}: {type(e).__name__}")
    out["raises"] = np.array(raised)
    save("ref_phases.npz", **out)


@contextlib.contextmanager
def injected_noise(normals, uniforms):
    """np.random.randn (one per von Karman filter step, vonkarman.py:34) and random.uniform (the
    sigmas of _new_filters, vonkarman.py:62-63) replaced by recorded streams; yields the counters
    {"n": normals consumed, "u": uniforms consumed}.  Uniforms past the given ones: the midpoint."""
    cnt = {"n": 0, "u": 0}
    orig_randn, orig_uniform = np.random.randn, random.uniform

    def fake_randn(*a):
        v = normals[cnt["n"]]; cnt["n"] += 1
        return v

    def fake_uniform(a, b):
        v = uniforms[cnt["u"]] if cnt["u"] < len(uniforms) else a + (b - a) * 0.5
        cnt["u"] += 1
        return v

    np.random.randn, random.uniform = fake_randn, fake_uniform
    try:
        yield cnt
    finally:
        np.random.randn, random.uniform = orig_randn, orig_uniform


WIND_INFO = ["acceleration_x_component_wind", "acceleration_y_component_wind", "M_wind_z", "mass_flow",
             "air_density", "mach_number", "CL", "CD", "gimbal_angle_deg", "d_cp_cg"]


def phases_wind(rp, rl_env_cls):
    """Wind (full_wind_model.WindModel: percentile profile + von Karman gusts below 15 km) on the
    five phases besides the two landing burns, which phases() and wind_episodes() leave out.

    (a) 120 teacher-forced compile_physics steps per phase from states of the phase's recorded
    run: rows with i % 4 < 2 get an altitude U(300, 14 500) m inside the gust band, the others keep
    theirs (at least 20 of them above the 15 km ceiling, placed at U(15 500, 40 000) m where the
    recorded run has too few).  Rows 0..99: stochastic wind, a fresh WindModel per row with the
    percentile cycling over ints and floats, injected sigmas, N(0, 1) filter pre-states and 8
    injected normals; rows 100..119: the same with stochastic_wind=False.
    (b) one windy rl_wrapped_env_pytorch episode per RL-steppable phase (noise injected as in
    wind_episodes, actions of phases()' second spec), at most 300 steps."""
    from src.envs.wind.full_wind_model import WindModel
    out = {}
    pcts = [50, 57.0, 75, 88.0, 99]      # wrappers pass an int, WindModel draws float(randint)
    n_rows, n_stoch = 120, 100
    for k, (tag, phase, A) in enumerate((("pc", "landing_burn_pure_throttle_Pcontrol", 1),
                                         ("ba", "ballistic_arc_descent", 1), ("fl", "flip_over_boostbackburn", 1),
                                         ("sub", "subsonic", 2), ("sup", "supersonic", 2))):
        rng = np.random.default_rng(3100 + k)
        fn = rp.compile_physics(0.1, phase)
        pool, _ = phase_states(phase)
        S = pool[rng.choice(len(pool), n_rows, replace=len(pool) < n_rows)].copy()
        band = np.arange(n_rows) % 4 < 2
        S[band, 1] = rng.uniform(300.0, 14500.0, int(band.sum()))
        keep = np.nonzero(~band)[0]
        lows = keep[S[keep, 1] <= 15000.0]
        need = 20 - (len(keep) - len(lows))
        if need > 0:
            place = lows[np.linspace(0, len(lows) - 1, need).astype(int)]
            S[place, 1] = rng.uniform(15500.0, 40000.0, need)
        assert int((S[band, 1] < 14500.0).sum()) == n_rows // 2, tag
        assert int((S[~band, 1] > 15000.0).sum()) >= 20, tag
        assert int((S[:n_stoch][~band[:n_stoch], 1] > 15000.0).sum()) >= 10, tag
        if phase == "landing_burn_pure_throttle_Pcontrol":
            acts = rng.uniform(0, 1100, (n_rows, A))
        else:
            acts = rng.uniform(-1, 1, (n_rows, A))
        f32 = np.arange(n_rows) % 2 == 0            # even rows: float32 actions, odd: float64
        prev = rng.uniform(-10, 10, n_rows)
        stoch = np.arange(n_rows) < n_stoch
        pct = np.array([float(pcts[i % 5]) for i in range(n_rows)])
        sigma = np.stack([0.5 + (2.25 - 0.5) * rng.random(n_rows), 1.25 + (2.0 - 1.25) * rng.random(n_rows)], 1)
        filt_in = rng.standard_normal((n_rows, 4))
        normals = rng.standard_normal((n_rows, 8))
        res, inf, filt_out, gust, used = [], [], [], [], []
        for i in range(n_rows):
            st = [np.float64(v) for v in S[i]]
            a = acts[i].astype(np.float32) if f32[i] else acts[i].astype(np.float64)
            with injected_noise(normals[i], list(sigma[i])) as cnt, contextlib.redirect_stdout(io.StringIO()):
                wg = WindModel(0.1, stochastic_wind=bool(stoch[i]), given_percentile=pcts[i % 5])
                vk = wg.von_karman_generator_class
                assert (vk.sigma_u, vk.sigma_v) == tuple(sigma[i]) and cnt["u"] == 2
                vk.u_filter.state = filt_in[i, :2].copy()
                vk.v_filter.state = filt_in[i, 2:].copy()
                if phase == "flip_over_boostbackburn":
                    g = np.array([prev[i]], dtype=np.float32 if f32[i] else np.float64)
                    s2, info = fn(st, a, g, wind_generator=wg)
                else:
                    s2, info = fn(st, a, wind_generator=wg)
            in_band = S[i, 1] < 15000.0
            assert (cnt["n"] > 0) if (in_band and stoch[i]) else (cnt["n"] == 0), (tag, i, cnt["n"])
            used.append(cnt["n"])
            res.append([float(v) for v in s2])
            filt_out.append(np.concatenate([vk.u_filter.state, vk.v_filter.state]))
            gust.append([float(wg.vx_vals[-1]), float(wg.uy_vals[-1])])
            acc, mom, ai = info["acceleration_dict"], info["moment_dict"], info["action_info"]
            inf.append([float(acc["acceleration_x_component_wind"]), float(acc["acceleration_y_component_wind"]),
                        float(mom["M_wind_z"]), float(info["mass_flow"]), info["air_density"], info["mach_number"],
                        info["CL"], info["CD"], float(np.asarray(ai.get("gimbal_angle_deg", 0.0)).ravel()[0]),
                        float(info["d_cp_cg"])])
        out[f"{tag}_state_in"] = S
        out[f"{tag}_action"] = acts
        out[f"{tag}_f32"] = f32
        out[f"{tag}_prev"] = prev
        out[f"{tag}_stoch"] = stoch
        out[f"{tag}_percentile"] = pct
        out[f"{tag}_sigma"] = sigma
        out[f"{tag}_filt_in"] = filt_in
        out[f"{tag}_normals"] = normals
        out[f"{tag}_n_normals"] = np.array(used)
        out[f"{tag}_state_out"] = np.array(res)
        out[f"{tag}_filt_out"] = np.array(filt_out)
        out[f"{tag}_gust"] = np.array(gust)
        out[f"{tag}_info"] = np.array(inf)
    out["info_names"] = np.array(WIND_INFO)
    # (b) windy RL-wrapper episodes: the second spec of phases() (seed, scale)
    max_steps = 300
    for tag, phase, A, seed, scale in (("pc", "landing_burn_pure_throttle_Pcontrol", 1, 34, 0.2),
                                       ("ba", "ballistic_arc_descent", 1, 36, 0.1), ("sub", "subsonic", 2, 38, 0.05),
                                       ("sup", "supersonic", 2, 40, 0.05)):
        r = np.random.default_rng(seed)
        acts = (r.uniform(-1, 1, (2500, A)) * scale).astype(np.float32)
        if phase == "landing_burn_pure_throttle_Pcontrol":
            acts = r.uniform(-1, 1, (2500, A)).astype(np.float32) * np.float32(scale)
        if phase == "subsonic":      # the ascent needs throttle to leave the pad
            acts[:, 1] = np.clip(acts[:, 1] + np.float32(0.9), -1, 1)
        rng = np.random.default_rng(500 + seed)
        normals = rng.standard_normal(max_steps * 8)
        uniforms = [0.5 + (2.25 - 0.5) * rng.random(), 1.25 + (2.0 - 1.25) * rng.random()]
        cum = []
        with injected_noise(normals, uniforms) as cnt, contextlib.redirect_stdout(io.StringIO()):
            env = rl_env_cls(flight_phase=phase, enable_wind=True, stochastic_wind=True,
                             horiontal_wind_percentile=50, trajectory_length=100, discount_factor=0.99)
            cnt["n"] = 0; cnt["u"] = 0
            # reset() draws the per-episode sigmas (VKDisturbanceGenerator._new_filters)

            def step(e, a):
                res = e.step(a)
                cum.append(cnt["n"])
                return res
            ep = run_episode(env, acts, max_steps, step)
            vk = env.env.wind_generator.von_karman_generator_class
            su, sv = vk.sigma_u, vk.sigma_v
            used = cnt["n"]
        assert (su, sv) == tuple(uniforms), tag
        for key, v in ep.items():
            out[f"ep_{tag}_{key}"] = v
        out[f"ep_{tag}_actions"] = acts[:len(ep["reward"])]
        out[f"ep_{tag}_normals"] = normals[:used]
        out[f"ep_{tag}_sigma"] = np.array([su, sv])
        out[f"ep_{tag}_n_normals_cum"] = np.array(cum)
    save("ref_phases_wind.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "ref_phases_wind.npz"))
    assert size <= os.path.getsize(os.path.join(HERE, "ref_phases.npz")), size


def wind_profiles_ref():
    """HorizontalWindSpeed.compile_horizontal_fixed_wind for every percentile the envs use
    (WindModel: float(np.random.randint(50, 99)); the wrappers' horiontal_wind_percentile, an
    int, 50..99), at altitudes across and beyond each profile: a 0..50 km grid, every profile
    node and its neighbours 1 m either side, and negative altitudes."""
    os.chdir(REF)
    sys.path[:0] = [os.path.join(HERE, "shims"), REF]
    with contextlib.redirect_stdout(io.StringIO()):
        from src.envs.wind.HorizontalWindSpeed import compile_horizontal_fixed_wind, extract_horizontal_wind_data
        wd, _ = extract_horizontal_wind_data()
    nodes = np.unique(np.concatenate([v["altitude_km"] for v in wd.values()])) * 1000.0
    y = np.unique(np.concatenate([np.linspace(0.0, 50000.0, 401), nodes, nodes - 1.0, nodes + 1.0,
                                  [-500.0, -1.0, 60000.0, 1e6]]))
    pct = np.arange(50, 100)
    speed = np.empty((len(pct), len(y)))
    for i, p in enumerate(pct):
        f = compile_horizontal_fixed_wind(float(p))
        speed[i] = [float(f(v)) for v in y]
    save("ref_wind_profiles.npz", percentile=pct, y=y, speed=speed)


def main():
    print("recorded fixtures", file=sys.stderr)
    recorded()
    print("importing the reference (shims: ambiance, gymnasium; dill.load replaced)", file=sys.stderr)
    rp, acs_model, atm, rl_env_cls, pso_wrapper_cls = import_reference()
    print("KATs", file=sys.stderr); kats(rp, acs_model, atm)
    print("teacher-forced steps", file=sys.stderr); teacher_forced(rp)
    print("episodes", file=sys.stderr); episodes(rl_env_cls, pso_wrapper_cls)
    print("wind episodes", file=sys.stderr); wind_episodes(rl_env_cls)
    print("PSO objective", file=sys.stderr); pso_objective(import_reference.pso_wrapped_env)
    print("other phases", file=sys.stderr); recorded_phases(); phases(rp, rl_env_cls)
    print("other phases with wind", file=sys.stderr); phases_wind(rp, rl_env_cls)
    print("wind profiles", file=sys.stderr); wind_profiles_ref()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pso":     # only the PSO-objective fixture
        _, _, _, _, _ = import_reference()
        pso_objective(import_reference.pso_wrapped_env)
    elif len(sys.argv) > 1 and sys.argv[1] == "wind":     # only the wind-profile fixture
        wind_profiles_ref()
    elif len(sys.argv) > 1 and sys.argv[1] == "phases":     # only the other-phases fixture
        recorded_phases()
        rp, _, _, rl_env_cls, _ = import_reference()
        phases(rp, rl_env_cls)
    elif len(sys.argv) > 1 and sys.argv[1] == "phases_wind":     # only the windy other-phases fixture
        rp, _, _, rl_env_cls, _ = import_reference()
        phases_wind(rp, rl_env_cls)
    else:
        main()
