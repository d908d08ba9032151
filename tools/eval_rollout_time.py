#!/usr/bin/env python3
"""Times pdenv.sac.evaluate_agent's two paths on the same actor: the fused rollout
(pd_rollout_sac: the actor inside the step kernel's loop, one call) against the per-step path
built from the calls of the collection path (pd_step_sac_fused + pd_step per step, bookkeeping in
device tensors).  A third line, `per_step_bare`, is only the pd_step_sac_fused launches of the
longest episode -- no rewards, no bookkeeping: a lower bound for ANY per-step evaluation, not a
path that returns evaluate_agent's values.

4 096 envs, landing_burn_pure_throttle, no wind, binary64, a deterministic 2 x 256 actor
(torch-initialised, seed 0), max_steps 512.  Each timed window is INNER evaluations between two
device synchronisations (host clock); the paths alternate within each of REPEATS rounds after a
warm-up round; the JSON holds the median and the min/max over the rounds, so the spread is next to
every figure.  The paths' outputs are compared bit for bit first.
  python tools/eval_rollout_time.py [out.json]      (default profiles/eval_rollout.json)
Environment: N, REPEATS, INNER, MAX_STEPS."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))


def main():
    import torch
    import pdenv
    from pdenv.sac import Actor, ActorKernel, evaluate_agent
    if not torch.cuda.is_available():
        sys.exit("eval_rollout_time.py measures on the GPU: no HIP device visible")
    N = int(os.environ.get("N", 4096))
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 8))
    T = int(os.environ.get("MAX_STEPS", 512))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "eval_rollout.json")
    torch.manual_seed(0)
    actor = Actor(2, 1, hidden_dim=256, n_hidden_layers=2).cuda()
    env = pdenv.PoweredDescentEnv(N, flight_phase="landing_burn_pure_throttle", mode="rl", precision="f64", seed=1)
    kern = ActorKernel(actor)
    dev = env.device
    obs = torch.empty(N, 2, dtype=torch.float32, device=dev)
    act = torch.empty(N, 1, dtype=torch.float32, device=dev)
    slab = torch.empty(N, 7, dtype=torch.float32, device=dev)

    def fused():
        return evaluate_agent(actor, env, max_steps=T, fused=True)

    def per_step():
        return evaluate_agent(actor, env, max_steps=T, fused=False)

    ref = fused()
    assert ref.fused, "the handle does not take the fused rollout (lanes per env != 16?)"
    chk = per_step()
    equal = all(torch.equal(getattr(ref, k), getattr(chk, k)) for k in ("returns", "steps", "done", "trunc_id"))
    steps_max = int(ref.steps.max())

    def per_step_bare():
        obs.copy_(env.reset())
        for _ in range(steps_max):
            env.step_sac_fused(kern.S, kern.A, kern.H, kern.nl, kern.ptrs(), actor.log_std_min, actor.log_std_max,
                               actor.max_action, deterministic=True, ring=slab, action=act, obs32=obs)

    paths = {"fused": fused, "per_step": per_step, "per_step_bare": per_step_bare}
    times = {k: [] for k in paths}
    for rnd in range(repeats + 1):                  # round 0: warm-up, not kept
        for name, fn in paths.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize(dev)
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    env_steps = int(ref.steps.sum())
    res = {"n_envs": N, "max_steps": T, "actor": "2x256 deterministic", "precision": "f64", "wind": False,
           "repeats": repeats, "evaluations_per_window": inner, "outputs_equal_bitwise": bool(equal),
           "episode_length_mean": float(ref.steps.double().mean()), "episode_length_max": steps_max,
           "mean_reward": ref.mean_reward, "success_rate": ref.success_rate, "paths": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["paths"][name] = {"env_steps": env_steps, "wall_ms": med, "wall_ms_min": min(ts), "wall_ms_max": max(ts),
                              "ms_per_step_all_envs": med / steps_max,
                              "episode_length_mean": res["episode_length_mean"], "episode_length_max": steps_max,
                              "returns_evaluate_agent_values": name != "per_step_bare"}
    res["speedup_fused_vs_per_step"] = res["paths"]["per_step"]["wall_ms"] / res["paths"]["fused"]["wall_ms"]
    res["speedup_fused_vs_per_step_bare"] = res["paths"]["per_step_bare"]["wall_ms"] / res["paths"]["fused"]["wall_ms"]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
