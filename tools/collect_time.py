#!/usr/bin/env python3
"""Times the SAC collection's two paths on the same actor and replay ring: SACCollector.collect(K)
(pd_collect_sac: K steps per call, the actor inside the step kernel's fused-step loop) against K
SACCollector.step() calls (pd_step_sac_fused: one launch per step), for K in 1, 8, 32, 128.

4 096 envs, landing_burn_pure_throttle, no wind, binary64, auto_reset on (the collection loop
resets an env at its episode's end, sac_pytorch_powered_descent.py:160-183: every timed step runs
on envs inside an episode), a stochastic 2 x 256 actor (torch-initialised, seed 0),
DevicePrioritizedReplayBuffer(1 000 000) in ring mode.  First collect(K_CHECK) on one collector is
compared bit for bit with K_CHECK step() calls on a twin: the ring's rows, the priorities, the
ring state, obs and the handle checkpoint (K_CHECK 240, the most the ring takes in one call: the
JSON records how many envs crossed an in-kernel reset in it).  Then, per K, each timed
window is STEPS / K rounds of collect(K), or of K step() calls, between two device synchronisations
(host clock; STEPS = 8 192 steps of all envs, a few tenths of a second); the two paths alternate
within each of REPEATS rounds after a warm-up round; the JSON holds the median and the min/max over
the rounds in ms per step of all envs.
  python tools/collect_time.py [out.json]      (default profiles/sac_collect.json)
Environment: N, REPEATS, STEPS, K_CHECK."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))

KS = (1, 8, 32, 128)


def main():
    import torch
    import pdenv
    from pdenv import _lib as L
    from pdenv.sac import Actor, DevicePrioritizedReplayBuffer, SACCollector
    if not torch.cuda.is_available():
        sys.exit("collect_time.py measures on the GPU: no HIP device visible")
    N = int(os.environ.get("N", 4096))
    repeats, steps = int(os.environ.get("REPEATS", 7)), int(os.environ.get("STEPS", 8192))
    k_check = int(os.environ.get("K_CHECK", 240))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "sac_collect.json")
    capacity = 1_000_000
    torch.manual_seed(0)
    actor = Actor(2, 1, hidden_dim=256, n_hidden_layers=2).cuda()

    def collector():
        env = pdenv.PoweredDescentEnv(N, flight_phase="landing_burn_pure_throttle", mode="rl", precision="f64", seed=1,
                                      auto_reset=True)
        return SACCollector(env, actor, DevicePrioritizedReplayBuffer(capacity, env.obs_dim, env.action_dim, env.device))

    c, twin = collector(), collector()
    dev = c.obs.device
    assert c.ring and c.kernel is not None, "the collector is not in ring mode with the kernel's actor"
    launched = []
    real = c.env.collect_sac
    c.env.collect_sac = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
    ep0 = c.env.episode_counters()[0].clone()
    rows = c.collect(k_check)
    resets = c.env.episode_counters()[0] - ep0            # in-kernel resets of the checked call, per env
    want = torch.cat([twin.step().clone() for _ in range(k_check)])
    assert launched, "collect() did not call pd_collect_sac"
    c.env.collect_sac = real

    def checkpoint(env):
        # (a zeroed blob: pd_checkpoint_save leaves the padding between the per-env buffers unwritten)
        blob = torch.zeros(int(env.lib.pd_checkpoint_size(env.h)), dtype=torch.uint8, device=env.device)
        L.check(env.lib.pd_checkpoint_save(env.h, blob.data_ptr(), torch.cuda.current_stream(env.device).cuda_stream))
        return blob

    def same(x, y):
        return x.dtype == y.dtype and x.shape == y.shape and bool(torch.equal(x.view(torch.uint8), y.view(torch.uint8)))

    checks = {"rows": same(rows, want), "buffer": same(c.buffer.data, twin.buffer.data),
              "priorities": same(c.buffer.priorities, twin.buffer.priorities),
              "ring_state": c.buffer.state_dev.tolist() == twin.buffer.state_dev.tolist() == [c.buffer.position, c.buffer.size, 0],
              "obs": same(c.obs, twin.obs), "checkpoint": same(checkpoint(c.env), checkpoint(twin.env))}
    equal = all(checks.values())

    def fused(k):
        c.collect(k)

    def per_step(k):
        for _ in range(k):
            c.step()

    paths = {"collect": fused, "per_step": per_step}
    times = {k: {name: [] for name in paths} for k in KS}
    for rnd in range(repeats + 1):                  # round 0: warm-up, not kept
        for k in KS:
            inner = max(1, steps // k)
            for name, fn in paths.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn(k)
                torch.cuda.synchronize(dev)
                if rnd:
                    times[k][name].append((time.perf_counter() - t0) * 1e3 / (inner * k))
    ep1 = c.env.episode_counters()[0]
    res = {"n_envs": N, "actor": "2x256 stochastic", "precision": "f64", "wind": False, "auto_reset": True,
           "buffer_capacity": capacity,
           "ring_mode": True, "step_fuse": c.env.tuning()["step_fuse"], "repeats": repeats, "steps_per_window": steps,
           "checked_steps": k_check, "outputs_equal_bitwise": bool(equal), "checks": checks,
           "checked_envs_crossing_a_reset": int((resets >= 1).sum()), "checked_resets_per_env_max": int(resets.max()),
           "episodes_per_env_in_the_run": [int((ep1 - ep0).min()), int((ep1 - ep0).max())],
           "unit": "ms per step of all envs", "K": {}}
    for k in KS:
        row = {}
        for name, ts in times[k].items():
            row[name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts),
                         "window_ms": statistics.median(ts) * max(1, steps // k) * k}
        row["speedup_median"] = row["per_step"]["median"] / row["collect"]["median"]
        row["collect_max_below_per_step_min"] = row["collect"]["max"] < row["per_step"]["min"]
        res["K"][str(k)] = row
    res["speed_claim_holds_at_K32"] = res["K"]["32"]["collect_max_below_per_step_min"]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not equal:
        sys.exit(f"collect({k_check}) and {k_check} step() calls differ: {checks}")


if __name__ == "__main__":
    main()
