#!/usr/bin/env python3
"""Times what logging the learning statistics costs a learner update, three ways in the same run:
  (a) `no_stats`    pdenv.sac.sac_update without stats (sample, TdTarget, CriticUpdate, ActorUpdate,
                    update_priorities on a KernelPrioritizedReplayBuffer: no host synchronisation)
  (b) `kernel`      the same with a LearningStats on the kernel: one pd_sac_learning_stats launch more
  (c) `torch_items` the same with LearningStats(kernel=False) -- the 37 numbers by float64 torch
                    reductions on the device -- plus the four .item() reads the reference makes per
                    update (critic_loss, actor_loss, alpha_loss, alpha: sac_pytorch.py:606-609)
each on its own learner from the same initial values.  (S, A) = (2, 1), hidden 256, two hidden layers
(the driver's defaults), PER and clipping on; batches 256 and 512.

Before a batch size is timed the kernel is checked there: the same pd_sac_learning_stats call twice
gives equal bytes, and its row agrees with the torch path's within the bound of
tests/test_gpu_learning_stats.py.

The protocol of tools/actor_update_time.py: each timed window is INNER updates between two device
synchronisations (host clock, one synchronisation at the end of the window only); the variants
alternate within each of REPEATS rounds after a warm-up round; the JSON holds the median and the
min / max over the rounds.  The rings hold more rows than a run records, so no flush falls into a
window of (b); (c) synchronises at every update by construction.
  python tools/learning_stats_time.py [out.json]      (default profiles/sac_learning_stats.json)
Environment: REPEATS, INNER, BATCHES (comma-separated)."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

S, A, H, NL = 2, 1, 256, 2
LR, TAU, MAX_NORM, GAMMA = 3e-4, 0.005, 1.0, 0.99


def learner(batch, slab):
    import numpy as np
    import torch
    from pdenv.sac import Actor, ActorUpdate, Critic, CriticUpdate, KernelPrioritizedReplayBuffer, TdTarget
    torch.manual_seed(0)
    actor, critic, target = Actor(S, A, H, NL).cuda(), Critic(S, A, H, NL).cuda(), Critic(S, A, H, NL).cuda()
    target.load_state_dict(critic.state_dict())
    la = torch.tensor([np.log(0.2)], dtype=torch.float32, device="cuda", requires_grad=True)
    buf = KernelPrioritizedReplayBuffer(slab.shape[0], S, A, torch.device("cuda"))
    buf.add_batch(slab)
    td = TdTarget(actor, target, la, GAMMA)
    cu = CriticUpdate(critic, target, torch.optim.Adam(critic.parameters(), lr=LR), tau=TAU, max_grad_norm=MAX_NORM)
    au = ActorUpdate(actor, critic, la, torch.optim.Adam(actor.parameters(), lr=LR), torch.optim.Adam([la], lr=LR),
                     max_grad_norm=MAX_NORM)
    assert td.kernel and cu.kernel and au.kernel
    return dict(buf=buf, td=td, cu=cu, au=au, la=la)


def check(batch, slab):
    """Equal bytes twice, and the kernel's row against the torch path's, after one real update."""
    import numpy as np
    import torch
    import learning_stats_ref as M
    from pdenv.sac import LearningStats, sac_update
    k = learner(batch, slab)
    dev = torch.device("cuda")
    rings = [LearningStats(S, A, dev, capacity=4), LearningStats(S, A, dev, capacity=4),
             LearningStats(S, A, dev, capacity=4, kernel=False)]
    sac_update(k["buf"], k["td"], k["cu"], k["au"], batch)
    rows, tq = k["buf"].last_rows, k["td"]._out[batch]
    lp, w = k["au"]._buffers(batch, rows.device)["log_prob"], k["buf"]._out[batch][1].reshape(-1, 1)
    for r in rings:
        r.record(rows, tq, k["cu"], k["au"], lp, w, k["buf"])
    assert rings[0].last_kernel and rings[1].last_kernel and not rings[2].last_kernel
    a, b, t = (r.rows[0] for r in rings)
    assert a.tobytes() == b.tobytes(), "the same call gave other bytes"
    scale = M.model_row(rows.cpu().numpy(), k["au"].q.cpu().numpy(), tq.cpu().numpy(), lp.cpu().numpy(), S, A,
                        weights=w.cpu().numpy(), scales=True)[1]
    assert M.same_number(a[M.MINMAX], t[M.MINMAX]) and M.same_bits(a[M.COPIED], t[M.COPIED])
    rel = np.abs(a[M.BOUNDED] - t[M.BOUNDED]) / np.abs(scale[M.BOUNDED])
    assert np.nanmax(rel) <= 2.0 ** -30, float(np.nanmax(rel))
    return dict(equal_bytes_twice=True, kernel_minus_torch_over_scale=float(np.nanmax(rel)))


def variants(batch, slab, rows_needed):
    import torch
    from pdenv.sac import LearningStats, sac_update
    dev = torch.device("cuda")
    a, b, c = learner(batch, slab), learner(batch, slab), learner(batch, slab)
    on_kernel = LearningStats(S, A, dev, capacity=rows_needed + 8)
    on_torch = LearningStats(S, A, dev, capacity=rows_needed + 8, kernel=False)

    def torch_items():
        sac_update(c["buf"], c["td"], c["cu"], c["au"], batch, stats=on_torch)
        return (c["cu"].critic_loss.item(), c["au"].actor_loss.item(), c["au"].alpha_loss.item(), c["la"].exp().item())

    return {"no_stats": lambda: sac_update(a["buf"], a["td"], a["cu"], a["au"], batch),
            "kernel": lambda: sac_update(b["buf"], b["td"], b["cu"], b["au"], batch, stats=on_kernel),
            "torch_items": torch_items}, on_kernel, on_torch


def timed(calls, repeats, inner):
    import torch
    times = {k: [] for k in calls}
    for rnd in range(repeats + 1):              # round 0: warm-up, not kept
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    return {name: {"ms": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)} for name, ts in times.items()}


def main():
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("learning_stats_time.py measures on the GPU: no HIP device visible")
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 50))
    batches = [int(x) for x in os.environ.get("BATCHES", "256,512").split(",")]
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "sac_learning_stats.json")
    res = {"block": "SACPyTorch.update's body (sac_pytorch.py:416-531) on the kernels, without and with the learning "
                    "statistics of _track_learning_stats (sac_pytorch.py:553-634)",
           "state_dim": S, "action_dim": A, "hidden": H, "hidden_layers": NL, "per": True, "clip": True,
           "repeats": repeats, "calls_per_window": inner, "shapes": []}
    for batch in batches:
        rng = np.random.default_rng(batch)
        slab = rng.standard_normal((4 * batch, 2 * S + A + 2)).astype(np.float32)
        slab[:, S:S + A] = np.tanh(slab[:, S:S + A])
        slab[:, -1] = np.arange(4 * batch) % 5 == 3
        slab = torch.from_numpy(slab).cuda()
        checks = check(batch, slab)
        calls, on_kernel, on_torch = variants(batch, slab, (repeats + 1) * inner)
        entry = {"batch": batch, "checks_passed": True, **checks, **timed(calls, repeats, inner)}
        assert on_kernel.last_kernel and not on_torch.last_kernel and on_kernel._flushed == 0
        entry["logging_cost_kernel_ms"] = entry["kernel"]["ms"] - entry["no_stats"]["ms"]
        entry["logging_cost_torch_items_ms"] = entry["torch_items"]["ms"] - entry["no_stats"]["ms"]
        entry["kernel_faster_than_torch_items"] = entry["kernel"]["ms"] < entry["torch_items"]["ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
