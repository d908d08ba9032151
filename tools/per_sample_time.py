#!/usr/bin/env python3
"""Times one learner round trip on the prioritized replay buffer -- sample(B) followed by
update_priorities -- for both classes of pdenv.sac in the same run: DevicePrioritizedReplayBuffer
(the torch expression over the whole ring; its update reads the maximum back to the host) and
KernelPrioritizedReplayBuffer (pd_per_sample / pd_per_update, no read-back).

Ring sizes 32 768, 262 144 and 1 000 000 (the driver's), batches 256 and 512 (the driver's), rows of
the pure-throttle task (7 floats), log-uniform priorities 1e-6 .. 1e3, alpha 0.6.  Before a shape is
timed the kernel path is checked there: the same (seed, draw) twice gives equal bits in every
output, the keys are within 32 binary64 ulp of the NumPy model (tests/per_ref.py), the indices are
the model's (after asserting that the model's first B + 1 sorted keys are more than 1e-9 apart,
relatively), the weights within one float32 ulp, the rows the ring's.  The largest key error seen
and the bound are recorded.

Each timed window is INNER round trips between two device synchronisations (host clock, one
synchronisation at the end of the window only); the two classes alternate within each of REPEATS
rounds after a warm-up round; the JSON holds the median and the min / max over the rounds.
  python tools/per_sample_time.py [out.json]      (default profiles/per_sample.json)
Environment: REPEATS, INNER, SIZES, BATCHES (comma-separated)."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

SEED, ALPHA, S, A = 12345, 0.6, 2, 1


def check_shape(np, torch, per_ref, buf, pri_np, batch, draw):
    """The kernel path at one timed shape against itself and the model; returns the largest
    relative key error."""
    beta = buf.beta
    first = [t.clone() for t in buf.sample(batch, draw=draw, check=True, keys=True)]
    buf.beta = beta
    second = buf.sample(batch, draw=draw, check=True, keys=True)
    for x, y in zip(first, second):
        ints = torch.int64 if x.element_size() == 8 else torch.int32
        assert torch.equal(x.contiguous().view(ints), y.contiguous().view(ints)), "the same draw gave other bits"
    m_idx, m_w, m_keys, m_n, _ = per_ref.sample(pri_np, batch, ALPHA, beta, SEED, draw)
    keys = first[7].cpu().numpy()
    assert np.array_equal(np.isinf(keys), np.isinf(m_keys))
    fin = np.isfinite(m_keys)
    err = float(np.max(np.abs(keys[fin] - m_keys[fin]) / m_keys[fin]))
    assert err <= per_ref.KEY_BOUND, f"key error {err:.3e} above the bound {per_ref.KEY_BOUND:.3e}"
    gap = per_ref.min_gap(m_keys, batch)
    assert gap > 1e-9, f"the model's keys are too close for an exact comparison (gap {gap:.2e}): pick another draw"
    idx = first[6].cpu().numpy()
    assert m_n == batch and np.array_equal(idx, m_idx), "indices differ from the model's"
    w = first[5].cpu().numpy().ravel()
    assert (np.abs(w.astype(np.float64) - m_w) <= np.spacing(m_w)).all() and w.max() == 1.0
    rows = torch.cat(first[:5], dim=1)
    assert torch.equal(rows.view(torch.int32), buf.data[first[6]].view(torch.int32))
    return err


def main():
    import numpy as np
    import torch
    import per_ref
    from pdenv.sac import DevicePrioritizedReplayBuffer, KernelPrioritizedReplayBuffer
    if not torch.cuda.is_available():
        sys.exit("per_sample_time.py measures on the GPU: no HIP device visible")
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 50))
    sizes = [int(x) for x in os.environ.get("SIZES", "32768,262144,1000000").split(",")]
    batches = [int(x) for x in os.environ.get("BATCHES", "256,512").split(",")]
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "per_sample.json")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"round_trip": "sample(B) then update_priorities(indices, td)", "row_floats": 2 * S + A + 2, "alpha": ALPHA,
           "priorities": "log-uniform 1e-6 .. 1e3", "repeats": repeats, "round_trips_per_window": inner,
           "key_error_bound_rel": per_ref.KEY_BOUND, "key_error_bound_ulp": 32, "shapes": []}
    worst = 0.0
    for size in sizes:
        pri_np = (10.0 ** rng.uniform(-6, 3, size)).astype(np.float32)
        rows = torch.from_numpy(rng.standard_normal((size, 2 * S + A + 2)).astype(np.float32)).to(dev)
        for batch in batches:
            bufs = {"torch": DevicePrioritizedReplayBuffer(size, S, A, dev, alpha=ALPHA),
                    "kernel": KernelPrioritizedReplayBuffer(size, S, A, dev, alpha=ALPHA, seed=SEED)}
            for b in bufs.values():
                b.add_batch(rows)
                b.priorities.copy_(torch.from_numpy(pri_np))
                b.max_priority = float(pri_np.max())
            err = check_shape(np, torch, per_ref, bufs["kernel"], pri_np, batch, draw=1)
            worst = max(worst, err)
            td = torch.from_numpy((10.0 ** rng.uniform(-6, 3, batch)).astype(np.float32)).to(dev)
            gen = torch.Generator(device=dev).manual_seed(0)

            def trip(name):
                b = bufs[name]
                out = b.sample(batch, generator=gen) if name == "torch" else b.sample(batch)
                b.update_priorities(out[6], td)

            times = {k: [] for k in bufs}
            for rnd in range(repeats + 1):              # round 0: warm-up, not kept
                for name in bufs:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(inner):
                        trip(name)
                    torch.cuda.synchronize(dev)
                    if rnd:
                        times[name].append((time.perf_counter() - t0) * 1e3 / inner)
            entry = {"size": size, "batch": batch, "checks_passed": True, "key_error_rel": err,
                     "key_error_ulp": err / per_ref.ULP64}
            for name, ts in times.items():
                entry[name] = {"ms": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
            entry["torch_over_kernel"] = entry["torch"]["ms"] / entry["kernel"]["ms"]
            res["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
    res["key_error_max_rel"] = worst
    res["key_error_max_ulp"] = worst / per_ref.ULP64
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
