#!/usr/bin/env python3
"""Times the critic step of the SAC update -- steps 2, 3 and 8 of SACPyTorch.update and step 7's |td|
(sac_pytorch.py:445-483, :526, :530-531) -- on the rows of a sampled batch, both ways in the same run:
`torch`, the block as torch expressions (critic forward, the loss, zero_grad, backward, optional
clip_grad_norm_, Adam.step, the Polyak loop, max |td|), and `kernel`, pdenv.sac.CriticUpdate
(pd_sac_critic_grad and pd_adam_step: three launches).  Both run on the same rows, targets and PER
weights, each on its own copy of the nets and its own torch.optim.Adam.

(S, A) = (2, 1), hidden 256, two hidden layers (the driver's defaults); batches 256 and 512; L2 loss
with PER weights, without and with clipping.  Before a shape is timed the kernel path is checked
there as tests/test_gpu_sac_update.py does: the same call twice gives equal bits (gradients, q, td_abs,
loss), and every gradient tensor is within max(4 x torch's float32 autograd error, B 2^-24 sum |terms|)
of float64 autograd.

Each timed window is INNER calls between two device synchronisations (host clock, one
synchronisation at the end of the window only); the variants alternate within each of REPEATS rounds
after a warm-up round; the JSON holds the median and the min / max over the rounds.  Also timed the
same way: the two C calls alone (`grad_alone`: the row pass and the weight-gradient pass;
`adam_alone`: the optimizer pass).  The three kernels one by one come from a kernel trace:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/critic_update_time.py --loop BATCH
  python tools/critic_update_time.py --stats BATCH=DIR/.../*_kernel_stats.csv ... [out.json]
adds their average durations to an existing JSON.
  python tools/critic_update_time.py [out.json]      (default profiles/sac_critic_update.json)
Environment: REPEATS, INNER, BATCHES (comma-separated)."""
import copy
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

S, A, H, L = 2, 1, 256, 2
LR, TAU, MAX_NORM = 3e-4, 0.005, 1.0
KERNELS = ("k_critic_rows", "k_critic_wgrad", "k_adam")


def make(batch):
    """The case of one batch size on the device: critic, target, rows, target_q, weights."""
    import torch
    import sac_grad_nets as gn
    import sac_td_nets as td
    case = gn.grad_case(S, A, H, L, n=batch)
    dev = dict(critic=copy.deepcopy(case["critic"]).cuda(), target=td.real_critic(S, A, H, L, seed=1).cuda(),
               rows=torch.from_numpy(case["rows"]).cuda(), tq=torch.from_numpy(case["target"]).cuda().reshape(-1, 1),
               w=torch.from_numpy(case["weights"]).cuda().reshape(-1, 1))
    return case, dev


def check_shape(case, dev):
    """Equal bits twice and the gradients within the bound, at this batch size; the worst ratio
    err_kernel / max(4 err_torch, floor)."""
    import numpy as np
    import torch
    import sac_grad_nets as gn
    import sac_td_nets as td
    import test_gpu_sac_update as T
    n = case["n"]
    critic = dev["critic"]
    params = [[t for m in td.q_linears(net) for t in (m.weight.data, m.bias.data)] for net in (critic.q1, critic.q2)]
    run = lambda: T.run_grad(params, dev["rows"], n, S, A, H, L, target=dev["tq"].reshape(-1), weights=dev["w"].reshape(-1))
    first, second = run(), run()
    for w in range(2):
        for a, b in zip(first["grads"][w], second["grads"][w]):
            assert T.same_bits(a, b), "the same call gave other gradient bits"
    for k in ("q", "td_abs", "loss", "partials"):
        assert T.same_bits(first[k], second[k]), f"{k}: the same call gave other bits"
    rows, tq, w = (torch.from_numpy(case[k]) for k in ("rows", "target", "weights"))
    ref, _ = T.torch_grads(copy.deepcopy(case["critic"]).double(), rows.double(), tq.double(), w.double(), S, A)
    g_gpu, _ = T.torch_grads(copy.deepcopy(critic), dev["rows"], dev["tq"], dev["w"], S, A)
    g_cpu, _ = T.torch_grads(copy.deepcopy(case["critic"]), rows, tq, w, S, A)
    _, terms, _ = gn.full_backward(td.critic_params(case["critic"]), case["rows"][:, :S + A], case["target"],
                                   case["weights"], gn.L2)
    got = [g.cpu().numpy().astype(np.float64) for k in range(2) for g in first["grads"][k]]
    worst = 0.0
    for k, r in enumerate(ref):
        err_k = float(np.abs(got[k].reshape(r.shape) - r).max())
        err_t = max(float(np.abs(g_gpu[k] - r).max()), float(np.abs(g_cpu[k] - r).max()))
        bound = max(T.REAL_C * err_t, n * gn.EPS32 * terms[k])
        assert err_k <= bound, (k, err_k, err_t, bound)
        worst = max(worst, err_k / bound)
    return dict(grad_err_over_bound=worst)


def variants(dev, clip):
    """{name: callable} on copies of the nets: the torch block, CriticUpdate, and the two C calls alone."""
    import torch
    import torch.nn.functional as F
    from pdenv.sac import CriticUpdate
    rows, tq, w = dev["rows"], dev["tq"], dev["w"]
    states, actions = rows[:, :S], rows[:, S:S + A]         # the views a buffer's sample returns
    max_norm = MAX_NORM if clip else None
    ct, tt = copy.deepcopy(dev["critic"]), copy.deepcopy(dev["target"])
    ot = torch.optim.Adam(ct.parameters(), lr=LR)

    def torch_call():
        q1, q2 = ct(states, actions)
        loss = (w * F.mse_loss(q1, tq, reduction="none") + w * F.mse_loss(q2, tq, reduction="none")).mean()
        ot.zero_grad()
        loss.backward()
        if clip:
            torch.nn.utils.clip_grad_norm_(ct.parameters(), max_norm=max_norm)
        ot.step()
        for p, tp in zip(ct.parameters(), tt.parameters()):
            tp.data.copy_((1 - TAU) * tp.data + TAU * p.data)
        return torch.max((tq - q1).abs(), (tq - q2).abs()).detach()

    ck, tk = copy.deepcopy(dev["critic"]), copy.deepcopy(dev["target"])
    upd = CriticUpdate(ck, tk, torch.optim.Adam(ck.parameters(), lr=LR), tau=TAU, max_grad_norm=max_norm)
    assert upd.kernel
    upd(rows, tq, w)                                        # (creates the state and p.grad)
    B = int(rows.shape[0])
    return {"torch": torch_call, "kernel": lambda: upd(rows, tq, w), "grad_alone": lambda: upd.backward(rows, tq, w),
            "adam_alone": lambda: upd._kernel_step(B, rows.device)}


def loop(batch, calls=200):
    """--loop: CriticUpdate calls alone, for a kernel trace."""
    import torch
    _, dev = make(batch)
    fn = variants(dev, True)["kernel"]
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def merge_stats(out_path, pairs):
    res = json.load(open(out_path))
    for pair in pairs:
        batch, path = pair.split("=", 1)
        rows = list(csv.DictReader(open(path)))
        avg = {}
        for r in rows:
            for k in KERNELS:
                if k in r["Name"]:
                    avg[k] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
        for entry in res["shapes"]:
            if entry["batch"] == int(batch) and entry["clip"]:      # (the traced loop clips)
                entry["kernels_traced"] = avg
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("merged", pairs, "into", out_path)


def main():
    import torch
    args = sys.argv[1:]
    default = os.path.join(REPO, "profiles", "sac_critic_update.json")
    if args and args[0] == "--loop":
        return loop(int(args[1]))
    if args and args[0] == "--stats":
        pairs = [a for a in args[1:] if "=" in a]
        rest = [a for a in args[1:] if "=" not in a]
        return merge_stats(rest[0] if rest else default, pairs)
    if not torch.cuda.is_available():
        sys.exit("critic_update_time.py measures on the GPU: no HIP device visible")
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 50))
    batches = [int(x) for x in os.environ.get("BATCHES", "256,512").split(",")]
    out_path = args[0] if args else default
    res = {"block": "critic(states, actions); the L2 loss with PER weights; zero_grad(); backward(); [clip_grad_norm_]; "
                    "Adam.step(); the Polyak loop; max |td|  (sac_pytorch.py:445-483, :526, :530-531)",
           "state_dim": S, "action_dim": A, "hidden": H, "hidden_layers": L, "lr": LR, "tau": TAU, "max_norm": MAX_NORM,
           "repeats": repeats, "calls_per_window": inner, "shapes": []}
    for batch in batches:
        case, dev = make(batch)
        checks = check_shape(case, dev)
        for clip in (False, True):
            calls = variants(dev, clip)
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
            entry = {"batch": batch, "clip": clip, "checks_passed": True, **checks}
            for name, ts in times.items():
                entry[name] = {"ms": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
            entry["torch_over_kernel"] = entry["torch"]["ms"] / entry["kernel"]["ms"]
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
