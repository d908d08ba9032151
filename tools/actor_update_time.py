#!/usr/bin/env python3
"""Times the actor and temperature steps of the SAC update -- steps 4 to 6 of SACPyTorch.update
(sac_pytorch.py:485-521) -- on the rows of a sampled batch, both ways in the same run: `torch`, the
block as torch expressions (actor.sample, the critic on the new actions, the loss, zero_grad,
backward, optional clip_grad_norm_, both Adam steps), and `kernel`, pdenv.sac.ActorUpdate
(pd_sac_actor_grad and two pd_adam_step calls: five launches).  Both run on the same rows, eps and PER
weights, each on its own copy of the actor and log_alpha and its own torch.optim.Adams.

(S, A) = (2, 1), hidden 256, two hidden layers (the driver's defaults); batches 256 and 512; PER
weights, without and with clipping.  Before a shape is timed the kernel path is checked there as
tests/test_gpu_sac_actor_update.py does: the same call twice gives equal bits (gradients and every
output), and every gradient tensor is within max(4 x torch's float32 autograd error, B 2^-24 sum
|terms|) of float64 autograd (the rows are that test's fixture at this batch size: rows at which the
loss is differentiable with margin).

Each timed window is INNER calls between two device synchronisations (host clock, one
synchronisation at the end of the window only); the variants alternate within each of REPEATS rounds
after a warm-up round; the JSON holds the median and the min / max over the rounds.  Also timed the
same way: `grad_alone` (pd_sac_actor_grad: three launches), `adam_alone` (both pd_adam_step calls)
and `kernel_fixed_alpha` (ActorUpdate without an alpha optimizer: what the second pd_adam_step call
costs is kernel - kernel_fixed_alpha).

A second table, `whole_update`: pdenv.sac.sac_update (sample, TdTarget, CriticUpdate, ActorUpdate,
update_priorities on a KernelPrioritizedReplayBuffer: no host synchronisation) against the body of
SACPyTorch.update in torch on the device buffers (DevicePrioritizedReplayBuffer.sample, the no_grad
block, the critic step, the actor and temperature steps, update_priorities -- which reads the largest
priority back, as the reference does -- and the Polyak loop), the same protocol.

The kernels one by one come from a kernel trace:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/actor_update_time.py --loop BATCH
  python tools/actor_update_time.py --stats BATCH=DIR/.../*_kernel_stats.csv ... [out.json]
adds their average durations to the whole-update table of an existing JSON; --loop-actor BATCH and
--stats-actor do the same for ActorUpdate calls alone and the per-call table (the whole update's
kernels run behind other kernels and on freshly sampled rows, so their durations differ a little).
  python tools/actor_update_time.py [out.json]      (default profiles/sac_actor_update.json)
Environment: REPEATS, INNER, BATCHES (comma-separated)."""
import copy
import csv
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

S, A, H, L = 2, 1, 256, 2
LR, LR_ALPHA, TAU, MAX_NORM, GAMMA = 3e-4, 3e-4, 0.005, 1.0, 0.99
KERNELS = ("k_actor_fwd", "k_actor_bwd", "k_actor_wgrad", "k_adam", "k_critic_rows", "k_critic_wgrad", "k_sac_td_target",
           "k_per_")


def make(batch):
    """The case of one batch size on the device: actor, critic, rows, eps, weights, log_alpha."""
    import torch
    import sac_actor_grad_nets as an
    case = an.real_case(S, A, H, L, n=batch)
    dev = dict(actor=copy.deepcopy(case["actor"]).cuda(), critic=copy.deepcopy(case["critic"]).cuda(),
               rows=torch.from_numpy(case["rows"]).cuda(), eps=torch.from_numpy(case["eps"]).cuda(),
               w=torch.from_numpy(case["weights"]).cuda().reshape(-1, 1),
               log_alpha=torch.full((1,), case["log_alpha"], device="cuda"))
    return case, dev


def check_shape(case, dev):
    """Equal bits twice and the gradients within the bound, at this batch size; the worst ratio
    err_kernel / max(4 err_torch, floor)."""
    import numpy as np
    import torch
    import sac_actor_grad_nets as an
    import sac_grad_nets as gn
    import sac_td_nets as td
    import test_gpu_sac_actor_update as T
    n = case["n"]
    actor, critic = dev["actor"], dev["critic"]
    aparams = [t.data for t in T.actor_tensors(actor)]
    cparams = [[t for m in td.q_linears(net) for t in (m.weight.data, m.bias.data)] for net in (critic.q1, critic.q2)]
    run = lambda: T.run_actor(aparams, cparams, dev["rows"], n, S, A, H, L, H, L, weights=dev["w"].reshape(-1),
                              eps=dev["eps"], log_alpha=dev["log_alpha"], ma=actor.max_action)
    first, second = run(), run()
    for a, b in zip(first["grads"], second["grads"]):
        assert T.same_bits(a, b), "the same call gave other gradient bits"
    for k in T.OUTS:
        assert T.same_bits(first[k], second[k]), f"{k}: the same call gave other bits"
    rows, eps, w = (torch.from_numpy(case[k]) for k in ("rows", "eps", "weights"))
    la, te = torch.full((1,), case["log_alpha"]), case["target_entropy"]
    ref = an.torch_block(copy.deepcopy(case["actor"]).double(), copy.deepcopy(case["critic"]).double(),
                         rows[:, :S].double(), eps.double(), w.double(), la.double(), te)["grads"]
    g_gpu = an.torch_block(copy.deepcopy(actor), copy.deepcopy(critic), dev["rows"][:, :S], dev["eps"], dev["w"],
                           dev["log_alpha"], te)["grads"]
    g_cpu = an.torch_block(copy.deepcopy(case["actor"]), copy.deepcopy(case["critic"]), rows[:, :S], eps, w, la, te)["grads"]
    got = [g.cpu().numpy().astype(np.float64) for g in first["grads"]]
    worst = 0.0
    for k, r in enumerate(ref):
        err_k = float(np.abs(got[k].reshape(r.shape) - r).max())
        err_t = max(float(np.abs(g_gpu[k] - r).max()), float(np.abs(g_cpu[k] - r).max()))
        bound = max(T.REAL_C * err_t, n * gn.EPS32 * case["ref"]["terms"][k])
        assert err_k <= bound, (k, err_k, err_t, bound)
        worst = max(worst, err_k / bound)
    return dict(grad_err_over_bound=worst, fixture_dropped=case["dropped"])


def torch_actor_block(actor, critic, log_alpha, opt, aopt, states, eps, w, max_norm, te):
    """Steps 4 to 6 (sac_pytorch.py:485-521) as torch expressions, Actor.sample written out on eps."""
    import torch
    mean, log_std = actor(states)
    std = log_std.exp()
    x = mean + std * eps
    action = torch.tanh(x)
    log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727
                - torch.log(1 - action.pow(2) + 1e-6)).sum(-1, keepdim=True)
    q1, q2 = critic(states, action * actor.max_action)
    q = torch.min(q1, q2)
    alpha = log_alpha.detach().exp()
    actor_loss = (w * (alpha * log_prob - q)).mean()
    opt.zero_grad()
    actor_loss.backward()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(actor.parameters(), max_norm=max_norm)
    opt.step()
    if aopt is not None:
        alpha_loss = -(log_alpha * w * (log_prob + te).detach()).mean()
        aopt.zero_grad()
        alpha_loss.backward()
        aopt.step()
    return log_prob


def variants(dev, clip):
    """{name: callable} on copies of the nets: the torch block, ActorUpdate, and its parts alone."""
    import torch
    from pdenv.sac import ActorUpdate
    rows, eps, w = dev["rows"], dev["eps"], dev["w"]
    states = rows[:, :S]                                    # the view a buffer's sample returns
    max_norm = MAX_NORM if clip else None
    te = -float(A)
    at, ct = copy.deepcopy(dev["actor"]), copy.deepcopy(dev["critic"])
    lt = dev["log_alpha"].clone().requires_grad_(True)
    ot, aot = torch.optim.Adam(at.parameters(), lr=LR), torch.optim.Adam([lt], lr=LR_ALPHA)

    def make_upd(tune):
        ak, ck = copy.deepcopy(dev["actor"]), copy.deepcopy(dev["critic"])
        lk = dev["log_alpha"].clone().requires_grad_(True)
        upd = ActorUpdate(ak, ck, lk, torch.optim.Adam(ak.parameters(), lr=LR),
                          torch.optim.Adam([lk], lr=LR_ALPHA) if tune else None, max_grad_norm=max_norm)
        assert upd.kernel
        upd(rows, w, eps=eps)                               # (creates the state and p.grad)
        return upd

    upd, fixed = make_upd(True), make_upd(False)
    B = int(rows.shape[0])
    return {"torch": lambda: torch_actor_block(at, ct, lt, ot, aot, states, eps, w, max_norm, te),
            "kernel": lambda: upd(rows, w, eps=eps), "kernel_fixed_alpha": lambda: fixed(rows, w, eps=eps),
            "grad_alone": lambda: upd.backward(rows, w, eps=eps), "adam_alone": lambda: upd._kernel_step(B, rows.device)}


def whole_variants(case, dev, batch, clip):
    """{name: callable}: sac_update on the kernels, and SACPyTorch.update's body in torch, each on its
    own learner over a buffer of 4 x batch rows."""
    import torch
    import torch.nn.functional as F
    import sac_td_nets as td
    from pdenv.sac import (ActorUpdate, CriticUpdate, DevicePrioritizedReplayBuffer, KernelPrioritizedReplayBuffer,
                           TdTarget, sac_update)
    max_norm = MAX_NORM if clip else None
    te = -float(A)
    slab = torch.cat([dev["rows"]] * 4)
    slab[:, -1] = (torch.arange(slab.shape[0], device="cuda") % 5 == 3).float()

    def learner(buffer_cls):
        actor, critic = copy.deepcopy(dev["actor"]), copy.deepcopy(dev["critic"])
        target = td.real_critic(S, A, H, L, seed=1).cuda()
        la = dev["log_alpha"].clone().requires_grad_(True)
        buf = buffer_cls(slab.shape[0], S, A, "cuda")
        buf.add_batch(slab)
        return dict(actor=actor, critic=critic, target=target, la=la, buf=buf,
                    copt=torch.optim.Adam(critic.parameters(), lr=LR), aopt=torch.optim.Adam(actor.parameters(), lr=LR),
                    lopt=torch.optim.Adam([la], lr=LR_ALPHA))

    k = learner(KernelPrioritizedReplayBuffer)
    tdt = TdTarget(k["actor"], k["target"], k["la"], GAMMA)
    cu = CriticUpdate(k["critic"], k["target"], k["copt"], tau=TAU, max_grad_norm=max_norm)
    au = ActorUpdate(k["actor"], k["critic"], k["la"], k["aopt"], k["lopt"], max_grad_norm=max_norm)
    assert tdt.kernel and cu.kernel and au.kernel
    t = learner(DevicePrioritizedReplayBuffer)

    def torch_update():
        states, actions, rewards, next_states, dones, w, idx = t["buf"].sample(batch)
        with torch.no_grad():
            na, nlp = t["actor"].sample(next_states)
            nq1, nq2 = t["target"](next_states, na)
            target_q = rewards + (1 - dones) * GAMMA * (torch.min(nq1, nq2) - t["la"].exp() * nlp)
        q1, q2 = t["critic"](states, actions)
        loss = (w * F.mse_loss(q1, target_q, reduction="none") + w * F.mse_loss(q2, target_q, reduction="none")).mean()
        t["copt"].zero_grad()
        loss.backward()
        if clip:
            torch.nn.utils.clip_grad_norm_(t["critic"].parameters(), max_norm=max_norm)
        t["copt"].step()
        eps = torch.randn(batch, A, device="cuda")
        torch_actor_block(t["actor"], t["critic"], t["la"], t["aopt"], t["lopt"], states, eps, w, max_norm, te)
        t["buf"].update_priorities(idx, torch.max((target_q - q1).abs(), (target_q - q2).abs()).detach())
        for p, tp in zip(t["critic"].parameters(), t["target"].parameters()):
            tp.data.copy_((1 - TAU) * tp.data + TAU * p.data)

    return {"torch": torch_update, "kernel": lambda: sac_update(k["buf"], tdt, cu, au, batch)}


def loop(batch, actor_only=False, calls=200):
    """--loop: sac_update calls alone, for a kernel trace of the whole update; --loop-actor: ActorUpdate
    calls alone on fixed rows, the per-call table's setting."""
    import torch
    case, dev = make(batch)
    fn = variants(dev, True)["kernel"] if actor_only else whole_variants(case, dev, batch, True)["kernel"]
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def merge_stats(out_path, pairs, table):
    """Average kernel durations of a trace into the clipped entry of its batch in `table`."""
    res = json.load(open(out_path))
    for pair in pairs:
        batch, path = pair.split("=", 1)
        rows = list(csv.DictReader(open(path)))
        avg = {}
        for r in rows:
            for k in KERNELS:
                m = re.search(r"\b(" + k + r"\w*(?:<[^>]*>)?)", r["Name"])
                if m:
                    avg[m.group(1)] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
        for entry in res[table]:
            if entry["batch"] == int(batch) and entry["clip"]:      # (the traced loops clip)
                entry["kernels_traced"] = avg
                if table == "shapes":
                    entry["kernels_traced_sum_us"] = sum(v["avg_us"] * v["calls"] for v in avg.values()) / 200
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("merged", pairs, "into", out_path, table)


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
    import torch
    args = sys.argv[1:]
    default = os.path.join(REPO, "profiles", "sac_actor_update.json")
    if args and args[0] in ("--loop", "--loop-actor"):
        return loop(int(args[1]), actor_only=args[0] == "--loop-actor")
    if args and args[0] in ("--stats", "--stats-actor"):
        pairs = [a for a in args[1:] if "=" in a]
        rest = [a for a in args[1:] if "=" not in a]
        return merge_stats(rest[0] if rest else default, pairs, "whole_update" if args[0] == "--stats" else "shapes")
    if not torch.cuda.is_available():
        sys.exit("actor_update_time.py measures on the GPU: no HIP device visible")
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 50))
    batches = [int(x) for x in os.environ.get("BATCHES", "256,512").split(",")]
    out_path = args[0] if args else default
    res = {"block": "actor.sample(states); critic(states, new_actions); min; the actor loss with PER weights; zero_grad(); "
                    "backward(); [clip_grad_norm_]; actor Adam.step(); the temperature loss; alpha Adam.step()  "
                    "(sac_pytorch.py:485-521)",
           "whole_block": "SACPyTorch.update's body (sac_pytorch.py:416-531): PER sample, the no_grad block, the critic step, "
                          "the actor and temperature steps, update_priorities, the Polyak loop",
           "state_dim": S, "action_dim": A, "hidden": H, "hidden_layers": L, "lr": LR, "tau": TAU, "max_norm": MAX_NORM,
           "repeats": repeats, "calls_per_window": inner, "shapes": [], "whole_update": []}
    for batch in batches:
        case, dev = make(batch)
        checks = check_shape(case, dev)
        for clip in (False, True):
            entry = {"batch": batch, "clip": clip, "checks_passed": True, **checks, **timed(variants(dev, clip), repeats, inner)}
            entry["torch_over_kernel"] = entry["torch"]["ms"] / entry["kernel"]["ms"]
            entry["second_adam_call_ms"] = entry["kernel"]["ms"] - entry["kernel_fixed_alpha"]["ms"]
            res["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            whole = {"batch": batch, "clip": clip, **timed(whole_variants(case, dev, batch, clip), repeats, inner)}
            whole["torch_over_kernel"] = whole["torch"]["ms"] / whole["kernel"]["ms"]
            res["whole_update"].append(whole)
            print(json.dumps(whole), flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
