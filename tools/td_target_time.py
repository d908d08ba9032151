#!/usr/bin/env python3
"""Times the inference-only third of the SAC update -- the torch.no_grad() block of
SACPyTorch.update (sac_pytorch.py:439-443) -- on the rows of a sampled batch, both ways in the same
run: `torch`, the block as torch expressions (Actor.sample with its own torch.randn, the Critic, the
two lines of arithmetic), and `kernel`, pdenv.sac.TdTarget (pd_sac_td_target, one launch, eps drawn
in the kernel).

Batches 256 and 512, (S, A) = (2, 1), hidden 256 and two hidden layers for the actor and the critic
(the driver's defaults).  Before a shape is timed the kernel path is checked there: the same call
twice gives equal bits; heads and next_q are pd_sac_actor's and pd_sac_critic's bits; the
elementwise chain is within its a-priori bound of the binary64 model (tests/sac_td_nets.py); and
max |target_q - ref64| is at most 4 times torch's own float32 error on the same eps.

Each timed window is INNER calls between two device synchronisations (host clock, one
synchronisation at the end of the window only); the two alternate within each of REPEATS rounds
after a warm-up round; the JSON holds the median and the min / max over the rounds.
  python tools/td_target_time.py [out.json]      (default profiles/sac_td_target.json)
Environment: REPEATS, INNER, BATCHES (comma-separated)."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

S, A, H, L = 2, 1, 256, 2
REAL_C = 4.0


def check_shape(np, torch, td, case, dev, tdt):
    """The kernel path at one timed shape against its pieces and the models; returns the measured
    figures."""
    from pdenv.sac import ActorKernel, CriticKernel
    n = case["n"]
    bits = lambda t: t.contiguous().view(torch.int32)

    def run():
        out = dict(target_q=torch.empty(n, device="cuda"), next_actions=torch.empty(n, A, device="cuda"),
                   next_log_prob=torch.empty(n, device="cuda"), next_q=torch.empty(n, 2, device="cuda"),
                   heads=torch.empty(n, 2 * A, device="cuda"), eps_out=torch.empty(n, A, device="cuda"))
        tdt(dev["rows"], out=out["target_q"], eps=dev["eps"], **{k: v for k, v in out.items() if k != "target_q"})
        torch.cuda.synchronize()
        return out

    first, second = run(), run()
    for k in first:
        assert torch.equal(bits(first[k]), bits(second[k])), f"{k}: the same call gave other bits"
    ns = dev["rows"][:, S + A + 1:2 * S + A + 1].contiguous()
    heads, q = torch.empty(n, 2 * A, device="cuda"), torch.empty(n, 2, device="cuda")
    ActorKernel(dev["actor"])(ns, heads)
    CriticKernel(dev["critic"])(ns, first["next_actions"], q)
    torch.cuda.synchronize()
    assert torch.equal(bits(first["heads"]), bits(heads)) and torch.equal(bits(first["next_q"]), bits(q))
    actor = case["actor"]
    c = td.chain(first["heads"].cpu().numpy(), first["eps_out"].cpu().numpy(), first["next_q"].cpu().numpy(),
                 case["rows"], S, A, actor.log_std_min, actor.log_std_max, actor.max_action,
                 float(case["log_alpha"][0]), case["gamma"])
    worst = 0.0
    for name, bound in zip(("next_actions", "next_log_prob", "target_q"), td.chain_bound(c)):
        err = np.abs(first[name].cpu().numpy().astype(np.float64) - c[name])
        assert (err <= bound).all(), f"{name}: the chain misses its bound"
        worst = max(worst, float((err / bound).max()))
    ref = td.full(case)[0]["target_q"]
    g = td.torch_block(dev["actor"], dev["critic"], dev["rows"], dev["eps"], dev["log_alpha"], case["gamma"], S, A)[0]
    err_k = float(np.abs(first["target_q"].cpu().numpy().astype(np.float64) - ref).max())
    err_g = float(np.abs(g.cpu().numpy().astype(np.float64).reshape(-1) - ref).max())
    assert err_g > 0 and err_k <= REAL_C * err_g, (err_k, err_g)
    return dict(chain_err_over_bound=worst, err_kernel=err_k, err_torch=err_g)


def main():
    import copy
    import numpy as np
    import torch
    import sac_td_nets as td
    from pdenv.sac import TdTarget
    if not torch.cuda.is_available():
        sys.exit("td_target_time.py measures on the GPU: no HIP device visible")
    repeats, inner = int(os.environ.get("REPEATS", 7)), int(os.environ.get("INNER", 50))
    batches = [int(x) for x in os.environ.get("BATCHES", "256,512").split(",")]
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "sac_td_target.json")
    res = {"block": "actor.sample(next_states); critic_target(next_states, next_actions); min - alpha * log_prob; "
                    "rewards + (1 - dones) * gamma * next_q  (sac_pytorch.py:439-443)",
           "state_dim": S, "action_dim": A, "hidden": H, "hidden_layers": L, "repeats": repeats,
           "calls_per_window": inner, "shapes": []}
    for batch in batches:
        case = td.td_case(S, A, H, L, n=batch)
        dev = dict(actor=copy.deepcopy(case["actor"]).cuda(), critic=copy.deepcopy(case["critic"]).cuda(),
                   rows=torch.from_numpy(case["rows"]).cuda(), eps=torch.from_numpy(case["eps"]).cuda(),
                   log_alpha=case["log_alpha"].clone().cuda())
        tdt = TdTarget(dev["actor"], dev["critic"], dev["log_alpha"], case["gamma"], seed=1)
        assert tdt.kernel
        checks = check_shape(np, torch, td, case, dev, tdt)
        rows, actor, critic, log_alpha, gamma = dev["rows"], dev["actor"], dev["critic"], dev["log_alpha"], case["gamma"]
        # the views a buffer's sample returns
        rewards, next_states, dones = rows[:, S + A:S + A + 1], rows[:, S + A + 1:2 * S + A + 1], rows[:, 2 * S + A + 1:]

        def torch_call():
            with torch.no_grad():
                next_actions, next_log_probs = actor.sample(next_states)
                next_q1, next_q2 = critic(next_states, next_actions)
                next_q = torch.min(next_q1, next_q2) - log_alpha.exp() * next_log_probs
                return rewards + (1 - dones) * gamma * next_q

        # (for DESIGN.md s6's grid note: the two pieces as launches of their own on the same rows)
        from pdenv.sac import ActorKernel, CriticKernel
        ak, ck = ActorKernel(actor), CriticKernel(critic)
        ns_c = next_states.contiguous()
        heads, na, q = (torch.zeros(batch, k, device="cuda") for k in (2 * A, A, 2))
        calls = {"torch": torch_call, "kernel": lambda: tdt(rows), "pd_sac_actor_alone": lambda: ak(ns_c, heads),
                 "pd_sac_critic_alone": lambda: ck(ns_c, na, q)}
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
        entry = {"batch": batch, "checks_passed": True, **checks}
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
