"""Regenerates tests/golden/ref_learning_stats.npz (arrays and names only, a few kilobytes).

Imports the reference's SACPyTorch (PDENV_REFERENCE, read-only) on the CPU from a temporary working
directory (its constructor creates data/agent_saves/... under the cwd), calls its own
_track_learning_stats on seeded inputs and stores the inputs and the values it recorded, for three
shapes (S, A, B, per).  Also measured here and stored per shape: the reference's largest deviation
from the binary64 model (tests/learning_stats_ref.py) relative to each column's scale -- the reference
computes in float32 -- which the CPU test allows four times over.

    python tests/golden/make_golden_learning_stats.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PDENV_REFERENCE", "/root/reference")
SHAPES = ((2, 1, 261, True), (5, 4, 17, True), (8, 2, 512, False))
sys.path.insert(0, os.path.dirname(HERE))
import learning_stats_ref as M  # noqa: E402


def main():
    import torch
    import scipy.stats  # noqa: F401  (the reference says `import scipy` and uses scipy.stats)
    sys.path.insert(0, os.path.join(REF, "src", "agents"))
    out = {"names": np.array(M.NAMES), "shapes": np.array([[s, a, b, int(p)] for s, a, b, p in SHAPES])}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            from sac_pytorch import SACPyTorch
            for k, (S, A, B, per) in enumerate(SHAPES):
                rng = np.random.default_rng(1000 + k)
                rows, q, target_q, log_prob, weights = M.make_inputs(rng, S, A, B, per=per)
                for name, x in M.series_of(rows, q, target_q, log_prob, S, A).items():
                    for s in (x if name == "state" else [x]):
                        assert np.abs(s).max() <= 64 * s.astype(np.float64).std(), (name, S, A, B)
                losses = rng.standard_normal(3).astype(np.float32)
                log_alpha = np.float32(np.log(0.2) + 0.1 * k)
                beta, max_prio, step = 0.4 + 0.01 * k, float(np.float32(1.5 + k)), 7 + k
                agent = SACPyTorch(S, A, hidden_dim_actor=8, hidden_dim_critic=8, buffer_size=16, batch_size=4,
                                   device="cpu", use_per=per)
                agent.log_alpha = torch.tensor(float(log_alpha), dtype=torch.float64)
                agent.updates = step
                if per:
                    agent.replay_buffer.beta, agent.replay_buffer.max_priority = beta, max_prio
                t = torch.from_numpy
                with contextlib.redirect_stdout(io.StringIO()):
                    agent._track_learning_stats(
                        states=t(rows[:, :S]), actions=t(rows[:, S:S + A]), rewards=t(rows[:, S + A:S + A + 1]),
                        critic_loss=t(losses[0:1])[0], actor_loss=t(losses[1:2])[0], alpha_loss=t(losses[2:3])[0],
                        q_values=torch.min(t(q[:, :1]), t(q[:, 1:])), target_q=t(target_q), log_probs=t(log_prob),
                        weights=t(weights) if per else None)
                keys = list(agent.learning_stats)
                rec = np.array([float(agent.learning_stats[n][0]) for n in keys])
                model, scale = M.model_row(rows, q, target_q, log_prob, S, A, weights=weights, critic_loss=losses[0],
                                           actor_loss=losses[1], alpha_loss=losses[2], log_alpha=log_alpha,
                                           max_priority=max_prio if per else None, per_beta=beta, step=step,
                                           scales=True)
                idx = [M.NAMES.index(n) for n in keys]
                dev = np.abs(rec - model[idx]) / np.abs(scale[idx])
                worst = int(np.argmax(dev))
                print(f"(S, A, B, per) = {(S, A, B, per)}: largest deviation {dev.max():.3e} ({keys[worst]}), "
                      f"relative to the value {np.max(np.abs(rec - model[idx]) / np.maximum(np.abs(model[idx]), 1e-300)):.3e}",
                      file=sys.stderr)
                out.update({f"rows_{k}": rows, f"q_{k}": q, f"target_q_{k}": target_q, f"log_prob_{k}": log_prob,
                            f"losses_{k}": losses, f"log_alpha_{k}": np.float32(log_alpha),
                            f"per_{k}": np.array([beta, max_prio]), f"step_{k}": np.int64(step),
                            f"keys_{k}": np.array(keys), f"recorded_{k}": rec, f"deviation_{k}": dev,
                            f"max_deviation_{k}": np.float64(dev.max())})
                if per:
                    out[f"weights_{k}"] = weights
        finally:
            os.chdir(cwd)
    path = os.path.join(HERE, "ref_learning_stats.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
