"""bench.py's command line: the plain run's line, --full, and --dump-outputs.

The plain run (`--gpus 1 --steps K --warmup W`) times exactly K steps and prints the headline
fields alone; --dump-outputs writes the last timed step's outputs as float32 / float64 .npy files
from seeded inputs, so two runs of the same arguments write the same bytes."""
import json
import os
import sys

import numpy as np
import pytest

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "workload_counts", "launch_index", "c3_descent", "c3_fresh", "c3_staggered",
             "other_workloads", "cpu_baseline", "secondary")


def run_bench(monkeypatch, capsys, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)
    arrays = {"big": big, "flags": torch.tensor([0, 1, 1], dtype=torch.uint8), "ids": torch.tensor([-1, 4], dtype=torch.int8),
              "f32": torch.tensor([0.5, 1.5])}
    bench.dump_outputs(str(tmp_path / "a"), 0, arrays)
    bench.dump_outputs(str(tmp_path / "b"), 0, arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == sorted(arrays)
    assert got["big"].dtype == np.float64 and all(got[k].dtype == np.float32 for k in ("flags", "ids", "f32"))
    assert got["flags"].tolist() == [0.0, 1.0, 1.0] and got["ids"].tolist() == [-1.0, 4.0]
    assert sum(a.nbytes for a in got.values()) <= 4096
    # the oversized array: a sorted sample of its own elements, the same one in every run
    s = got["big"]
    assert s.ndim == 1 and s.size == 4096 // 4 // 8 and np.all(np.diff(s) > 0) and np.all(np.isin(s, big.numpy()))
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    bench.dump_outputs(str(tmp_path / "a"), 3, {"f32": arrays["f32"]})
    assert os.path.exists(tmp_path / "a" / "f32_rank3.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [1, 2, 128])
def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys, fuse):
    """5 timed steps in launches of `fuse` (one per step; two full and a partial one; one partial
    launch): the line holds the headline fields and none of --full's; the dump is the last timed
    step of the same seeded run stepped through the public step_n, bit for bit, twice."""
    import torch
    import bench
    import pdenv
    n, K, W, B = 192, 5, 3, 7
    argv = ["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(n), "--c3-burn-in", str(B),
            "--fuse", str(fuse)]
    dumps = []
    for d in ("a", "b"):
        line = run_bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / d)])
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == K and line["warmup"] == W and line["dtype"] == "f64" and line["unit"] == "env-steps/s"
        assert line["higher_is_better"] is True and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(n * 1e3 / line["ms_per_step"])
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert sorted(a) == ["done", "obs", "reward", "state", "trunc_id", "truncated"]
    for k in a:
        assert a[k].dtype == (np.float64 if k in ("obs", "reward", "state") else np.float32)
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["obs"].shape == (n, 2) and a["state"].shape == (n, 11) and a["reward"].shape == (n,)
    # the same run through the public surface: B + W + K steps of the benchmark's actions
    import math
    env = pdenv.PoweredDescentEnv(n, flight_phase="landing_burn_pure_throttle", mode="rl", precision="f64", device=0,
                                  enable_wind=True, stochastic_wind=True, wind_percentile=None, auto_reset=True,
                                  tilt_sigma_rad=math.radians(1.0), seed=1234, env_offset=0)
    g = torch.Generator(device=env.device).manual_seed(42)
    acts = bench.c3_actions(B + W + K, n, g, env.device, False)
    obs, rew, dn, tr, tid = env.step_n(acts)
    want = {"obs": obs[-1], "reward": rew[-1], "done": dn[-1], "truncated": tr[-1], "trunc_id": tid[-1], "state": env.state}
    for k, t in want.items():
        assert np.array_equal(a[k], t.double().cpu().numpy() if a[k].dtype == np.float64 else t.float().cpu().numpy(),
                              equal_nan=True), k


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements(monkeypatch, capsys):
    """--full at a small size: the roofline fields, the counts and the other c3 windows are in the
    line as before, beside the same headline fields."""
    line = run_bench(monkeypatch, capsys, ["--gpus", "1", "--steps", "4", "--warmup", "2", "--envs", "192",
                                           "--c3-burn-in", "6", "--full", "--cpu-baseline", "0"])
    assert all(k in line for k in HEADLINE)
    for k in ("roofline", "workload_counts", "launch_index", "c3_descent", "c3_fresh", "c3_staggered"):
        assert k in line, k
    assert line["roofline"]["kernel_launches_timed"] == 1 and line["workload_counts"]["env_substeps"] == 192 * 4 * 4
