#!/usr/bin/env python3
"""Wave lifetimes of the 512-thread c3 step kernel (diagnostic build -DPD_WAVE_TIMES of the c3 unit:
`python tools/variants.py wt=-DPD_WAVE_TIMES`, with `-DPD_PACE=n` for a pacing variant;
PDENV_LIB=.../libpdenv_wt.so): per wave of a FUSE-step launch (default 128) its start and end
(s_memrealtime, 100 MHz), its hardware slot (XCC, SE, CU, SIMD of HW_ID / XCC_ID), its index in the
workgroup and its clock after every 16th env-step.  Reports, per launch, the span, the wave
lifetimes, and for every SIMD (the two waves of a workgroup with the same SIMD id) when its first
and its last wave end -- split by whether the earlier one is the workgroup's wave 0-3 or 4-7 --
and how far apart the two are at each progress sample.  DESCENT=1: c3-descent."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "psso-sac-for-powered-descent_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import pdenv  # noqa: E402
import bench  # noqa: E402

F = int(os.environ.get("FUSE", "128"))
descent = os.environ.get("DESCENT") == "1"
n = 65536
REC = 16          # words per wave (pd_step_impl.h kWaveRec)
WPG = 8           # waves per workgroup
MS = 10e-9 * 1e3  # s_memrealtime tick in ms
env = pdenv.PoweredDescentEnv(n, enable_wind=True, stochastic_wind=True, wind_percentile=None, auto_reset=True,
                              tilt_sigma_rad=math.radians(1.0), seed=1234,
                              table_flags=int(os.environ.get("TABLE_FLAGS", "0")))
env.set_tuning(step_fuse=F)
burn = bench.DESCENT_BURN_IN if descent else 32
L = int(os.environ.get("LAUNCHES", "6"))
g = torch.Generator(device="cuda").manual_seed(42)
acts = bench.c3_actions(burn + L * F, n, g, "cuda", descent)
for t0 in range(0, burn, F):
    env.step_n_raw(acts[t0:min(t0 + F, burn)])
torch.cuda.synchronize()
fn = env.lib.pd_debug_wave_times
fn.argtypes = [C.c_void_p, C.c_int]
W = n * 2 // 64
NS = min(8, F // 16)   # progress samples per launch


def r4(x):
    return round(float(x), 4)


out = []
for k in range(L):
    env.step_n_raw(acts[burn + k * F:burn + (k + 1) * F])
    torch.cuda.synchronize()
    rec = np.zeros((W, REC), dtype=np.uint64)
    assert fn(rec.ctypes.data, W) == 0
    r = rec.astype(np.int64)
    t0, t1, hw, xcc, wv = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4]
    smp = r[:, 5:5 + NS]
    peer = r[:, 13]
    simd = (hw >> 4) & 3
    cu = (hw >> 8) & 15
    sh = (hw >> 12) & 1
    se = (hw >> 13) & 7
    slot = (((xcc & 15) * 8 + se) * 2 + sh) * 16 * 4 + cu * 4 + simd
    wg = np.arange(W) // WPG
    assert np.array_equal(wv, np.arange(W) % WPG), "wave index words"
    origin = t0.min()
    span = (t1.max() - origin) * MS
    dur = (t1 - t0) * MS
    # the SIMDs: the waves of one workgroup with one SIMD id
    pairs, odd = [], 0
    for w0 in range(0, W, WPG):
        for s in range(4):
            m = [w0 + j for j in range(WPG) if simd[w0 + j] == s]
            if len(m) == 2:
                pairs.append(m)
            elif m:
                odd += 1
    pairs = np.array(pairs)                     # [P][2], lower wave index first
    lo, hi = pairs[:, 0], pairs[:, 1]
    e_lo, e_hi = (t1[lo] - origin) * MS, (t1[hi] - origin) * MS
    first, last = np.minimum(e_lo, e_hi), np.maximum(e_lo, e_hi)
    gap = (last - first) / span
    lo_first = e_lo <= e_hi                     # the earlier-ending wave is the lower one (0-3 when partners are w, w + 4)
    early_low_half = np.where(lo_first, wv[lo], wv[hi]) < WPG // 2
    slow = int(np.argmax(last))

    def part(m):
        if not m.any():
            return {"simds": 0}
        return {"simds": int(m.sum()), "first_end_over_span": r4((first[m] / span).mean()),
                "last_end_over_span": r4((last[m] / span).mean()), "gap_over_span": r4(gap[m].mean())}
    # progress: the upper wave's clock minus the lower wave's at each sample (positive: the upper one is behind)
    dprog = (smp[hi] - smp[lo]) * MS / span
    o = {"launch_span_ms": r4(span), "wave_ms_mean": r4(dur.mean()), "wave_ms_min": r4(dur.min()),
         "wave_ms_max": r4(dur.max()), "wave_mean_over_span": r4(dur.mean() / span),
         "wave_min_over_span": r4(dur.min() / span), "start_spread_ms": r4((t0.max() - t0.min()) * MS),
         "hw_slots": int(len(np.unique(slot))), "simds": int(len(pairs)), "simds_not_two_waves": odd,
         "partners_w_plus_4_frac": r4(np.mean(hi - lo == WPG // 2)),
         "pace_partner_found_frac": r4(np.mean(peer[lo] == wv[hi])),
         "first_end_over_span": r4((first / span).mean()), "last_end_over_span": r4((last / span).mean()),
         "gap_over_span_mean": r4(gap.mean()), "gap_over_span_p10": r4(np.percentile(gap, 10)),
         "gap_over_span_p90": r4(np.percentile(gap, 90)), "gap_over_span_max": r4(gap.max()),
         "gap_above_5pct_frac": r4(np.mean(gap > 0.05)),
         "lower_wave_ends_first_frac": r4(lo_first.mean()),
         "early_is_wave_0_3": part(early_low_half), "early_is_wave_4_7": part(~early_low_half),
         "slowest_simd": {"first_end_over_span": r4(first[slow] / span), "last_end_over_span": r4(last[slow] / span),
                          "early_wave": int(wv[lo[slow]] if lo_first[slow] else wv[hi[slow]])},
         "progress_steps": [16 * (j + 1) for j in range(NS)],
         "progress_upper_minus_lower_over_span_mean": [r4(x) for x in dprog.mean(axis=0)],
         "progress_abs_gap_over_span_mean": [r4(x) for x in np.abs(dprog).mean(axis=0)]}
    out.append(o)
print(json.dumps({"lib": os.path.basename(os.environ.get("PDENV_LIB", "libpdenv.so")), "descent": descent, "fuse": F,
                  "table_flags": int(os.environ.get("TABLE_FLAGS", "0")), "launches": out}))
