"""developer tool: cost of reading ALEPPO_F_BATCH_STATS against what a caller needs for the same ten numbers without it -
the four plane reads (values, returns, advantages, masks: each a device pass, a copy and a stream synchronise) plus the
numpy reduction of tests/batch_stats_ref.py - at two rollout shapes: 128 envs x T = 128 (bf16 network) and 4096 envs x
T = 5 (fp32, v1.yaml's shape).  `python tests/tools/batch_stats_time.py [reps]`.  After a warm-up the two are alternated
in one process on one context; host clock around calls that end in a stream synchronise; the median, the minimum and the
10th / 90th percentiles over `reps` (default 200) repetitions each.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))
import batch_stats_ref as br  # noqa: E402
import hashfill as hf  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_gpu_at_size import DeviceBytes, _flags  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
pkg = load_package()


def summary(ts):
    v = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(float(v[0]), 1),
                p10_us=round(float(v[len(v) // 10]), 1), p90_us=round(float(v[len(v) * 9 // 10]), 1))


out = {"reps": reps}
for E, T, prec, H in ((128, 128, "bf16", 512), (4096, 5, "fp32", 32)):
    eng = pkg.Engine(E, T, 4, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
    eng.load_params(hf.fill_params(310, H, 4))
    eb = min(E, 128)
    base = hf.hf_bytes(311, (T, eb, 84, 84))
    dev = DeviceBytes(np.concatenate([base ^ np.uint8(37 * k % 256) for k in range(E // eb)], axis=1))
    te, tr, st = _flags(312, T, E, 0.02, 0.01)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, hf.hf_range(313, (T, E), -1, 1), te, tr, st)
    eng.finish_rollout()
    dev.free()

    def new_read():
        return eng.batch_stats()

    def plane_reads():
        return [eng.read_batch(k) for k in ("values", "returns", "advantages", "masks")]

    def old_read():
        return br.reference(*plane_reads())[0]

    for _ in range(10):  # warm-up: scratch growth, first launches
        a, b = new_read(), old_read()
    assert all(abs(a[k] - b[k]) <= 1e-6 * max(1.0, abs(b[k])) or (np.isnan(a[k]) and np.isnan(b[k])) for k in br.NAMES)
    ts = {"batch_stats_read": [], "four_plane_reads_and_numpy": [], "four_plane_reads_alone": []}
    for _ in range(reps):
        for name, fn in (("batch_stats_read", new_read), ("four_plane_reads_and_numpy", old_read),
                         ("four_plane_reads_alone", plane_reads)):
            t0 = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t0)
    out[f"{E}x{T}_{prec}"] = {k: summary(v) for k, v in ts.items()}
    eng.close()
print(json.dumps(out))
