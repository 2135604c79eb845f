"""developer tool: what ALEPPO_OPT_REWARD_SCALE costs in aleppo_finish_rollout, and that the option-off path costs what it
did - at two rollout shapes: 128 envs x T = 128 (bf16 network) and 4096 envs x T = 5 (fp32, v1.yaml's shape).
`python tests/tools/reward_scale_time.py [reps] [off]`.  One context per shape; every repetition replays a recorded rollout
(not timed) and then times aleppo_finish_rollout with the host clock (the call ends in a stream synchronise) and reads
ALEPPO_K_GAE's device time of that one launch group; the option is off and on in alternate calls.  With ALEPPO_LIB_PATH
naming an older build's library (one without the option), or with `off` as the second argument, only the off path is
measured (never setting the option): run the two builds that way in alternate processes of one session and compare the
medians against the older build's own process-to-process spread.  Prints one JSON
line: per shape and path the median, minimum and 10th / 90th percentiles over `reps` (default 60) repetitions."""
import ctypes
import json
import os
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))
import hashfill as hf  # noqa: E402
import reward_scale_ref as rr  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_gpu_at_size import DeviceBytes  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
off_only = len(sys.argv) > 2 and sys.argv[2] == "off"  # like for like against a build without the option
pkg = load_package()
_so = ctypes.CDLL(pkg.LIB_PATH)
has_option = hasattr(_so, "aleppo_reward_scale")
pkg.EXPORTS[:] = [n for n in pkg.EXPORTS if hasattr(_so, n)]  # (an older build's library lacks the newest entry points)


def summary(ts):
    v = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(float(v[0]), 1),
                p10_us=round(float(v[len(v) // 10]), 1), p90_us=round(float(v[len(v) * 9 // 10]), 1))


out = {"reps": reps, "library": os.path.basename(os.path.dirname(pkg.LIB_PATH)) + "/" + os.path.basename(pkg.LIB_PATH),
       "has_option": has_option}
for E, T, prec, H in ((128, 128, "bf16", 512), (4096, 5, "fp32", 32)):
    eng = pkg.Engine(E, T, 4, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
    eng.load_params(hf.fill_params(310, H, 4))
    eb = min(E, 128)
    base = hf.hf_bytes(311, (T, eb, 84, 84))
    dev = DeviceBytes(np.concatenate([base ^ np.uint8(37 * k % 256) for k in range(E // eb)], axis=1))
    r, te, tr, st, _ = rr.generate(312, E, T)
    eng.profile(True)
    modes = ("off", "on") if has_option and not off_only else ("off",)
    ts = {m: [] for m in modes}
    dev_ts = {m: [] for m in modes}
    for i in range(reps + 5):  # (five warm-up rounds: first launches, the state's allocation)
        for m in modes:
            if has_option:
                eng.set_option(pkg.OPT_REWARD_SCALE, int(m == "on"))
            eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, r, te, tr, st)
            eng.profile_reset()
            t0 = time.perf_counter()
            eng.finish_rollout()
            dt = time.perf_counter() - t0
            ms, n = eng.profile_read("gae")
            assert n == 1
            if i >= 5:
                ts[m].append(dt)
                dev_ts[m].append(ms * 1e-3)
    dev.free()
    out[f"{E}x{T}_{prec}"] = {m: dict(finish_rollout=summary(ts[m]), k_gae=summary(dev_ts[m])) for m in modes}
    eng.close()
print(json.dumps(out))
