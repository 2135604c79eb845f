"""developer tool: what an open episode recorder adds to a device rollout.  `python tests/tools/recorder_time.py [processes] [rollouts]`.

The protocol of tests/tools/device_env_time.py: at the benchmark's shape (E = 128, T = 128, bf16, H = 512), ms per
aleppo_env_rollout + aleppo_finish_rollout (host clock; finish_rollout ends in a stream synchronise) for 84x84 frames and for
raw pairs, with
  off        no recorder,
  obs        a recorder of environment 0 with the observation plane only,
  both       frames + observation,
the log (capacity T) cleared after every rollout outside the timed region.  Every variant runs in `processes` (default 3)
fresh child processes, the variants alternating; each child times `rollouts` (default 20) rollouts after 3 warm-up rollouts.
The recording children then run 3 more rollouts with profiling on and report the capture kernel's own mean time from HIP
events (kernel class rec_capture).  Prints one JSON line: per variant the per-process medians, their median and spread
(max - min of the process medians), the added microseconds per slot against `off` of the same frame kind, and the capture
kernel's microseconds."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(_T)
sys.path.insert(0, _T)
sys.path.insert(0, ROOT)

E, T, A, H = 128, 128, 4, 512
VARIANTS = tuple(f"{kind}_{rec}" for kind in ("84", "raw") for rec in ("off", "obs", "both"))


def child(variant, rollouts):
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    kind, rec = variant.split("_")
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    eng.env_open(frame_kind=pkg.FRAMES_RAW_PAIR if kind == "raw" else pkg.FRAMES_84)
    if rec != "off":
        eng.rec_open("rollout", index=0, frames=rec == "both", observation=True, capacity=T)

    def rollout():
        eng.env_rollout()
        eng.finish_rollout()
    out, ts = {}, []
    for k in range(3 + rollouts):
        t0 = time.perf_counter()
        rollout()
        if k >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
        if rec != "off":
            assert eng.rec_count("rollout")["rows"] == T
            eng.rec_clear("rollout")
    out["ms"] = ts
    if rec != "off":
        eng.profile(True)
        eng.profile_reset()
        for _ in range(3):
            rollout()
            eng.rec_clear("rollout")
        ms, n = eng.profile_read("rec_capture")
        eng.profile(False)
        out["capture_us"], out["capture_launches"] = float(ms) * 1e3, int(n)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        processes = int(sys.argv[1]) if len(sys.argv) > 1 else 3
        rollouts = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        runs = {v: [] for v in VARIANTS}
        for _ in range(processes):
            for v in VARIANTS:  # alternating: every variant sees the same drift of the machine
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, str(rollouts)],
                                   capture_output=True, text=True, timeout=600, cwd=ROOT)
                if r.returncode:
                    raise SystemExit(f"{v} failed: " + r.stderr[-2000:])
                runs[v].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        out = dict(shape=dict(E=E, T=T, H=H, precision="bf16"), processes=processes, rollouts=rollouts)
        for v, rs in runs.items():
            med = [float(np.median(r["ms"])) for r in rs]
            out[v] = dict(process_medians_ms=[round(m, 3) for m in med], median_ms=round(float(np.median(med)), 3),
                          spread_ms=round(max(med) - min(med), 3))
            if "capture_us" in rs[0]:
                ks = [r["capture_us"] for r in rs]
                out[v]["capture_kernel_us"] = dict(process_means=[round(k, 2) for k in ks], median=round(float(np.median(ks)), 2),
                                                   launches=rs[0]["capture_launches"])
        for v in VARIANTS:
            off = out[v.split("_")[0] + "_off"]["median_ms"]
            out[v]["added_us_per_slot"] = round((out[v]["median_ms"] - off) * 1e3 / T, 2)
        print(json.dumps(out))
