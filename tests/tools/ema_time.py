"""developer tool: what one update of the exponentially averaged parameters costs at the benched shape (128 environments x
T = 128, max_minibatch = 4096, bf16, H = 512, A = 4).
`python tests/tools/ema_time.py [processes] [reps] [--ms-per-step X]`.  Every process is fresh (a child of this script, with
a time limit; a failed child ends the tool, nothing is tried again), creates one context with hashed parameters, opens the
average, warms the call up (first launches) and then measures, per call:
  ema_update_ms   host clock around aleppo_ema_update + aleppo_synchronize: the streaming pass, the finalising launch of the
                  statistics, two launch latencies and the synchronise
  pass_ms         the streaming pass alone, from the library's device events (kernel class ema)
The bytes the pass moves follow from the shape: per padded element 4 (P read) + 4 (average read) + 4 (average written) + 2
(bf16 compute copy written) = 14 in bf16, 12 in fp32; pass_gb_s = bytes / pass_ms.
--ms-per-step: the rollout + update time of a bench.py run taken in the same session, for the share of one update per
rollout.  Reported: the median of the process medians and their spread (min .. max).  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))

E, T, A, H, MAXB = 128, 128, 4, 512, 4096
KEYS = ("ema_update_ms", "pass_ms")


def padded_elements(h, a):
    sizes = ((a + 1) * h, a + 1, h * 3136, h, 64 * 576, 64, 64 * 512, 64, 32 * 256, 32)
    return sum((s + 63) // 64 * 64 for s in sizes)


def child(reps):
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    eng.load_params(hf.fill_params(9100, H, A))
    eng.ema_open()
    for _ in range(5):
        eng.ema_update(0.999)
    eng.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.ema_update(0.999)
        eng.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        eng.ema_update(0.999)
    ms, launches = eng.profile_read("ema")
    assert launches == reps, launches
    eng.profile(False)
    stats = eng.ema_stats()
    eng.close()
    print(json.dumps(dict(ema_update_ms=float(np.median(ts)), pass_ms=ms, updates=stats["updates"])))


def main():
    argv = sys.argv[1:]
    per_step = None
    if "--ms-per-step" in argv:
        i = argv.index("--ms-per-step")
        per_step = float(argv[i + 1])
        del argv[i:i + 2]
    procs = int(argv[0]) if argv else 3
    reps = int(argv[1]) if len(argv) > 1 else 50
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    n = padded_elements(H, A)
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", padded_elements=n), processes=procs,
               reps=reps, bytes_per_element=14, pass_bytes=14 * n)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 5), min=round(float(m.min()), 5), max=round(float(m.max()), 5))
    out["pass_gb_s"] = round(14 * n / (out["pass_ms"]["median"] * 1e-3) / 1e9, 1)
    if per_step is not None:
        out["rollout_plus_update_ms"] = per_step
        out["ema_update_share_of_a_step"] = round(out["ema_update_ms"]["median"] / per_step, 6)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
