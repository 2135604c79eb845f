"""developer tool: what aleppo_refresh_advantages costs at the benched shape (128 environments x T = 128, max_minibatch =
4096, bf16, H = 512, A = 4: 16384 samples in four forward chunks, then the 128 post-rollout observations), next to one
epoch of the update it sits in front of.  `python tests/tools/refresh_time.py [processes] [reps]`.  Every process is fresh (a
child of this script, with a time limit; a failed child ends the tool, nothing is tried again), creates one context with
hashed parameters, replays one hashed rollout and finishes it, warms both calls up and then measures with profiling off,
alternating the two calls so that clock and thermal drift hit them alike (the clocks are as the machine left them: nothing is
pinned), per call:
  refresh_ms        host clock around aleppo_refresh_advantages(LIVE) with the statistics: the synchronise, per chunk the
                    forward pass and the value launch, the two statistics launches, the GAE scan, one copy of 13 doubles.
                    The call ends in a stream synchronise.
  refresh_nostat_ms the same with stats = NULL
  train_epoch_ms    host clock around aleppo_train(lr, 1, 4): one epoch over the same 16384 samples (it synchronises too)
and, in a separate pass with profiling on, from the library's device events per refresh:
  forward_ms        the five forward passes (classes conv_fwd + fc_fwd, or conv1_fwd .. conv3_fwd + fc_fwd)
  value_ms          the five value launches and the two statistics launches (class act_stats)
  gae_ms            the scan (class gae)
  rest_ms           refresh_ms - forward_ms - value_ms - gae_ms: the synchronise, the copy and the launch latencies
Reported: the median of the process medians and their spread (min .. max).  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))

E, T, A, H, MAXB, M = 128, 128, 4, 512, 4096, 4
N = E * T
LR = 2.5e-4
KEYS = ("refresh_ms", "refresh_nostat_ms", "train_epoch_ms", "forward_ms", "value_ms", "gae_ms", "rest_ms")
FWD_CLASSES = ("conv_fwd", "fc_fwd", "conv1_fwd", "conv2_fwd", "conv3_fwd")


def child(reps):
    import ctypes
    import hashfill as hf
    import refresh_ref as rf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB, seed=3)
    eng.load_params(hf.fill_params(9400, H, A))
    hip = ctypes.CDLL("libamdhip64.so")
    base = hf.hf_bytes(9401, (T, 32, 84, 84))  # (a block of environments, byte-permuted across the rest)
    frames = np.ascontiguousarray(np.concatenate([base ^ np.uint8(37 * k % 256) for k in range(E // 32)], axis=1))
    ptr = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(frames.nbytes)) == 0
    assert hip.hipMemcpy(ptr, frames.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(frames.nbytes), 1) == 0
    te, tr, st = rf.row_flags(9402, E, T, p=0.03)
    eng.replay_rollout(ptr.value, pkg.FRAMES_84, E * 7056, rf.row_rewards(9403, E, T), te, tr, st)
    eng.finish_rollout()

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    calls = (lambda: eng.refresh_advantages(), lambda: eng.refresh_advantages(stats=False), lambda: eng.train(LR, 1, M))
    for _ in range(3):  # warm-up: every shape the timed window uses
        for f in calls:
            f()
    times = [[], [], []]
    for _ in range(reps):
        for k, f in enumerate(calls):
            times[k].append(timed(f))
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        stats = eng.refresh_advantages()
    per = {}
    for k in FWD_CLASSES + ("act_stats", "gae"):
        ms, launches = eng.profile_read(k)
        per[k] = (ms * launches / reps, launches / reps)
    assert per["act_stats"][1] == N // MAXB + 1 and per["gae"][1] == 1, per  # a bracket per chunk; the last holds the statistics
    eng.profile(False)
    eng.close()
    assert hip.hipFree(ptr) == 0
    r = float(np.median(times[0]))
    fwd = sum(per[k][0] for k in FWD_CLASSES)
    print(json.dumps(dict(refresh_ms=r, refresh_nostat_ms=float(np.median(times[1])),
                          train_epoch_ms=float(np.median(times[2])), forward_ms=fwd, value_ms=per["act_stats"][0],
                          gae_ms=per["gae"][0], rest_ms=r - fwd - per["act_stats"][0] - per["gae"][0], stats=stats)))


def main():
    argv = sys.argv[1:]
    procs = int(argv[0]) if argv else 3
    reps = int(argv[1]) if len(argv) > 1 else 30
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=400)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=N), processes=procs, reps=reps,
               stats=runs[0]["stats"])
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    out["refresh_over_train_epoch"] = round(out["refresh_ms"]["median"] / out["train_epoch_ms"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
