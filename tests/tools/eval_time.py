"""developer tool: what the evaluation lanes cost.  `python tests/tools/eval_time.py [bench repeats] [slot reps]`.

A. a plain `python bench.py` on this build and on the parent's (ale-libtorch-ppo_amd/libaleppo_prev.so from
   tests/tools/build_prev.sh, selected with ALEPPO_LIB_PATH), alternated in one call, `repeats` (default 3) runs of 20 steps
   after 5 warm-up steps each, every run a fresh child process.  The feature adds nothing to that path (a context that never
   calls aleppo_eval_open allocates and enqueues nothing new), so the two must agree within the run-to-run spread of the
   parent's own runs, which is recorded next to them.  Skipped (null) when there is no parent build.
B. the time per evaluation slot, eval_push_frames + eval_act (greedy, frames in host memory), at L = 128 and 4096 lanes,
   bf16, H = 512, beside the time per training slot, aleppo_act + aleppo_step, at E = L on the same build (the act waits for the
   previous step's kernels and its own head; the step only enqueues): host clock, after a warm-up; median, minimum, 10th / 90th percentile.  A plain
   measurement for the record.
Prints one JSON line."""
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
import hashfill as hf  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
PREV = os.path.join(ROOT, "ale-libtorch-ppo_amd", "libaleppo_prev.so")
PARENT_BENCH = ("import runpy, sys; sys.path.insert(0, %r); import __graft_entry__ as g; p = g.load_package(); "
                "p.EXPORTS[:] = [e for e in p.EXPORTS if not e.startswith('aleppo_eval_')]; "
                "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')" % ROOT)


def bench(lib_path):
    env = {k: v for k, v in os.environ.items() if k != "ALEPPO_LIB_PATH"}
    if lib_path:
        env["ALEPPO_LIB_PATH"] = lib_path
    args = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    if lib_path:  # the parent's library lacks the new entry points: the same bench.py, with the package's list of symbols
        # to resolve trimmed to the parent's before the library is loaded
        cmd = [sys.executable, "-c", PARENT_BENCH, os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    if r.returncode:
        raise SystemExit("bench.py failed: " + r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["ms_per_step"]


def summary(ts):
    v = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(float(v[0]), 1),
                p10_us=round(float(v[len(v) // 10]), 1), p90_us=round(float(v[len(v) * 9 // 10]), 1))


out = {"bench_repeats": repeats, "slot_reps": reps, "bench_ms_per_step": None}
if os.path.exists(PREV):
    runs = {"this": [], "parent": []}
    for _ in range(repeats):
        runs["this"].append(bench(None))
        runs["parent"].append(bench(PREV))
    out["bench_ms_per_step"] = {k: dict(runs=[round(x, 4) for x in v], median=round(float(np.median(v)), 4),
                                        spread=round(max(v) - min(v), 4)) for k, v in runs.items()}

pkg = load_package()
for L in (128, 4096):
    H, A, T = 512, 4, 64
    eng = pkg.Engine(L, T, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    eng.eval_open(L)
    frames = hf.hf_bytes(311, (L, 84, 84))
    zeros8, zerosf = np.zeros(L, np.uint8), np.zeros(L, np.float32)

    def eval_slot():
        eng.eval_push_frames(frames, zeros8)
        eng.eval_act("greedy")

    def train_slot(state=[0]):
        eng.act()
        eng.step(frames, zerosf, zeros8, zeros8, zeros8)
        state[0] += 1
        if state[0] == T:  # the buffer is full: the next rollout (its own, untimed, call)
            state[0] = 0
            return True
        return False

    for _ in range(10):
        eval_slot()
        train_slot()
    ts = {"eval_push_frames+eval_act": [], "act+step": []}
    for i in range(reps):
        t0 = time.perf_counter()
        eval_slot()
        ts["eval_push_frames+eval_act"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        full = train_slot()
        ts["act+step"].append(time.perf_counter() - t0)
        if full:
            eng.finish_rollout()
    out[f"L{L}_bf16"] = {k: summary(v) for k, v in ts.items()}
    eng.close()
print(json.dumps(out))
