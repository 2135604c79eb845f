"""developer tool: wall time per aleppo_tensor_stats call at the flagship learner shape (H = 512, A = 6, bf16), for the
PARAMS section alone (one flat vector read) and for both sections (four: P, G, M1, M2), beside one aleppo_state_digest
call in the same processes - the existing one-pass reader of the same arrays (P, M1, M2, plus the frame stacks).
`python tests/tools/tensor_stats_time.py [processes] [reps]`.  Every process is fresh (a child of this script), creates one
context, runs one update so that the step section is valid, warms the three calls up (scratch allocation, first launches)
and then alternates them `reps` (default 200) times; host clock around calls that end in a stream synchronise.  Reported:
per call the median of the process medians and their spread (min .. max) over `processes` (default 5), and the bytes the
pass reads.  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))

H, A, E, T = 512, 6, 32, 8
CALLS = ("tensor_stats_params", "tensor_stats_both", "state_digest")


def child(reps):
    import hashfill as hf
    from __graft_entry__ import load_package
    from test_tensor_stats import _batch
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    eng.set_batch(*_batch(320, E * T, A))
    eng.train(2.5e-4, 1, 2)
    fns = dict(tensor_stats_params=lambda: eng.tensor_stats("params", raw=True),
               tensor_stats_both=lambda: eng.tensor_stats("all", raw=True), state_digest=eng.state_digest)
    for _ in range(10):
        for name in CALLS:
            fns[name]()
    ts = {name: [] for name in CALLS}
    for _ in range(reps):
        for name in CALLS:
            t0 = time.perf_counter()
            fns[name]()
            ts[name].append(time.perf_counter() - t0)
    padded = sum((int(np.prod(s)) + 63) // 64 * 64 for s in ((A + 1, H), (A + 1,), (H, 3136), (H,), (64, 576), (64,),
                                                               (64, 512), (64,), (32, 256), (32,)))
    eng.close()
    print(json.dumps(dict(medians_us={k: float(np.median(v)) * 1e6 for k, v in ts.items()}, flat_vector_bytes=padded * 4)))


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    vec = runs[0]["flat_vector_bytes"]
    out = dict(shape=dict(H=H, A=A, precision="bf16"), processes=procs, reps=reps,
               bytes_read=dict(tensor_stats_params=vec, tensor_stats_both=4 * vec, state_digest_learner=3 * vec))
    for name in CALLS:
        m = np.array([r["medians_us"][name] for r in runs])
        out[name] = dict(median_of_process_medians_us=round(float(np.median(m)), 1), min_us=round(float(m.min()), 1),
                         max_us=round(float(m.max()), 1))
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
