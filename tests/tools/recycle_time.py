"""developer tool: what a recycle costs at the benched shape (128 environments x T = 128, max_minibatch = 4096, bf16,
H = 512, A = 4: 672 units, a batch of 16384 samples in four forward chunks).
`python tests/tools/recycle_time.py [processes] [reps] [--ms-per-step X]`.  Every process is fresh (a child of this script,
with a time limit; a failed child ends the tool, nothing is tried again), creates one context with hashed parameters, loads
a batch of random observations, warms every call up (scratch allocation, first launches) and then measures, per call:
  recycle_dormant_ms  host clock around aleppo_recycle_dormant(NULL, 0): the measurement of aleppo_activation_stats (four
                      forward passes, four read-only passes, the finalising launch), the mask launch, the masked pass, the
                      rebuild of the derived copies, the stream's synchronise and the copy of the mask
  activation_stats_ms the same clock around aleppo_activation_stats(NULL, 0) in the same process, to set it against
  recycle_units_ms    host clock around aleppo_recycle_units with 7 of the 672 units masked (about 1 %: one of conv1, conv2
                      and conv3 each, four of fc): the mask upload, the masked pass, the rebuild, the synchronise
  pass_ms             the masked pass alone, from the library's device events (kernel class recycle), same mask
--ms-per-step: the rollout + update time of a bench.py run taken in the same session, for the share of one recycle_dormant
in recycle_interval rollouts.  Reported: the median of the process medians and their spread (min .. max).  Prints one JSON
line."""
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
INTERVAL = 64  # the trainer's default recycle_interval
KEYS = ("recycle_dormant_ms", "activation_stats_ms", "recycle_units_ms", "pass_ms")


def one_percent_mask():
    m = np.zeros(160 + H, np.uint8)
    m[[1, 32 + 2, 96 + 3, 160 + 4, 160 + 5, 160 + 6, 160 + 7]] = 1
    return m


def child(reps):
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    eng.load_params(hf.fill_params(9100, H, A))
    rng = np.random.default_rng(0)
    n = E * T
    obs = rng.integers(0, 256, (n, 4, 84, 84), dtype=np.uint8)
    logp = np.full((n, A), -np.log(A), np.float32)
    eng.set_batch(obs, rng.integers(0, A, n), logp, rng.standard_normal(n).astype(np.float32),
                  rng.standard_normal(n).astype(np.float32), np.ones(n, np.uint8))
    mask = one_percent_mask()
    for k in range(3):
        eng.activation_stats(raw=True)
        eng.recycle_dormant(key=k)
        eng.recycle_units(mask, key=k)
    ts = {k: [] for k in KEYS}
    recycled = []
    for k in range(reps):
        t0 = time.perf_counter()
        eng.activation_stats(raw=True)
        ts["activation_stats_ms"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        recycled.append(eng.recycle_dormant(key=100 + k)[1]["total"])
        ts["recycle_dormant_ms"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.recycle_units(mask, key=200 + k)
        ts["recycle_units_ms"].append((time.perf_counter() - t0) * 1e3)
    eng.profile(True)
    eng.profile_reset()
    for k in range(reps):
        eng.recycle_units(mask, key=300 + k)
    ms, launches = eng.profile_read("recycle")
    assert launches == reps, launches
    eng.profile(False)
    eng.close()
    out = {k: float(np.median(v)) for k, v in ts.items() if v}
    out.update(pass_ms=ms, recycled_units=recycled)
    print(json.dumps(out))


def main():
    argv = sys.argv[1:]
    per_step = None
    if "--ms-per-step" in argv:
        i = argv.index("--ms-per-step")
        per_step = float(argv[i + 1])
        del argv[i:i + 2]
    procs = int(argv[0]) if argv else 3
    reps = int(argv[1]) if len(argv) > 1 else 20
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=E * T, units=160 + H,
                          masked_units=int(one_percent_mask().sum())), processes=procs, reps=reps)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    out["recycled_units_first_process"] = runs[0]["recycled_units"]
    if per_step is not None:
        out["rollout_plus_update_ms"] = per_step
        out["recycle_dormant_share_at_interval_%d" % INTERVAL] = round(
            out["recycle_dormant_ms"]["median"] / (per_step * INTERVAL), 6)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
