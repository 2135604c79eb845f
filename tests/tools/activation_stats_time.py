"""developer tool: what aleppo_activation_stats costs at the benched shape (128 environments x T = 128, max_minibatch =
4096, bf16, H = 512, A = 4: a batch of 16384 samples in four forward chunks).
`python tests/tools/activation_stats_time.py [processes] [reps] [--ms-per-step X]`.  Every process is fresh (a child of this
script, with a time limit; a failed child ends the tool, nothing is tried again), creates one context, loads a batch of
random observations, warms both sources up (scratch allocation, first launches) and then measures, per call:
  batch_source_ms     host clock around aleppo_activation_stats(NULL, 0): four forward passes, four read-only passes, the
                      finalising launch, the stream's synchronise and the two copies
  caller_source_ms    the same around the caller source at n = 4096 (one chunk; the 115 MB of observations cross PCIe)
  pass_ms             the read-only pass of ONE chunk of 4096 samples alone, from the library's device events (kernel class
                      act_stats), and the forward pass of the same chunk (classes conv_fwd + fc_fwd) beside it
The pass is set against its HBM floor, computed here from the shapes: it reads 2 (12800 + 5184 + 3136) + 4 H bytes per
sample once; the peak is the 8 TB/s of the data sheet (6.3 TB/s is what a plain copy reaches).  --ms-per-step: the
rollout + update time of a bench.py run taken in the same session, for the call's share of it.  Reported: the median of
the process medians and their spread (min .. max).  Prints one JSON line."""
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
PEAK_HBM_GBS = 8000.0
KEYS = ("batch_source_ms", "caller_source_ms", "pass_ms", "forward_ms")


def pass_bytes(n, h=H, elem=2):
    """what the read-only pass has to read for n samples: the three conv activations in T and the fp32 fc output"""
    return n * (elem * (12800 + 5184 + 3136) + 4 * h)


def child(reps):
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    rng = np.random.default_rng(0)
    n = E * T
    obs = rng.integers(0, 256, (n, 4, 84, 84), dtype=np.uint8)
    logp = np.full((n, A), -np.log(A), np.float32)
    eng.set_batch(obs, rng.integers(0, A, n), logp, rng.standard_normal(n).astype(np.float32),
                  rng.standard_normal(n).astype(np.float32), np.ones(n, np.uint8))
    first = np.ascontiguousarray(obs[:MAXB])
    for _ in range(3):
        eng.activation_stats(raw=True)
        eng.activation_stats(first, raw=True)
    ts = {k: [] for k in KEYS}
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.activation_stats(raw=True)
        ts["batch_source_ms"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.activation_stats(first, raw=True)
        ts["caller_source_ms"].append((time.perf_counter() - t0) * 1e3)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        eng.activation_stats(raw=True)
    ms, launches = eng.profile_read("act_stats")
    assert launches == 4 * reps, launches
    fwd = sum(eng.profile_read(k)[0] for k in ("conv_fwd", "fc_fwd"))
    eng.profile(False)
    eng.close()
    out = {k: float(np.median(v)) for k, v in ts.items() if v}
    out.update(pass_ms=ms, forward_ms=fwd)
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
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=E * T), processes=procs, reps=reps)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    b = pass_bytes(MAXB)
    gbs = b / (out["pass_ms"]["median"] * 1e-3) / 1e9
    out["pass"] = dict(chunk_samples=MAXB, bytes=b, hbm_floor_ms=round(b / (PEAK_HBM_GBS * 1e9) * 1e3, 4),
                       achieved_GBps=round(gbs, 1), peak_GBps=PEAK_HBM_GBS, frac_of_peak=round(gbs / PEAK_HBM_GBS, 4))
    if per_step is not None:
        out["rollout_plus_update_ms"] = per_step
        out["batch_source_share"] = round(out["batch_source_ms"]["median"] / per_step, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
