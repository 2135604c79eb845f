"""developer tool: what aleppo_feature_rank costs at the benched shape (128 environments x T = 128, max_minibatch = 4096,
bf16, H = 512, A = 4; the batch source: 16384 samples in four forward chunks), next to the route it replaces.
`python tests/tools/feature_rank_time.py [processes] [reps]`.  Every process is fresh (a child of this script, with a time
limit; a failed child ends the tool, nothing is tried again), creates one context with hashed parameters and a hashed
caller batch, warms both routes up and then measures, per call:
  call_ms      host clock around aleppo_feature_rank(NULL, 0): the synchronise, four forward passes, four times the three
               read-only launches, one copy of G and s (1.2 MB), the host solve
  forward_ms   (a) the four forward passes alone, from the library's device events (HIP events; classes conv_fwd + fc_fwd)
  gram_ms      (b) the flags, Gram and reduce launches of the four chunks, from the library's device events (class act_stats)
  host_ms      (c) the copy and the host solve: call_ms - forward_ms - gram_ms (it also holds the launch latencies)
  svd_route_ms (d) forward_activations(fc) over the same 16384 observations in chunks of max_minibatch (the observations
               cross to the device, 32 MB of features come back) plus numpy.linalg.svd(compute_uv=False) of the float64
               [16384, 512] matrix; svd_ms: the SVD alone
The Gram arithmetic with symmetry: 36 of 64 blocks x 64 x 64 x 16384 rows x 2 = 4.83 GFLOP (4.3 GFLOP is the exact
triangle); the features read: 16384 x 512 x 4 = 33.6 MB per pass over them.  Reported: the median of the process medians
and their spread (min .. max).  Prints one JSON line."""
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
N = E * T
KEYS = ("call_ms", "forward_ms", "gram_ms", "host_ms", "svd_route_ms", "svd_ms")


def child(reps):
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    eng.load_params(hf.fill_params(9100, H, A))
    base = hf.hf_bytes(9101, (MAXB, 4, 84, 84))  # (one hashed chunk, its copies made distinct by a per-chunk mask)
    obs = np.concatenate([base ^ np.uint8(17 * k) for k in range(N // MAXB)])
    eng.set_batch(obs, (hf.hf_u32(9102, N) % np.uint32(A)).astype(np.int64), np.full((N, A), -np.log(A), np.float32),
                  hf.hf_range(9103, (N,), -1, 1), hf.hf_range(9104, (N,), -1, 1), np.ones(N, np.uint8))

    def svd_route():
        t0 = time.perf_counter()
        phi = np.concatenate([eng.forward_activations(obs[i:i + MAXB], layers=("fc",))["fc"] for i in range(0, N, MAXB)])
        t1 = time.perf_counter()
        sv = np.linalg.svd(phi.astype(np.float64), compute_uv=False)
        return (time.perf_counter() - t0) * 1e3, (time.perf_counter() - t1) * 1e3, sv

    for _ in range(3):
        first = eng.feature_rank(spectrum=True)
    route, svd, sv = svd_route()  # (warm-up; it also shows that both routes see the same spectrum)
    assert abs(first["sigma"][0] - sv[0]) <= 1e-6 * sv[0], (first["sigma"][0], sv[0])
    calls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.feature_rank()
        calls.append((time.perf_counter() - t0) * 1e3)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        eng.feature_rank()
    gram_ms, launches = eng.profile_read("act_stats")
    assert launches == 4 * reps, launches
    fwd_ms = sum(eng.profile_read(k)[0] * eng.profile_read(k)[1] for k in ("conv_fwd", "fc_fwd", "conv1_fwd", "conv2_fwd",
                                                                             "conv3_fwd")) / reps
    gram_ms = gram_ms * launches / reps
    eng.profile(False)
    routes = [svd_route()[:2] for _ in range(max(1, min(reps, 3)))]
    eng.close()
    call = float(np.median(calls))
    print(json.dumps(dict(call_ms=call, forward_ms=fwd_ms, gram_ms=gram_ms, host_ms=call - fwd_ms - gram_ms,
                          svd_route_ms=float(np.median([r[0] for r in routes])), svd_ms=float(np.median([r[1] for r in routes])),
                          stats=first["stats"])))


def main():
    argv = sys.argv[1:]
    procs = int(argv[0]) if argv else 3
    reps = int(argv[1]) if len(argv) > 1 else 10
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=400)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=N), processes=procs, reps=reps,
               gram_gflop=36 * 64 * 64 * N * 2 / 1e9, feature_bytes=N * H * 4, stats=runs[0]["stats"])
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    out["gram_tflops"] = round(out["gram_gflop"] / out["gram_ms"]["median"], 3)
    out["speedup_over_the_svd_route"] = round(out["svd_route_ms"]["median"] / out["call_ms"]["median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
