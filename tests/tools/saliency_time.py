"""developer tool: what aleppo_saliency costs at the benched shape (128 environments x T = 128, max_minibatch = 4096, bf16,
H = 512, A = 4) at the default stride 5: environment 0's 128 samples are 128 x 289 = 36 992 pairs, ten forward chunks.
`python tests/tools/saliency_time.py [processes] [reps]`.  Every process is fresh (a child of this script, with a time
limit; a failed child ends the tool, nothing is tried again), creates one context, loads a batch of random observations,
warms the call up (staging allocation, first launches) and then measures, per call:
  batch_source_ms   host clock around aleppo_saliency(NULL, 0, 128): the unperturbed forward, then per chunk the blur where
                    needed, the blend, the forward pass, the head and the scoring launch, the stream's synchronise, one copy
  blur_ms / perturb_ms / score_ms / forward_ms
                    one launch of each alone, from the library's device events (kernel classes sal_blur, sal_perturb,
                    sal_score; conv_fwd + fc_fwd beside them), averaged over the call's launches
The blend writes 28 224 B per pair; its bandwidth is set against the 6.3 TB/s a plain copy reaches on this chip (DESIGN.md
4i).  The whole call is set against pairs / 4096 forward passes of a full chunk: the rest is what the new kernels, the head
and the copies add.  Reported: the median of the process medians and their spread (min .. max).  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))

E, T, A, H, MAXB, STRIDE = 128, 128, 4, 512, 4096, 5
COPY_GBS = 6300.0
FORWARD_US_4I = 118.7  # the forward pass of one 4096-sample chunk
KEYS = ("batch_source_ms", "blur_ms", "perturb_ms", "score_ms", "forward_ms")


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
    del obs
    for _ in range(2):
        eng.saliency(first=0, n=T, stride=STRIDE)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.saliency(first=0, n=T, stride=STRIDE)
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.profile(True)
    eng.profile_reset()
    eng.saliency(first=0, n=T, stride=STRIDE)
    out = dict(batch_source_ms=float(np.median(ts)))
    launches = {}
    for k in ("sal_blur", "sal_perturb", "sal_score", "conv_fwd", "fc_fwd"):
        ms, launches[k] = eng.profile_read(k)
        out[k] = ms
    eng.profile(False)
    eng.close()
    chunks = -(-T * pkg.saliency_grid(STRIDE) ** 2 // MAXB)
    assert launches["sal_perturb"] == launches["sal_score"] == chunks and launches["conv_fwd"] == chunks + 1, launches  # (the blur runs ahead: one launch here)
    out = dict(batch_source_ms=out["batch_source_ms"], blur_ms=out["sal_blur"], perturb_ms=out["sal_perturb"],
               score_ms=out["sal_score"], forward_ms=out["conv_fwd"] + out["fc_fwd"], blur_launches=launches["sal_blur"])
    print(json.dumps(out))


def main():
    argv = sys.argv[1:]
    procs = int(argv[0]) if argv else 3
    reps = int(argv[1]) if len(argv) > 1 else 10
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    G = (84 + STRIDE - 1) // STRIDE
    pairs = T * G * G
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=T, stride=STRIDE, pairs=pairs,
                          chunks=-(-pairs // MAXB), blur_launches=runs[0]["blur_launches"]), processes=procs, reps=reps)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    # the launches are averages over chunks of which the last is partial: the bytes of an average launch
    per_launch = pairs / out["shape"]["chunks"] * 28224
    gbs = per_launch / (out["perturb_ms"]["median"] * 1e-3) / 1e9
    out["perturb"] = dict(bytes_written_per_launch=int(per_launch), achieved_write_GBps=round(gbs, 1), copy_GBps=COPY_GBS,
                          frac_of_copy=round(gbs / COPY_GBS, 4))
    fwd_only = pairs / MAXB * FORWARD_US_4I * 1e-3
    out["forward_only_ms_at_4i"] = round(fwd_only, 4)
    out["call_over_forward_only"] = round(out["batch_source_ms"]["median"] / fwd_only, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
