"""developer tool: what the gradient probes cost at the benched shape (128 environments x T = 128, max_minibatch = 4096,
bf16, H = 512, A = 4), next to what they mirror and the route a user had before them.
`python tests/tools/grad_probe_time.py [processes] [reps]`.  Every process is fresh (a child of this script, with a time
limit; a failed child ends the tool, nothing is tried again), creates one context with hashed parameters and a hashed
caller batch, warms every route up and then measures, alternating the routes so that clock and thermal drift hit them
alike (the clocks are as the machine left them: nothing is pinned), per call:
  probe_ms          host clock around aleppo_grad_probe(slot, 0, 4096, NULL): the synchronise, the minibatch's forward, head,
                    backward and slab reduces, one copy of the count, the synchronise
  step_ms           host clock around aleppo_train(lr, 1, 4) over the 16384 samples, divided by its 4 minibatches: the step
                    the probe mirrors, with the norm pass and Adam, without a synchronise per minibatch
  probe_kernels_ms  the probe's launches from the library's device events, summed over the update's kernel classes
  step_kernels_ms   the same classes (and adam) per minibatch of aleppo_train; the two streams overlap, so a sum of classes
                    is more than the wall time of either
  gram2_ms, gram4_ms     host clock around aleppo_grad_gram of 2 / 4 slots: the partial pass, the one-workgroup second
                    stage, the synchronise, one copy; gram2_kernels_ms / gram4_kernels_ms: the two launches from the device
                    events (class act_stats); gram*_gbs: k vectors of the padded layout over the kernel time
  tensor_stats_ms   host clock around aleppo_tensor_stats(PARAMS | STEP): the pass of the same structure over four vectors
  interference_ms   Engine.gradient_interference on 4096 samples end to end: three probes, one Gram of three slots, the host
                    arithmetic
  host_route_ms     what it replaces, on a batch of the same 4096 samples: three times aleppo_train(lr = 0, 1, 1) +
                    aleppo_export_grads (1.7 M floats through the export permutation), then the per-tensor inner products
                    in numpy - which advances Adam's moments and step three times and cannot separate the loss terms
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
UPDATE_CLASSES = ("head", "conv_fwd", "conv1_fwd", "conv2_fwd", "conv3_fwd", "fc_fwd", "fc_dgrad", "fc_wgrad", "conv3_dgrad",
                  "conv3_wgrad", "conv2_dgrad", "conv2_wgrad", "conv1_wgrad", "conv_bwd", "reduce", "adam")
KEYS = ("probe_ms", "step_ms", "probe_kernels_ms", "step_kernels_ms", "gram2_ms", "gram4_ms", "gram2_kernels_ms",
        "gram4_kernels_ms", "tensor_stats_ms", "interference_ms", "host_route_ms")


def _clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def child(reps):
    import grad_probe_ref as gp
    import update_harness as uh
    from __graft_entry__ import load_package
    import hashfill as hf
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    eng.load_params(hf.fill_params(9300, H, A))
    batch = uh.hashed_batch(9301, N, A, mask_p=0.1, distinct=N // MAXB)
    eng.set_batch(*batch)
    lr = 1e-5
    spans = gp.bounds(H, A)

    def kernels(run, count):
        eng.profile(True)
        eng.profile_reset()
        for _ in range(count):
            run()
        ms = sum(eng.profile_read(k)[0] * eng.profile_read(k)[1] for k in UPDATE_CLASSES) / count
        eng.profile(False)
        return ms

    def gram_kernels(slots, count):
        eng.profile(True)
        eng.profile_reset()
        for _ in range(count):
            eng.grad_gram(slots, raw=True)
        ms, launches = eng.profile_read("act_stats")
        eng.profile(False)
        assert launches == count, launches
        return ms

    for _ in range(3):  # warm-up: every route once
        eng.train(lr, 1, M)
        for s in range(4):
            eng.grad_probe(s, 0, MAXB)
        eng.grad_gram([0, 1, 2, 3], raw=True)
        eng.tensor_stats("all", raw=True)
    out = {k: [] for k in KEYS}
    for _ in range(reps):
        out["probe_ms"].append(_clock(lambda: eng.grad_probe(0, 0, MAXB)))
        out["step_ms"].append(_clock(lambda: eng.train(lr, 1, M)) / M)
        out["gram2_ms"].append(_clock(lambda: eng.grad_gram([0, 1], raw=True)))
        out["gram4_ms"].append(_clock(lambda: eng.grad_gram([0, 1, 2, 3], raw=True)))
        out["tensor_stats_ms"].append(_clock(lambda: eng.tensor_stats("all", raw=True)))
    out["probe_kernels_ms"].append(kernels(lambda: eng.grad_probe(0, 0, MAXB), reps))
    out["step_kernels_ms"].append(kernels(lambda: eng.train(lr, 1, M), reps) / M)
    out["gram2_kernels_ms"].append(gram_kernels([0, 1], reps))
    out["gram4_kernels_ms"].append(gram_kernels([0, 1, 2, 3], reps))
    # the two routes to the interference figures, on the same 4096 samples
    eng.set_batch(*(a[:MAXB] for a in batch))

    def host_route():
        g = []
        for _ in range(3):
            eng.train(0.0, 1, 1)
            g.append(eng.export_grads().astype(np.float64))
        return [[[float(g[i][b:e] @ g[j][b:e]) for j in range(3)] for i in range(3)] for b, e in spans]

    eng.gradient_interference(0, MAXB)
    host_route()
    for _ in range(max(1, min(reps, 5))):
        out["interference_ms"].append(_clock(lambda: eng.gradient_interference(0, MAXB)))
        out["host_route_ms"].append(_clock(host_route))
    eng.close()
    print(json.dumps({k: float(np.median(v)) for k, v in out.items()}))


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
    import grad_probe_ref as gp
    padded = sum((n + 63) // 64 * 64 for n in (gp.sizes(H, A)[:8] + [(A + 1) * H, A + 1]))  # the ten internal tensors
    out = dict(shape=dict(E=E, T=T, A=A, H=H, max_minibatch=MAXB, precision="bf16", samples=N, probe_samples=MAXB),
               processes=procs, reps=reps, vector_bytes=padded * 4)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    for k in (2, 4):
        out[f"gram{k}_gbs"] = round(k * padded * 4 / out[f"gram{k}_kernels_ms"]["median"] / 1e6, 1)
    out["probe_over_step"] = round(out["probe_ms"]["median"] / out["step_ms"]["median"], 2)
    out["speedup_over_the_host_route"] = round(out["host_route_ms"]["median"] / out["interference_ms"]["median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
