"""developer tool: what the regularised optimizer step and aleppo_shrink_perturb cost at the benched shape (128 environments x
T = 128, 4 minibatches of 4096, bf16, H = 512, A = 4).

`python tests/tools/reg_time.py [processes] [reps]`: every process is fresh (a child of this script, with a time limit; a
failed child ends the tool, nothing is tried again), creates one context with hashed parameters and a hashed anchor, warms
every call up and then measures
  update_plain_ms / update_reg_ms   host clock around aleppo_train (1 epoch x 4 minibatches; it waits for the device), the
                  coefficients zero / non-zero, the calls alternating so that clock drift hits both alike
  sp_pass_ms      aleppo_shrink_perturb's pass alone, from the library's device events (kernel class recycle)
  sp_call_ms      host clock around the whole call: the pass, the rebuilt compute copies, the synchronise
  recycle_pass_ms / recycle_call_ms   the same two for aleppo_recycle_units on a mask of a quarter of the units
The step kernels themselves are timed from a kernel trace of their own, which holds both entry points because the child
alternates them:
  rocprofv3 --kernel-trace --stats -d OUT -o reg --output-format csv -- python tests/tools/reg_time.py --child 20
  python tests/tools/reg_time.py --stats OUT
--stats reads the trace's kernel summary and prints, for adam_kernel and reg_step_kernel, calls, mean / min duration and the
bytes over the mean.  Bytes per padded element, bf16: adam_kernel 4 x 4 read (G, M1, M2, P) + 3 x 4 written (M1, M2, P) + 2
(compute copy) = 30, plus 2 for every element of fc.w / conv3.w / conv2.w (the transposed layouts); reg_step_kernel the same
plus 4 (the anchor): the one expectation is that one more fp32 stream.  Prints one JSON line."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))

E, T, A, H, M = 128, 128, 4, 512, 4
KEYS = ("update_plain_ms", "update_reg_ms", "sp_pass_ms", "sp_call_ms", "recycle_pass_ms", "recycle_call_ms")


def sizes(h, a):
    return ((a + 1) * h, a + 1, h * 3136, h, 64 * 576, 64, 64 * 512, 64, 32 * 256, 32)


def padded_elements(h, a):
    return sum((s + 63) // 64 * 64 for s in sizes(h, a))


def step_bytes(h, a, reg):
    transposed = h * 3136 + 64 * 576 + 64 * 512
    return padded_elements(h, a) * (34 if reg else 30) + 2 * transposed


def child(reps):
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=E * T // M)
    eng.load_params(hf.fill_params(9300, H, A))
    eng.load_anchor(hf.fill_params(9301, H, A))
    rng = np.random.default_rng(0)
    N = E * T
    eng.set_batch(rng.integers(0, 256, (N, 4, 84, 84), dtype=np.uint8), rng.integers(0, A, N),
                  np.full((N, A), -np.log(A), np.float32), rng.standard_normal(N).astype(np.float32),
                  rng.standard_normal(N).astype(np.float32), (rng.random(N) > 0.02).astype(np.uint8))
    coef = {"plain": (0.0, 0.0), "reg": (1e-2, 1e-2)}
    ts = {k: [] for k in coef}
    for rep in range(reps + 2):  # (the first two rounds warm up: kernel attribute set-up, storage growth)
        for name, (wd, la) in coef.items():
            eng.set_regularization(weight_decay=wd, anchor_coef=la)
            t0 = time.perf_counter()
            eng.train(2.5e-4, 1, M)
            if rep >= 2:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    mask = (hf.hf_unit(9302, 160 + H) < np.float32(0.25)).astype(np.uint8)
    calls = {"sp": lambda k: eng.shrink_perturb(0.9, 0.01, key=k), "recycle": lambda k: eng.recycle_units(mask, key=k)}
    out = dict(update_plain_ms=float(np.median(ts["plain"])), update_reg_ms=float(np.median(ts["reg"])))
    for name, call in calls.items():
        for k in range(3):
            call(k)
        host = []
        for k in range(reps):
            t0 = time.perf_counter()
            call(k)
            host.append((time.perf_counter() - t0) * 1e3)
        eng.profile(True)
        eng.profile_reset()
        for k in range(reps):
            call(k)
        ms, launches = eng.profile_read("recycle")
        assert launches == reps, launches
        eng.profile(False)
        out[name + "_pass_ms"] = ms
        out[name + "_call_ms"] = float(np.median(host))
    eng.close()
    print(json.dumps(out))


def stats(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if len(files) != 1:
        sys.exit("expected one *kernel_stats.csv under %s, found %d" % (directory, len(files)))
    out = dict(shape=dict(E=E, T=T, A=A, H=H, minibatches=M, precision="bf16", padded_elements=padded_elements(H, A)))
    for row in csv.DictReader(open(files[0])):
        for name, reg in (("adam_kernel", False), ("reg_step_kernel", True)):
            if name in row["Name"]:
                mean, b = float(row["AverageNs"]), step_bytes(H, A, reg)
                out[name] = dict(calls=int(row["Calls"]), mean_us=round(mean / 1e3, 3), min_us=round(float(row["MinNs"]) / 1e3, 3),
                                 bytes=b, gb_s_at_mean=round(b / mean, 1))
    if "adam_kernel" in out and "reg_step_kernel" in out:
        a, r = out["adam_kernel"], out["reg_step_kernel"]
        out["extra_us"] = round(r["mean_us"] - a["mean_us"], 3)
        out["one_more_stream_us_at_adam_rate"] = round(4 * padded_elements(H, A) / a["gb_s_at_mean"] / 1e3, 3)
    print(json.dumps(out))


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            sys.exit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    out = dict(shape=dict(E=E, T=T, A=A, H=H, minibatches=M, precision="bf16", padded_elements=padded_elements(H, A)),
               processes=procs, reps=reps)
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 5), min=round(float(m.min()), 5), max=round(float(m.max()), 5))
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        stats(sys.argv[2])
    else:
        main()
