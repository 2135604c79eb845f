"""developer tool: what aleppo_policy_diff costs at the benched shape (128 environments x T = 128, max_minibatch = 4096,
bf16, H = 512, A = 4; the batch source: 16384 samples in four forward chunks), next to the routes a user had before it.
`python tests/tools/policy_diff_time.py [processes] [reps]`.  Every process is fresh (a child of this script, with a time
limit; a failed child ends the tool, nothing is tried again), creates one context with hashed parameters in the snapshot,
a hashed perturbation of them live and a hashed caller batch, warms every route up and then measures, alternating the
routes so that clock and thermal drift hit them alike (the clocks are as the machine left them: nothing is pinned), per call:
  call_ms          host clock around aleppo_policy_diff(NULL, 0, SNAPSHOT, LIVE), stats only: the synchronise, per chunk two
                   forward passes, two head launches, one device copy of set a's fc rows (8 MB), the comparison and the
                   finalising launch; one copy of 16 doubles.  The call ends in a stream synchronise.
  forward_ms       (a) the eight forward passes alone, from the library's device events (classes conv_fwd + fc_fwd)
  compare_ms       (b) the comparison and finalising launches of the four chunks, from the library's device events (class
                   act_stats); compare_gbs: the two fc reads (2 x 16384 x 512 x 4 = 67 MB) over it
  rest_ms          (c) call_ms - forward_ms - compare_ms: the head launches, the device copies, the synchronise and the launch
                   latencies
  snapshot_take_ms host clock around aleppo_snapshot_take(LIVE) + aleppo_synchronize (two device copies of the parameters)
  forward_route_ms (d) the route without the call, policy and value only: aleppo_forward over the 16384 observations in
                   chunks of max_minibatch on the live set, aleppo_load_params of the other set, the same sweep again,
                   aleppo_load_params back (the observations cross to the device twice, every logit comes back), plus the
                   numpy reference (tests/policy_diff_ref.py) with a one-column stand-in for the features, which
                   aleppo_forward does not return; reference_ms: the numpy part alone
  full_route_ms    (e) the same with aleppo_forward_activations(fc) in both sweeps as well (2 x 33.6 MB of features come
                   back), and the reference on the real features: everything the call reports
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

E, T, A, H, MAXB = 128, 128, 4, 512, 4096
N = E * T
KEYS = ("call_ms", "forward_ms", "compare_ms", "rest_ms", "snapshot_take_ms", "forward_route_ms", "full_route_ms",
        "reference_ms")


def child(reps):
    import hashfill as hf
    import policy_diff_ref as pdr
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=MAXB)
    pa = hf.fill_params(9100, H, A)
    pb = (pa + np.float32(0.02) * hf.hf_range(9105, pa.shape, -1, 1) * np.abs(pa)).astype(np.float32)
    eng.load_params(pa)
    eng.snapshot_take("live")
    eng.load_params(pb)
    base = hf.hf_bytes(9101, (MAXB, 4, 84, 84))  # (one hashed chunk, its copies made distinct by a per-chunk mask)
    obs = np.concatenate([base ^ np.uint8(17 * k) for k in range(N // MAXB)])
    eng.set_batch(obs, (hf.hf_u32(9102, N) % np.uint32(A)).astype(np.int64), np.full((N, A), -np.log(A), np.float32),
                  hf.hf_range(9103, (N,), -1, 1), hf.hf_range(9104, (N,), -1, 1), np.ones(N, np.uint8))

    def sweep(features):
        l, v, h = [], [], []
        for i in range(0, N, MAXB):
            a, b = eng.forward(obs[i:i + MAXB])
            l.append(a)
            v.append(b)
            if features:
                h.append(eng.forward_activations(obs[i:i + MAXB], layers=("fc",))["fc"])
        return np.concatenate(l), np.concatenate(v), np.concatenate(h) if features else np.ones((N, 1), np.float32)

    def route(features):
        t0 = time.perf_counter()
        fb = sweep(features)  # live = set b
        eng.load_params(pa)
        fa = sweep(features)
        eng.load_params(pb)
        t1 = time.perf_counter()
        ref = pdr.reference(*fa, *fb)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3, ref

    def call():
        t0 = time.perf_counter()
        got = eng.policy_diff("snapshot", "live")
        return (time.perf_counter() - t0) * 1e3, got

    for _ in range(3):
        first = eng.policy_diff("snapshot", "live", per_sample=True, transitions=True)
    ref = route(True)[2]  # (warm-up; it also shows that both routes see the same comparison)
    route(False)
    bad, worst = pdr.check(np.array([first["stats"][k] for k in pdr.STATS]), first["per_sample"], first["transitions"], ref)
    assert not bad, bad
    calls, light, full, refs, takes = [], [], [], [], []
    for k in range(reps):
        calls.append(call()[0])
        if k < max(1, min(reps, 3)):
            r = route(False)
            light.append(r[0])
            r = route(True)
            full.append(r[0])
            refs.append(r[1])
        t0 = time.perf_counter()
        eng.snapshot_take("live")  # (live is set b: set a is put back below)
        eng.synchronize()
        takes.append((time.perf_counter() - t0) * 1e3)
        eng.load_snapshot(pa)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        eng.policy_diff("snapshot", "live")
    cmp_ms, launches = eng.profile_read("act_stats")
    assert launches == 4 * reps, launches
    fwd_ms = sum(eng.profile_read(k)[0] * eng.profile_read(k)[1] for k in ("conv_fwd", "fc_fwd", "conv1_fwd", "conv2_fwd",
                                                                             "conv3_fwd")) / reps
    cmp_ms = cmp_ms * launches / reps
    eng.profile(False)
    eng.close()
    c = float(np.median(calls))
    print(json.dumps(dict(call_ms=c, forward_ms=fwd_ms, compare_ms=cmp_ms, rest_ms=c - fwd_ms - cmp_ms,
                          snapshot_take_ms=float(np.median(takes)), forward_route_ms=float(np.median(light)),
                          full_route_ms=float(np.median(full)), reference_ms=float(np.median(refs)), stats=first["stats"],
                          worst_of_bound=worst)))


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
               feature_bytes=2 * N * H * 4, stats=runs[0]["stats"], worst_of_bound=max(r["worst_of_bound"] for r in runs))
    for k in KEYS:
        m = np.array([r[k] for r in runs])
        out[k] = dict(median=round(float(np.median(m)), 4), min=round(float(m.min()), 4), max=round(float(m.max()), 4))
    out["compare_gbs"] = round(out["feature_bytes"] / out["compare_ms"]["median"] / 1e6, 1)
    out["speedup_over_the_forward_route"] = round(out["forward_route_ms"]["median"] / out["call_ms"]["median"], 1)
    out["speedup_over_the_full_route"] = round(out["full_route_ms"]["median"] / out["call_ms"]["median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
