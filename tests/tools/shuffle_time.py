"""developer tool: cost of ALEPPO_OPT_MINIBATCH_SHUFFLE at the BASELINE configs[1] update shape (128 envs x T = 128, 4 epochs x
4 minibatches of 4096, bf16): `python tests/tools/shuffle_time.py [reps] [both|contiguous|shuffled]`.  aleppo_train waits for
the device before it returns, so each timed call is the whole update; contiguous and shuffled calls alternate (one context,
the option toggled between calls) so that clock / thermal drift hits both alike.  Prints one JSON line.  For per-kernel times
run it on its own under `rocprofv3 --kernel-trace --stats -- python tests/tools/shuffle_time.py 10 shuffled`."""
import json, os, sys, time
import numpy as np
_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))
import hashfill as hf
from __graft_entry__ import load_package
pkg = load_package()
E, T, A, H, M, EP = 128, 128, 4, 512, 4, 4
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
mode = sys.argv[2] if len(sys.argv) > 2 else "both"
modes = {"both": (0, 1), "contiguous": (0,), "shuffled": (1,)}[mode]
eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=E * T // M)
eng.load_params(hf.fill_params(310, H, A))
rng = np.random.default_rng(0)
N = E * T
obs = rng.integers(0, 256, (N, 4, 84, 84), dtype=np.uint8)
eng.set_batch(obs, rng.integers(0, A, N), np.full((N, A), -np.log(A), np.float32), rng.standard_normal(N).astype(np.float32),
              rng.standard_normal(N).astype(np.float32), (rng.random(N) > 0.02).astype(np.uint8))
ts = {m: [] for m in modes}
for m in modes:  # warm-up: first-call kernel attribute set-up, storage growth
    eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, m)
    for _ in range(2):
        eng.train(2.5e-4, EP, M)
for _ in range(reps):
    for m in modes:
        eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, m)
        t0 = time.perf_counter()
        eng.train(2.5e-4, EP, M)
        ts[m].append(time.perf_counter() - t0)
out = {}
for m, name in ((0, "contiguous"), (1, "shuffled")):
    if m in ts:
        v = sorted(ts[m])
        out[name + "_ms_median"] = round(v[len(v) // 2] * 1e3, 3)
        out[name + "_ms_min"] = round(v[0] * 1e3, 3)
if len(modes) == 2:
    out["shuffled_over_contiguous"] = round(out["shuffled_ms_median"] / out["contiguous_ms_median"], 4)
print(json.dumps(out))
eng.close()
