"""developer tool: cost of ALEPPO_OPT_KL_PENALTY (beta = 0.2) at the BASELINE configs[1] update shape (128 envs x T = 128,
4 epochs x 4 minibatches of 4096, bf16, rollout batch): `python tests/tools/kl_penalty_time.py [reps] [package dir]`.  Two
phases, each alternating the option off / on per call on one context: the whole aleppo_train (host clock; it waits for
the device before it returns) with profiling off, then the head kernel's device time (aleppo_profile_read ALEPPO_K_HEAD,
HIP events) with profiling on; head_train_kl_kernel is profiled under that class.  The package dir
(default: this tree's) lets the same script time another build of the library, which has to have the option for the
`on` rows; without it (`off` only) it times the default path.  Prints one JSON line."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))
import hashfill as hf  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
pkg_dir = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(os.path.dirname(_T), "ale-libtorch-ppo_amd")
spec = importlib.util.spec_from_file_location("aleppo_timed", os.path.join(pkg_dir, "__init__.py"),
                                              submodule_search_locations=[pkg_dir])
pkg = importlib.util.module_from_spec(spec)
sys.modules["aleppo_timed"] = pkg
spec.loader.exec_module(pkg)
has_opt = hasattr(pkg, "OPT_KL_PENALTY")
modes = (0, 1) if has_opt else (0,)

E, T, A, H, M, EP = 128, 128, 4, 512, 4, 4
eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=E * T // M)
eng.load_params(hf.fill_params(310, H, A))
from test_gpu_at_size import DeviceBytes, _flags  # noqa: E402
dev = DeviceBytes(hf.hf_bytes(311, (T, E, 84, 84)))
te, tr, st = _flags(312, T, E, 0.01, 0.0)
eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, hf.hf_range(313, (T, E), -1, 1), te, tr, st)
eng.finish_rollout()
dev.free()


if has_opt:
    eng.set_kl_coef(0.2)


def set_mode(m):
    if has_opt:
        eng.set_option(pkg.OPT_KL_PENALTY, m)


out = {"package": os.path.basename(os.path.dirname(pkg_dir)) or pkg_dir, "kl_penalty_option": has_opt}
for m in modes:  # warm-up: first-call kernel attribute set-up, storage growth
    set_mode(m)
    for _ in range(2):
        eng.train(1e-6, EP, M)
ts = {m: [] for m in modes}
for _ in range(reps):
    for m in modes:
        set_mode(m)
        t0 = time.perf_counter()
        eng.train(1e-6, EP, M)
        ts[m].append(time.perf_counter() - t0)
head = {m: [] for m in modes}
eng.profile(True)
for _ in range(reps):
    for m in modes:
        set_mode(m)
        eng.profile_reset()
        eng.train(1e-6, EP, M)
        ms, n = eng.profile_read("head")
        head[m].append(ms)  # (aleppo_profile_read: the mean per launch over the call's epochs x minibatches)
eng.profile(False)
for m, name in ((0, "off"), (1, "on")):
    if m in ts:
        v = sorted(ts[m])
        h = sorted(head[m])
        out[f"train_ms_median_{name}"] = round(v[len(v) // 2] * 1e3, 3)
        out[f"train_ms_min_{name}"] = round(v[0] * 1e3, 3)
        out[f"head_us_per_launch_median_{name}"] = round(h[len(h) // 2] * 1e3, 2)
        out[f"head_us_per_launch_min_{name}"] = round(h[0] * 1e3, 2)
        out[f"head_us_per_launch_max_{name}"] = round(h[-1] * 1e3, 2)
if has_opt:
    out["train_on_over_off"] = round(out["train_ms_median_on"] / out["train_ms_median_off"], 4)
print(json.dumps(out))
eng.close()
