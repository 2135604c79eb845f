"""developer tool: what setting ALEPPO_OPT_CLIP_PARAM and its kin costs at the BASELINE configs[1] update shape (128
envs x T = 128, 4 epochs x 4 minibatches of 4096, bf16, rollout batch): `python tests/tools/hyper_time.py [reps]
[first]`.  Two contexts in one process on the same rollout, alternating per call: `off` never sets an option, `on` has
all five set to the config's own values; `first` (`off`, the default, or `on`) names the one that is created, warmed up
and timed first.  Both read the numbers from the device block that every aleppo_train uploads and launch the same
kernels, so the two columns should agree within the scatter.  ALEPPO_LIB_PATH lets the same script time another build of
the library: with one from before the kernel-argument entry points were removed, the `off` column is those entry points
and the `on` column the device block.  Two phases: the whole aleppo_train (host clock; it waits for the device before it
returns) with profiling off, then the head and Adam kernels' device time (aleppo_profile_read, HIP events) with
profiling on.  Prints one JSON line."""
import json
import os
import sys
import time

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _T)
sys.path.insert(0, os.path.dirname(_T))
import hashfill as hf  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_gpu_at_size import DeviceBytes, _flags  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
pkg = load_package()
E, T, A, H, M, EP = 128, 128, 4, 512, 4, 4
dev = DeviceBytes(hf.hf_bytes(311, (T, E, 84, 84)))
te, tr, st = _flags(312, T, E, 0.01, 0.0)
engs = {}
for name in (("on", "off") if sys.argv[2:3] == ["on"] else ("off", "on")):
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, max_minibatch=E * T // M)
    eng.load_params(hf.fill_params(310, H, A))
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, hf.hf_range(313, (T, E), -1, 1), te, tr, st)
    eng.finish_rollout()
    if name == "on":  # the config's own values: the same update, through the device block
        c = eng.cfg
        eng.set_hyper(clip_param=c.clip_param, value_clip_range=c.clip_param, value_loss_coef=c.value_loss_coef,
                      entropy_coef=c.entropy_coef, max_grad_norm=c.max_gradient_norm)
    engs[name] = eng
dev.free()

for eng in engs.values():  # warm-up: first-call kernel attribute set-up, storage growth
    for _ in range(2):
        eng.train(1e-6, EP, M)
ts = {k: [] for k in engs}
for _ in range(reps):
    for k, eng in engs.items():
        t0 = time.perf_counter()
        eng.train(1e-6, EP, M)
        ts[k].append(time.perf_counter() - t0)
kern = {k: {"head": [], "adam": []} for k in engs}
for eng in engs.values():
    eng.profile(True)
for _ in range(reps):
    for k, eng in engs.items():
        eng.profile_reset()
        eng.train(1e-6, EP, M)
        for cls in ("head", "adam"):
            kern[k][cls].append(eng.profile_read(cls)[0])  # (the mean per launch over the call's epochs x minibatches)
out = {"reps": reps}
for k in engs:
    v = sorted(ts[k])
    out[f"train_ms_median_{k}"] = round(v[len(v) // 2] * 1e3, 3)
    out[f"train_ms_min_{k}"] = round(v[0] * 1e3, 3)
    out[f"train_ms_max_{k}"] = round(v[-1] * 1e3, 3)
    for cls in ("head", "adam"):
        h = sorted(kern[k][cls])
        out[f"{cls}_us_per_launch_median_{k}"] = round(h[len(h) // 2] * 1e3, 2)
        out[f"{cls}_us_per_launch_min_{k}"] = round(h[0] * 1e3, 2)
out["update_ms_median_off"] = round(out["train_ms_median_off"] / EP, 3)  # per update of 4 minibatches (one epoch)
out["update_ms_median_on"] = round(out["train_ms_median_on"] / EP, 3)
out["train_on_over_off"] = round(out["train_ms_median_on"] / out["train_ms_median_off"], 4)
print(json.dumps(out))
for eng in engs.values():
    eng.close()
