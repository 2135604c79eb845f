"""developer tool: what one evaluation costs with and without host hand-offs.
`python tests/tools/eval_env_time.py [processes] [evaluations]`.

At H = 512 in bf16, with L = 8 and L = 128 evaluation lanes, for 84x84 frames and raw pairs: the wall time in ms (host
clock, ending in a read that synchronises the stream) of ONE evaluation of 10 episodes under the greedy rule through
  host     the host loop eval_act -> emulator -> eval_push_frames.  The emulator is the Python restatement
           (tests/device_env_ref.py), far slower than the trainer's C++ one, so two figures are given: the whole loop
           (host_ms) and the time inside eval_act + eval_push_frames alone (host_lib_ms), which no emulator can undercut;
  device   aleppo_eval_env_open + aleppo_eval_env_run in chunks of S = 32 + the reads of two log planes, until 10
           episodes are in hand (device_ms).
Every variant runs in `processes` (default 3) fresh child processes, the variants alternating; each child times
`evaluations` (default 5) evaluations after one warm-up evaluation, every evaluation under seeds of its own.  Prints one
JSON line: per variant the per-process medians, their median and spread (max - min of the process medians), the steps the
evaluation took (host: where the loop stops; device: a multiple of S) - so device steps - host steps of the same L and
frame kind is what the device ran past the host's stopping point."""
import json
import os
import subprocess
import sys
import time

import numpy as np

_T = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(_T)
sys.path.insert(0, _T)
sys.path.insert(0, ROOT)

A, H, S, EPISODES = 4, 512, 32, 10
VARIANTS = [f"{mode}_{L}_{kind}" for L in (8, 128) for kind in ("84", "raw") for mode in ("host", "device")]


def child(variant, evaluations):
    import device_env_ref as ref
    import hashfill as hf
    from __graft_entry__ import load_package
    mode, L, kind = variant.split("_")
    L, raw = int(L), kind == "raw"
    pkg = load_package()
    eng = pkg.Engine(8, 8, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    eng.eval_open(L)
    fk = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    out = dict(ms=[], lib_ms=[], steps=[])
    for k in range(evaluations + 1):
        done = steps = 0
        lib = 0.0
        t0 = time.perf_counter()
        if mode == "host":
            envs = ref.EnvSet(L, 1000 + k * L, raw=raw)
            while done < EPISODES:
                t1 = time.perf_counter()
                actions = eng.eval_act("greedy")
                lib += time.perf_counter() - t1
                o = envs.step(actions)
                t1 = time.perf_counter()
                eng.eval_push_frames(o.frames, o.start, kind=fk)
                lib += time.perf_counter() - t1
                done += int((o.ep_len > 0).sum())
                steps += 1
            t1 = time.perf_counter()
            eng.eval_read("values")  # (synchronises, as the trainer's evaluate() does)
            lib += time.perf_counter() - t1
        else:
            eng.eval_env_open(frame_kind=fk, seed_base=1000 + k * L, run_steps=S)
            while done < EPISODES:
                eng.eval_env_run("greedy", steps=S)
                eng.eval_env_read("episode_returns")
                done += int((eng.eval_env_read("episode_lengths") > 0).sum())
                steps += S
        if k:  # (evaluation 0 is the warm-up)
            out["ms"].append((time.perf_counter() - t0) * 1e3)
            out["lib_ms"].append(lib * 1e3)
            out["steps"].append(steps)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        processes = int(sys.argv[1]) if len(sys.argv) > 1 else 3
        evaluations = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        runs = {v: [] for v in VARIANTS}
        for _ in range(processes):
            for v in VARIANTS:  # alternating: every variant sees the same drift of the machine
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, str(evaluations)],
                                   capture_output=True, text=True, timeout=300, cwd=ROOT)
                if r.returncode:
                    raise SystemExit(f"{v} failed: " + r.stderr[-2000:])
                runs[v].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        out = dict(shape=dict(H=H, precision="bf16", S=S, episodes=EPISODES), processes=processes, evaluations=evaluations)
        for v, rs in runs.items():
            out[v] = dict(steps=sorted({s for r in rs for s in r["steps"]}))
            for key in ("ms", "lib_ms") if v.startswith("host") else ("ms",):
                med = [float(np.median(r[key])) for r in rs]
                out[v][key] = dict(process_medians=[round(m, 3) for m in med], median=round(float(np.median(med)), 3),
                                   spread=round(max(med) - min(med), 3))
        print(json.dumps(out))
