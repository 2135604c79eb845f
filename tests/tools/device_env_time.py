"""developer tool: what a rollout costs without host hand-offs.  `python tests/tools/device_env_time.py [processes] [rollouts]`.

At the benchmark's shape (E = 128, T = 128, bf16, H = 512), ms per rollout (host clock around the enqueue and
finish_rollout, which ends in a stream synchronise) of
  replay_84 / replay_raw   aleppo_replay_rollout from an HBM-resident trace (what the parent commit also has: the stream runs
                           one slot ahead of a host that waits for every slot's actions),
  env_84 / env_raw         aleppo_env_rollout (the device-resident environments, 84x84 frames / raw pairs),
and the environment kernel's own time per slot from HIP events (ALEPPO_ENV_F_STEP_MS, in rollouts of its own with profiling
on: the events serialise nothing, but they are kept out of the timed rollouts anyway).
Every variant runs in `processes` (default 3) fresh child processes, the variants alternating; each child times `rollouts`
(default 20) rollouts after 3 warm-up rollouts.  Prints one JSON line: per variant the per-process medians, their median
and spread (max - min of the process medians), and the env-steps/s that median means.
`--learn N`: instead, train on env_84 rollouts for N updates (v0.yaml's update: 4 epochs, 4 minibatches, lr 2.5e-4 annealed)
and print the mean episode length per 10 updates - an observation, not a test."""
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

E, T, A, H = 128, 128, 4, 512
VARIANTS = ("replay_84", "env_84", "replay_raw", "env_raw")


def engine():
    import hashfill as hf
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    return pkg, eng


def child(variant, rollouts):
    import torch
    pkg, eng = engine()
    raw = variant.endswith("raw")
    kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    out = {}
    if variant.startswith("env"):
        eng.env_open(frame_kind=kind)

        def rollout():
            eng.env_rollout()
            eng.finish_rollout()
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        shape = (T, E, 2, 210, 160) if raw else (T, E, 84, 84)
        frames = torch.randint(0, 256, shape, device="cuda", generator=g, dtype=torch.int16).to(torch.uint8)
        torch.cuda.synchronize()
        rew, zeros = np.zeros((T, E), np.float32), np.zeros((T, E), np.uint8)
        start = zeros.copy()
        start[0] = 1
        slot = frames[0].numel()

        def rollout():
            eng.replay_rollout(frames.data_ptr(), kind, slot, rew, zeros, zeros, start)
            eng.finish_rollout()
    for _ in range(3):
        rollout()
    ts = []
    for _ in range(rollouts):
        t0 = time.perf_counter()
        rollout()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["ms"] = ts
    if variant.startswith("env"):
        eng.profile(True)
        eng.profile_reset()
        for _ in range(3):
            rollout()
        ms, n = eng.env_read("step_ms")
        eng.profile(False)
        out["env_kernel_us"], out["env_kernel_launches"] = float(ms) * 1e3, int(n)
    eng.close()
    print(json.dumps(out))


def learn(updates):
    pkg, eng = engine()
    eng.env_open(frame_kind=pkg.FRAMES_84)
    eng.env_rollout()
    eng.finish_rollout()  # the warm rollout
    lens, t0 = [], time.perf_counter()
    for u in range(updates):
        eng.env_rollout()
        eng.finish_rollout()
        lens.extend(eng.env_episodes()[1].tolist())
        eng.train(2.5e-4 * (1 - u / updates), 4, 4)
        if (u + 1) % 10 == 0:
            print(json.dumps(dict(update=u + 1, episodes=len(lens), mean_episode_length=round(float(np.mean(lens)), 2) if lens
                                  else None, env_steps_per_s=round((u + 1) * E * T / (time.perf_counter() - t0)))), flush=True)
            lens = []
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--learn":
        learn(int(sys.argv[2]))
    else:
        processes = int(sys.argv[1]) if len(sys.argv) > 1 else 3
        rollouts = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        runs = {v: [] for v in VARIANTS}
        for _ in range(processes):
            for v in VARIANTS:  # alternating: every variant sees the same drift of the machine
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, str(rollouts)],
                                   capture_output=True, text=True, timeout=600, cwd=ROOT)
                if r.returncode:
                    raise SystemExit(f"{v} failed: " + r.stderr[-2000:])
                runs[v].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        out = dict(shape=dict(E=E, T=T, H=H, precision="bf16"), processes=processes, rollouts=rollouts)
        for v, rs in runs.items():
            med = [float(np.median(r["ms"])) for r in rs]
            out[v] = dict(process_medians_ms=[round(m, 3) for m in med], median_ms=round(float(np.median(med)), 3),
                          spread_ms=round(max(med) - min(med), 3), p10_p90_ms=[round(float(np.percentile(
                              np.concatenate([r["ms"] for r in rs]), q)), 3) for q in (10, 90)],
                          env_steps_per_s=round(E * T / (float(np.median(med)) * 1e-3)))
            if "env_kernel_us" in rs[0]:
                ks = [r["env_kernel_us"] for r in rs]
                out[v]["env_kernel_us_per_slot"] = dict(process_means=[round(k, 2) for k in ks],
                                                        median=round(float(np.median(ks)), 2),
                                                        spread=round(max(ks) - min(ks), 2))
        print(json.dumps(out))
