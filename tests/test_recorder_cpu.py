"""CPU: the trainer's record_video / record_observation / record_evaluation / record_interval keys against host-only stand-ins
(tests/stub/aleppo_stub_rec.cc: trainer/emulator.hpp itself behind the device-resident environments and the episode
recorders).  The files are parsed with tests/recorder_ref.py, and replaying a file's recorded actions through the numpy
restatement of the emulator (tests/device_env_ref.py) must give every frame of the file byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

import device_env_ref as ref
import recorder_ref as rr
from conftest import ROOT

E, T, ROLLOUTS, MAX_STEPS = 8, 8, 6, 60
BASE = f"total_environments: {E}\nhidden_size: 32\nhorizon: {T}\nnum_mini_batches: 4\nnum_rollouts: {ROLLOUTS}\n" \
       f"deterministic: true\nnum_workers: 2\nmax_steps: {MAX_STEPS}\n"
DEV = "device_environments: true\n"
EVAL = "eval_interval: 2\neval_environments: 3\neval_episodes: 4\ndevice_evaluation: true\ndevice_evaluation_steps: 8\n"
SLOTS = (ROLLOUTS + 1) * T  # (the warm rollout is recorded too)


def _make(target):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), target])
    return os.path.join(ROOT, "trainer", target)


@pytest.fixture(scope="module")
def stub():
    return _make("train_rec_stub")


def _run(exe, tmp_path, name, extra):
    d = tmp_path / name
    os.makedirs(d, exist_ok=True)
    cfg = d / "c.yaml"
    cfg.write_text(BASE + extra)
    r = subprocess.run([exe, "rom.bin", str(d / "x.log"), str(d / "video"), "g", str(cfg)], capture_output=True, text=True,
                       timeout=300)
    return d / "video", r


def _ok(r):
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]


def _numbers(video, prefix="episode_"):
    """{n: path without extension} of the finished episodes, and the same of the .part ones"""
    done, part = {}, {}
    for f in os.listdir(video):
        m = re.fullmatch(re.escape(prefix) + r"(\d+)\.(y4m|tsv)(\.part)?", f)
        if m:
            (part if m.group(3) else done)[int(m.group(1))] = os.path.join(video, prefix + m.group(1))
    return done, part


def _replay(env, base, raw, part=False):
    """the file's rows through env: every frame of the .y4m is the emulator's; -> (rows, the episode ended)"""
    ext = ".part" if part else ""
    hdr, frames = rr.parse_y4m(base + ".y4m" + ext)
    steps, logits = rr.parse_tsv(base + ".tsv" + ext)
    want = dict(W="160", H="210", F="30:1") if raw else dict(W="84", H="84", F="15:1")
    assert hdr == dict(want, I="p", A="1:1", C="mono"), hdr
    assert open(base + ".y4m" + ext, "rb").readline() == \
        f"YUV4MPEG2 W{want['W']} H{want['H']} F{want['F']} Ip A1:1 Cmono\n".encode()
    assert len(frames) == (2 if raw else 1) * len(steps) and logits.shape == (len(steps), 4)
    assert steps["start"][0] == 1 and not steps["start"][1:].any()
    assert (np.diff(steps["ordinal"].astype(np.int64)) == 1).all()
    ended = False
    for k, s in enumerate(steps):
        assert not ended
        if s["start"]:
            f, term, trunc, go = env.reset(), False, False, False
        else:
            f, _, term, trunc, go = env.step(int(s["action"]))
        got = frames[2 * k:2 * k + 2] if raw else frames[k]
        assert got.tobytes() == f.tobytes(), (base, k)  # (the gray table the trainer gives the library is the identity)
        assert (bool(s["terminated"]), bool(s["truncated"]), bool(s["game_over"])) == (term, trunc, bool(go) and (term or trunc))
        assert int(s["lives"]) == env.lives
        ended = term or trunc
    return len(steps), ended


@pytest.mark.parametrize("raw", [False, True], ids=["84", "raw-pairs"])
def test_record_video_files_replay_byte_for_byte(stub, tmp_path, raw):
    extra = DEV + "record_video: true\n" + ("device_preprocess: true\n" if raw else "")
    video, r = _run(stub, tmp_path, "v", extra)
    _ok(r)
    done, part = _numbers(video)
    env = ref.Env(0, MAX_STEPS, -1.0, raw)  # environment 0 of rank 0 is seed 0
    rows = 0
    for n in range(1, len(done) + 1):  # one emulator through all of them, in order: nothing in between is missing
        assert n in done, sorted(done)
        k, ended = _replay(env, done[n], raw)
        assert ended
        rows += k
    assert len(done) >= 3
    assert sorted(part) in ([], [len(done) + 1])  # no .part but the unfinished last episode
    if part:
        k, ended = _replay(env, part[len(done) + 1], raw, part=True)
        assert not ended
        rows += k
    assert rows == SLOTS  # every slot of environment 0 is in exactly one file: the files are ALL its finished episodes


def test_record_observation_interval_and_the_unrecorded_paths(stub, tmp_path):
    video, r = _run(stub, tmp_path, "frames", DEV + "record_video: true\n")
    _ok(r)
    base_out = r.stdout
    # record_observation at 84x84: the same bytes
    obs, r = _run(stub, tmp_path, "obs", DEV + "record_video: true\nrecord_observation: true\n")
    _ok(r)
    assert sorted(os.listdir(obs)) == sorted(os.listdir(video)) and len(os.listdir(video)) >= 6
    for f in os.listdir(video):
        assert (obs / f).read_bytes() == (video / f).read_bytes(), f
    # record_interval: 2 writes episodes 1, 3, ... and exactly what the full run wrote for them
    every, _ = _numbers(video)
    half, r = _run(stub, tmp_path, "half", DEV + "record_video: true\nrecord_interval: 2\n")
    _ok(r)
    done, part = _numbers(half)
    assert sorted(done) == [n for n in sorted(every) if n % 2 == 1] and all(n % 2 == 1 for n in part)
    for n in done:
        for ext in (".y4m", ".tsv"):
            assert open(done[n] + ext, "rb").read() == open(every[n] + ext, "rb").read(), (n, ext)
    # the recorder changes nothing the run computes: the summary line but for the speed
    summary = lambda out: re.search(r"steps \d+ episodes \d+ pending_starts \d+ slots \d+", out).group(0)
    plain, r = _run(stub, tmp_path, "plain", DEV)
    _ok(r)
    assert summary(r.stdout) == summary(base_out) and not os.path.exists(plain)
    # record_video without device_environments: a note, no file, and the run of the same config without the key
    host, r = _run(stub, tmp_path, "host", "record_video: true\n")
    _ok(r)
    assert "record_video ignored (it needs device_environments: true" in r.stderr and not os.path.exists(host)
    _, r2 = _run(stub, tmp_path, "host_plain", "")
    _ok(r2)
    assert summary(r.stdout) == summary(r2.stdout)


def test_record_evaluation_files_replay_byte_for_byte(stub, tmp_path):
    video, r = _run(stub, tmp_path, "e", DEV + EVAL + "record_evaluation: true\n")
    _ok(r)
    assert not [f for f in os.listdir(video) if f.endswith(".part")]  # the unfinished episode of an evaluation is discarded
    steps = sorted({int(m.group(1)) for m in (re.match(r"eval_(\d+)_episode_", f) for f in os.listdir(video)) if m})
    assert len(steps) == ROLLOUTS // 2, os.listdir(video)  # eval_interval: 2
    assert not _numbers(video)[0]  # (record_video is off: no training episode)
    for rnd, step in enumerate(steps):
        done, _ = _numbers(video, f"eval_{step}_episode_")
        assert sorted(done) == list(range(1, len(done) + 1)) and done
        env = ref.Env(E + rnd * 3, MAX_STEPS, -1.0, False)  # lane 0 of evaluation `rnd`: seeded past the training environments
        for n in sorted(done):
            assert _replay(env, done[n], False)[1]


def test_keys_are_refused_without_their_prerequisites(stub, tmp_path):
    for extra, msg in ((DEV + "record_evaluation: true\n", "record_evaluation needs device_evaluation: true"),
                       (DEV + "eval_interval: 2\nrecord_evaluation: true\n", "record_evaluation needs device_evaluation: true"),
                       (DEV + "record_interval: 2\n", "record_interval needs record_video: true or record_evaluation: true"),
                       (DEV + "record_video: true\nrecord_interval: 0\n", "record_interval must be positive")):
        video, r = _run(stub, tmp_path, "bad", extra)
        assert r.returncode == 1 and msg in r.stderr and not os.path.exists(video), (extra, r.stderr[-500:])
    # a library without the entry points
    old = _make("train_eval_stub")
    for extra in (DEV + "record_video: true\n", DEV + EVAL + "record_evaluation: true\n"):
        video, r = _run(old, tmp_path, "old", extra)
        assert r.returncode == 1 and "aleppo_rec_open is missing" in r.stderr and not os.path.exists(video), r.stderr[-500:]
    _, r = _run(old, tmp_path, "old_host", "record_video: true\n")  # (only noted: nothing is asked of the library)
    _ok(r)
