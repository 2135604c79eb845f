"""CPU: the trainer's `device_environments: true` against host-only stand-ins (tests/stub/aleppo_stub_env.cc implements the
device-resident environments with trainer/emulator.hpp itself).  The mode must be the run with host environments: the same
counters and the same checkpoint file, byte for byte, and a file written in one mode resumes in the other.  A library
without the entry points refuses the key."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

BASE = "total_environments: 8\nhidden_size: 32\nhorizon: 8\nnum_mini_batches: 4\nnum_rollouts: 6\ndeterministic: true\n" \
       "num_workers: 2\nmax_steps: 60\n"
DEVICE = "device_environments: true\n"


def _make(target):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), target])
    return os.path.join(ROOT, "trainer", target)


@pytest.fixture(scope="module")
def trainer_env_stub():
    return _make("train_env_stub")


def _run(exe, tmp_path, name, extra, env=None):
    d = tmp_path / name
    os.makedirs(d, exist_ok=True)
    cfg = d / "c.yaml"
    cfg.write_text(BASE + extra)
    r = subprocess.run([exe, "rom.bin", str(d / "x.log"), str(d), "g", str(cfg)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return r


def _summary(stdout):
    return re.search(r"steps (\d+) episodes (\d+) pending_starts (\d+)", stdout).groups()


@pytest.mark.parametrize("extra", ["", "device_preprocess: true\nslot_ahead: false\n", "max_return: 3\n"],
                         ids=["84", "raw-pairs", "max-return"])
def test_both_modes_write_the_same_checkpoint_file(trainer_env_stub, tmp_path, extra):
    out = {}
    for mode, key in (("host", ""), ("device", DEVICE)):
        ck = tmp_path / f"{mode}.ckpt"
        r = _run(trainer_env_stub, tmp_path, mode, extra + key + f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n")
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        out[mode] = (ck.read_bytes(), _summary(r.stdout), re.findall(r"checkpoint rollout \d+ digest [^>]*", r.stdout))
    assert out["host"][1] == out["device"][1] and int(out["host"][1][1]) > 0  # (steps, episodes, pending starts)
    assert out["host"][2] == out["device"][2] and len(out["host"][2]) == 3
    assert out["host"][0] == out["device"][0]


@pytest.mark.parametrize("first,second", [("", DEVICE), (DEVICE, "")], ids=["host-then-device", "device-then-host"])
def test_a_checkpoint_resumes_in_the_other_mode(trainer_env_stub, tmp_path, first, second):
    full_ck, ck, res_ck = tmp_path / "full.ckpt", tmp_path / "part.ckpt", tmp_path / "res.ckpt"
    full = _run(trainer_env_stub, tmp_path, "full", f"checkpoint_path: {full_ck}\ncheckpoint_interval: 2\n")
    assert full.returncode == 0, full.stderr[-2000:]
    part = _run(trainer_env_stub, tmp_path, "part", first + f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n",
                env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="4"))
    assert part.returncode == 0 and "stopped after the checkpoint of rollout 4" in part.stdout, part.stderr[-2000:]
    res = _run(trainer_env_stub, tmp_path, "res", second + f"resume: {ck}\ncheckpoint_path: {res_ck}\n")
    assert res.returncode == 0 and "at rollout 4 of 6, state digest verified" in res.stdout, res.stderr[-2000:]
    assert "Rollout 5 of 6" in res.stdout and "Rollout 4 of 6" not in res.stdout
    assert _summary(res.stdout) == _summary(full.stdout)
    assert res_ck.read_bytes() == full_ck.read_bytes()


def test_library_without_the_entry_points_refuses_the_key(tmp_path):
    for target in ("train_tsan", "train_ckpt_stub"):
        r = _run(_make(target), tmp_path, target, DEVICE)
        assert r.returncode == 1 and "aleppo_env_open is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
