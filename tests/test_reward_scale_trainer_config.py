"""The reward-scaling keys of the trainer, without a GPU: load-time refusals, a valid config loading, and the host-only
(ThreadSanitizer / stub) build refusing reward_scaling: true by naming the missing entry point while running as before
without the key."""
import os
import subprocess

import pytest

from conftest import ROOT
from shared_fixtures import trainer  # noqa: F401

BASE = "total_environments: 8\nhidden_size: 32\nhorizon: 8\nnum_mini_batches: 4\nnum_rollouts: 1\ndeterministic: true\n"


@pytest.fixture(scope="module")
def trainer_tsan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_tsan"])
    return os.path.join(ROOT, "trainer", "train_tsan")


def _run(exe, tmp_path, extra, env=None):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(BASE + extra)
    return subprocess.run([exe, "rom.bin", str(tmp_path / "x.log"), str(tmp_path), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300, env=env)


@pytest.mark.parametrize("extra,message", [
    ("reward_scaling: true\nreward_scale_clip: 0\n", "reward_scale_clip must be finite and positive"),
    ("reward_scaling: true\nreward_scale_clip: -10\n", "reward_scale_clip must be finite and positive"),
    ("reward_scaling: true\nreward_scale_clip: 1e39\n", "reward_scale_clip must be finite and positive"),
    ("reward_scaling: true\nreward_scale_clip: ten\n", "bad value for reward_scale_clip"),
    ("reward_scale_clip: 10.0\n", "reward_scale_clip needs reward_scaling: true"),
    ("reward_scaling: false\nreward_scale_clip: 5\n", "reward_scale_clip needs reward_scaling: true"),
])
def test_invalid_reward_scaling_keys_are_refused_when_the_config_is_loaded(trainer, tmp_path, extra, message):
    r = _run(trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr, r.stderr


@pytest.mark.parametrize("extra", ["reward_scaling: true\n", "reward_scaling: true\nreward_scale_clip: 10.0\n",
                                   "reward_scaling: true\nreward_scale_clip: 0.5\n", "reward_scaling: false\n"])
def test_valid_reward_scaling_keys_load(trainer, tmp_path, extra):
    """a valid config passes load_config (the run then stops at the initial-parameter dump: no GPU needed)"""
    r = _run(trainer, tmp_path, extra, env=dict(os.environ, ALEPPO_TRAINER_DUMP_INIT=str(tmp_path / "i.bin")))
    assert r.returncode == 0, r.stderr


def test_stub_build_refuses_reward_scaling_and_names_the_missing_entry_point(trainer_tsan, tmp_path):
    r = _run(trainer_tsan, tmp_path, "reward_scaling: true\n")
    assert r.returncode != 0 and "aleppo_export_reward_scale" in r.stderr, r.stderr
    r = _run(trainer_tsan, tmp_path, "")  # without the key the stub build runs as before
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    r = _run(trainer_tsan, tmp_path, "reward_scaling: false\n")
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
