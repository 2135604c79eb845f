"""The evaluation keys of the trainer and the numpy restatement of the evaluation rules, without a GPU: load-time
refusals of eval_* keys, the host-only (ThreadSanitizer / stub) build refusing a config that asks for evaluation by naming
the missing entry point, and tests/eval_ref.py on hand-written cases."""
import os
import subprocess

import numpy as np
import pytest

import eval_ref as er
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
    ("eval_interval: 1\neval_rule: argmax\n", "eval_rule must be greedy, sample or epsilon"),
    ("eval_interval: 1\neval_rule: epsilon\neval_epsilon: 1.5\n", "eval_epsilon must be in [0, 1]"),
    ("eval_interval: 1\neval_rule: epsilon\neval_epsilon: -0.1\n", "eval_epsilon must be in [0, 1]"),
    ("eval_interval: 1\neval_rule: sample\neval_temperature: 0\n", "eval_temperature must be finite and positive"),
    ("eval_interval: 1\neval_rule: sample\neval_temperature: -2\n", "eval_temperature must be finite and positive"),
    ("eval_environments: 4\n", "eval_environments needs eval_interval > 0"),
    ("eval_interval: 0\neval_episodes: 4\n", "eval_episodes needs eval_interval > 0"),
    ("eval_interval: 1\neval_environments: 0\n", "eval_environments must be in [1, 4096]"),
    ("eval_interval: 1\neval_environments: 5000\n", "eval_environments must be in [1, 4096]"),
    ("eval_interval: 1\neval_episodes: 0\n", "eval_episodes must be positive"),
    ("eval_interval: -1\n", "eval_interval must be non-negative"),
])
def test_invalid_eval_keys_are_refused_when_the_config_is_loaded(trainer, tmp_path, extra, message):
    r = _run(trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr, r.stderr


def test_valid_eval_keys_load(trainer, tmp_path):
    """a valid evaluation config passes load_config (the run then stops at the initial-parameter dump: no GPU needed)"""
    r = _run(trainer, tmp_path, "eval_interval: 2\neval_environments: 3\neval_episodes: 5\neval_rule: sample\n"
                                "eval_temperature: 0.5\n", env=dict(os.environ, ALEPPO_TRAINER_DUMP_INIT=str(tmp_path / "i.bin")))
    assert r.returncode == 0, r.stderr


def test_stub_build_refuses_evaluation_and_names_the_missing_entry_point(trainer_tsan, tmp_path):
    r = _run(trainer_tsan, tmp_path, "eval_interval: 1\n")
    assert r.returncode != 0 and "aleppo_eval_open" in r.stderr, r.stderr
    r = _run(trainer_tsan, tmp_path, "")  # without the keys the stub build runs as before
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------ the restatement on hand-written cases
def test_greedy_restatement():
    z = np.array([[0.1, 0.7, 0.3], [2.0, 2.0, 1.0], [-1.0, -3.0, -1.0], [0.0, 0.0, 0.0]], np.float32)
    np.testing.assert_array_equal(er.greedy(z), [1, 0, 0, 0])


def test_epsilon_greedy_restatement():
    z = np.array([[0.1, 0.7, 0.3, 0.0]] * 6, np.float32)  # greedy: 1; A = 4
    uw = np.array([[0.25, 0.0],              # u == epsilon: greedy
                   [0.2499999, 0.0],         # explores: (int)(0 * 4) = 0
                   [0.0, 0.5],               # (int)(2.0) = 2
                   [0.0, 0.74999994],        # (int)(2.9999998) = 2
                   [0.0, 0.99999994],        # (int)(3.9999998) = 3 = A - 1
                   [0.9, 0.99]], np.float32)  # greedy
    np.testing.assert_array_equal(er.epsilon_greedy(z, 0.25, uw), [1, 0, 2, 2, 3, 1])
    np.testing.assert_array_equal(er.epsilon_greedy(z, 0.0, uw), [1] * 6)
    np.testing.assert_array_equal(er.epsilon_greedy(z, 1.0, uw), [0, 0, 2, 2, 3, 3])
    # A = 3: w * A rounds up to A in fp32 for the largest w (0.99999994 * 3 = 2.9999998 -> 2; clamped either way)
    z3 = np.zeros((1, 3), np.float32)
    np.testing.assert_array_equal(er.epsilon_greedy(z3, 1.0, np.array([[0.0, 0.99999994]], np.float32)), [2])


def test_sample_restatement():
    z = np.log(np.array([[0.5, 0.25, 0.25]], np.float64)).astype(np.float32)
    # tau = 1: p = (0.5, 0.25, 0.25); q = (1, 0.4, 1) -> p / q = (0.5, 0.625, 0.25): action 1, gap 0.2
    a, gap = er.sample(z, 1.0, np.array([[1.0, 0.4, 1.0]], np.float32))
    assert a[0] == 1 and abs(gap[0] - 0.2) < 1e-6
    # tau = 0.5 squares the probabilities: p = (4, 1, 1) / 6 -> p / q = (0.667, 0.4167, 0.1667): action 0
    a, gap = er.sample(z, 0.5, np.array([[1.0, 0.4, 1.0]], np.float32))
    assert a[0] == 0 and abs(gap[0] - (1 - 0.625)) < 1e-6
    # a high temperature flattens them: tau = 1e6 -> p ~ 1/3 each: the smallest q wins
    a, _ = er.sample(z, 1e6, np.array([[1.0, 0.9, 0.8]], np.float32))
    assert a[0] == 2
    # exact tie: the first maximum, gap 0
    a, gap = er.sample(np.zeros((1, 4), np.float32), 2.0, np.ones((1, 4), np.float32))
    assert a[0] == 0 and gap[0] == 0


def test_builtin_noise_restatement_is_the_philox_block_function():
    # Philox4x32-10 known answers (Random123 kat_vectors): zero counter / key, and the all-ones vector
    z = er.philox4x32_10(np.zeros((1, 4), np.uint32), 0, 0)[0]
    assert [int(x) for x in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    o = er.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert [int(x) for x in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    uw = er.eval_noise(7, 3, 5, 4, "epsilon")
    assert uw.shape == (5, 2) and uw.dtype == np.float32 and (uw > 0).all() and (uw < 1).all()
    q = er.eval_noise(7, 3, 5, 18, "sample")
    assert q.shape == (5, 18) and (q > 0).all()
    assert (er.eval_noise(7, 4, 5, 4, "epsilon") != uw).all() and (er.eval_noise(8, 3, 5, 4, "epsilon") != uw).all()
