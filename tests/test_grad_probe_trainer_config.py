"""The trainer's log_gradient_stats keys on the host-only stand-in (tests/stub/aleppo_stub_grad_probe.cc, which counts and
records its calls and answers by a closed form: two loss-as-it-stands probes give |G|^2 = 1 and S = 64, the policy / value
cosine of row r is (r + 1) / 16): the tags with the key and without it, the interval, the probe sequence in front of the
update, and every start-up refusal.  No GPU."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import trainer_helpers
from conftest import ROOT

B = 8 * 32 // 4  # debug.yaml: total_environments * horizon / num_mini_batches
ROWS = dict(conv1=0, conv2=2, conv3=4, fc=6, all=12)  # the weight tensors' rows of the Gram, and the whole model
TAGS = {b"gradients/noise_scale", b"gradients/momentum_cosine"} | {f"gradients/policy_value_cosine/{n}".encode()
                                                                   for n in ROWS}
FUNCS = ("aleppo_grad_probe", "aleppo_grad_take", "aleppo_grad_gram")


def _scalars(blob):
    """{tag: [float, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<f", blob[m.end():m.end() + 4])[0])
    return out


def _run_trainer(binary, d, extra, rollouts=4):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def gradprobe_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_gradprobe_stub"])
    return os.path.join(ROOT, "trainer", "train_gradprobe_stub")


def _calls(r):
    out = []
    for f in FUNCS:
        m = re.search(rf"stub: {f} calls: (\d+)", r.stderr)
        assert m, r.stderr[-2000:]
        out.append(int(m.group(1)))
    return tuple(out)


def _sequence(r):
    """the stand-in's record in order, without the "stub: " prefix and the totals"""
    return [line[6:] for line in r.stderr.splitlines() if line.startswith("stub: aleppo_") and " calls: " not in line]


def _per_rollout(small):
    """what one probed rollout records in front of its update"""
    return [f"aleppo_grad_probe slot=0 first=0 n={small} cfg=null", f"aleppo_grad_probe slot=1 first=0 n={B} cfg=null",
            "aleppo_grad_gram slots=0,1", f"aleppo_grad_probe slot=2 first=0 n={B} cfg=1,0,0",
            f"aleppo_grad_probe slot=3 first=0 n={B} cfg=0,1,0", "aleppo_grad_take slot=0 source=0 set=0",
            "aleppo_grad_gram slots=0,1,2,3"]


def test_trainer_keys_with_the_stub_library(gradprobe_trainer, tmp_path):
    # name: (yaml, probed rollouts of 4, the small batch)
    runs = (("absent", "", 0, 0), ("false", "log_gradient_stats: false\n", 0, 0),
            ("true", "log_gradient_stats: true\n", 4, B // 4),
            ("every2", "log_gradient_stats: true\ngradient_stats_interval: 2\ngradient_stats_small_batch: 7\n", 2, 7))
    tags, blobs = {}, {}
    for name, extra, probed, small in runs:
        (tmp_path / name).mkdir()
        r = _run_trainer(gradprobe_trainer, tmp_path / name, extra)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        assert _calls(r) == (4 * probed, probed, 2 * probed), name  # the key off: the library is never called
        seq = _sequence(r)
        # debug.yaml runs its 2 epochs as one aleppo_train per rollout; the probes come BEFORE the update of their rollout
        want = []
        for k in range(4):
            every = 4 // probed if probed else 0
            want += (_per_rollout(small) if probed and (k + 1) % every == 0 else []) + ["aleppo_train"]
        assert seq == want, (name, seq)
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
        tags[name] = _scalars(blobs[name])
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    for name in ("absent", "false"):
        assert not any(t.startswith(b"gradients/") for t in tags[name]) and b"gradient_stats" not in blobs[name]
    for name, _, probed, small in runs:
        if not probed:
            continue
        t = tags[name]
        assert set(t) == set(tags["absent"]) | TAGS  # nothing else appears or goes
        for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
            assert tags["absent"][tag] == t[tag], tag
        # |G|^2 = 1 and S = 64 from the two probes' norms 1 + 64 / n, with the counts as the batch sizes
        s2, l2 = 1 + 64 / small, 1 + 64 / B
        g2 = (B * l2 - small * s2) / (B - small)
        want = ((s2 - l2) / (1 / small - 1 / B)) / g2
        assert abs(want - 64) < 1e-9
        np.testing.assert_allclose(t[b"gradients/noise_scale"], [want] * probed, rtol=1e-6)
        for n, row in ROWS.items():
            np.testing.assert_allclose(t[f"gradients/policy_value_cosine/{n}".encode()], [(row + 1) / 16] * probed, rtol=1e-6)
        # the moment is zero at the first take: no scalar; afterwards (0.6, 0.8) against (1, 8 / sqrt(B))
        mom = (0.6 + 0.8 * 8 / math.sqrt(B)) / math.sqrt(1 + 64 / B)
        np.testing.assert_allclose(t[b"gradients/momentum_cosine"], [mom] * (probed - 1), rtol=1e-6)
        assert b"log_gradient_stats" in blobs[name] and b"gradient_stats_interval" in blobs[name]  # the config dump
        assert (b"gradient_stats_small_batch" in blobs[name]) == (name == "every2")


@pytest.mark.parametrize("extra,message", [
    ("log_gradient_stats: true\ngradient_stats_interval: 0\n", "gradient_stats_interval must be positive"),
    ("log_gradient_stats: true\ngradient_stats_interval: -3\n", "gradient_stats_interval must be positive"),
    ("log_gradient_stats: true\ngradient_stats_interval: some\n", "bad value for gradient_stats_interval"),
    ("gradient_stats_interval: 2\n", "gradient_stats_interval needs log_gradient_stats: true"),
    ("log_gradient_stats: false\ngradient_stats_small_batch: 8\n", "gradient_stats_small_batch needs log_gradient_stats: true"),
    ("log_gradient_stats: true\ngradient_stats_small_batch: 0\n", "gradient_stats_small_batch must be positive"),
    ("log_gradient_stats: true\ngradient_stats_small_batch: -4\n", "gradient_stats_small_batch must be positive"),
    ("log_gradient_stats: true\ngradient_stats_small_batch: 64\n", "gradient_stats_small_batch must be smaller than the minibatch (64"),
    ("log_gradient_stats: true\ngradient_stats_small_batch: 200\n", "gradient_stats_small_batch must be smaller than the minibatch (64"),
])
def test_trainer_refuses_bad_keys(gradprobe_trainer, tmp_path, extra, message):
    r = _run_trainer(gradprobe_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == (0, 0, 0)


def test_library_without_the_symbols_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without the entry points)
    r = _run_trainer(plain, tmp_path, "log_gradient_stats: true\n", 2)
    assert r.returncode == 1 and "aleppo_grad_probe / aleppo_grad_take / aleppo_grad_gram are missing" in r.stderr, r.stderr
    assert "Rollout" not in r.stdout
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
