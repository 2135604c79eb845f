"""The trainer's log_feature_rank keys on the host-only stand-in (tests/stub/aleppo_stub_feature_rank.cc, which runs the
library's own host solver on a closed-form Gram and counts its calls): the tags with the key and without it, the interval,
that delta / eps / centered arrive, and every start-up refusal.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import trainer_helpers
from conftest import ROOT

NAMES = ("effective", "srank", "pca", "threshold", "stable", "numerical", "sigma_max", "sigma_min", "mean_sq_norm",
         "nonfinite_rows")
TAGS = [f"feature_rank/{n}".encode() for n in NAMES]
N = 8 * 32  # debug.yaml: total_environments x horizon


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _run_trainer(binary, d, extra, rollouts=4):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def frank_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_frank_stub"])
    return os.path.join(ROOT, "trainer", "train_frank_stub")


def _calls(r):
    m = re.search(r"stub: aleppo_feature_rank calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    return int(m.group(1))


def _closed_form(delta, eps, centered):
    """the stand-in's answer: sigma_i = sqrt(N) 2^-i, i < 8; centred, the first becomes sqrt(3 N / 4)"""
    sig = np.sqrt(N) * 0.5 ** np.arange(8)
    if centered:
        sig[0] = np.sqrt(0.75 * N)
        sig = np.sort(sig)[::-1]
    S1, S2 = sig.sum(), (sig ** 2).sum()
    p = sig / S1
    return dict(effective=np.exp(-(p * np.log(p)).sum()), srank=int(np.argmax(np.cumsum(sig) >= (1 - delta) * S1)) + 1,
                pca=int(np.argmax(np.cumsum(sig ** 2) >= (1 - delta) * S2)) + 1, threshold=int((sig / np.sqrt(N) > eps).sum()),
                stable=S2 / sig[0] ** 2, numerical=8, sigma_max=sig[0], sigma_min=0.0,
                mean_sq_norm=(4 / 3) * (1 - 0.25 ** 8), nonfinite_rows=0.0)


def test_trainer_keys_with_the_stub_library(frank_trainer, tmp_path):
    runs = (("absent", "", 0, None), ("false", "log_feature_rank: false\n", 0, None),
            ("true", "log_feature_rank: true\n", 4, (0.01, 0.01, False)),
            ("every2", "log_feature_rank: true\nfeature_rank_interval: 2\nfeature_rank_delta: 0.1\nfeature_rank_eps: 0.1\n"
                       "feature_rank_centered: true\n", 2, (0.1, 0.1, True)))
    tags, blobs = {}, {}
    for name, extra, calls, _ in runs:
        (tmp_path / name).mkdir()
        r = _run_trainer(frank_trainer, tmp_path / name, extra)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        assert _calls(r) == calls, name  # the key off: the library is never called
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
        tags[name] = _scalar_bits(blobs[name])
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    assert not set(TAGS) & set(tags["absent"]) and len(TAGS) == 10
    assert not any(t.startswith(b"feature_rank") for t in tags["absent"])
    for name, _, calls, cfg in runs[2:]:
        assert set(tags[name]) == set(tags["absent"]) | set(TAGS)  # nothing else appears or goes
        for tag in TAGS:
            assert len(tags[name][tag]) == calls and len(tags[name][b"mean_loss"]) == 4, tag
        for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
            assert tags["absent"][tag] == tags[name][tag], tag
        want = _closed_form(*cfg)
        for n in NAMES:
            got = [_f(b) for b in tags[name][f"feature_rank/{n}".encode()]]
            if n == "sigma_min":  # (a zero eigenvalue comes back as rounding noise of the solver: below sqrt(16 H u) sigma_1)
                assert all(0 <= g <= 1e-6 * want["sigma_max"] for g in got), got
            else:
                np.testing.assert_allclose(got, [want[n]] * calls, rtol=1e-6, err_msg=n)
        assert b"log_feature_rank" in blobs[name]  # the hparams flag of the config dump, only when set
    assert b"log_feature_rank" not in blobs["absent"] and b"log_feature_rank" not in blobs["false"]


@pytest.mark.parametrize("extra,message", [
    ("log_feature_rank: true\nfeature_rank_delta: 0\n", "feature_rank_delta must be in (0, 1)"),
    ("log_feature_rank: true\nfeature_rank_delta: 1\n", "feature_rank_delta must be in (0, 1)"),
    ("log_feature_rank: true\nfeature_rank_delta: some\n", "bad value for feature_rank_delta"),
    ("log_feature_rank: true\nfeature_rank_eps: -0.1\n", "feature_rank_eps must be finite and non-negative"),
    ("log_feature_rank: true\nfeature_rank_eps: nan\n", "feature_rank_eps"),
    ("log_feature_rank: true\nfeature_rank_interval: 0\n", "feature_rank_interval must be positive"),
    ("feature_rank_interval: 2\n", "feature_rank_interval needs log_feature_rank: true"),
    ("feature_rank_delta: 0.1\n", "feature_rank_delta needs log_feature_rank: true"),
    ("feature_rank_eps: 0.1\n", "feature_rank_eps needs log_feature_rank: true"),
    ("log_feature_rank: false\nfeature_rank_centered: true\n", "feature_rank_centered needs log_feature_rank: true"),
])
def test_trainer_refuses_bad_keys(frank_trainer, tmp_path, extra, message):
    r = _run_trainer(frank_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == 0


def test_library_without_the_symbol_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without aleppo_feature_rank)
    r = _run_trainer(plain, tmp_path, "log_feature_rank: true\n", 2)
    assert r.returncode == 1 and "aleppo_feature_rank is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
