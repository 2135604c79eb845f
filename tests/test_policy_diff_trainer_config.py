"""The trainer's log_policy_churn keys on the host-only stand-in (tests/stub/aleppo_stub_policy_diff.cc, which counts and
records its calls and answers (4 * set_a + set_b + k) / 64 for stat k): the tags with the key and without it, the interval,
a take before every comparison, the averaged comparison after the EMA update, and every start-up refusal.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import policy_diff_ref as pdr
import trainer_helpers
from conftest import ROOT

# tag -> the stat it must carry
NAMES = dict(churn="churn", kl="mean_kl_ab", kl_reverse="mean_kl_ba", tv="mean_tv", value_change="rms_dv",
             feature_cos="mean_feature_cos", feature_change="feature_rel_change")
EMA_NAMES = dict(ema_churn="churn", ema_kl="mean_kl_ab")
TAGS = {f"policy_churn/{n}".encode() for n in NAMES}
EMA_TAGS = {f"policy_churn/{n}".encode() for n in EMA_NAMES}
LIVE, AVERAGED, SNAPSHOT = 0, 1, 2


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
def pdiff_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_pdiff_stub"])
    return os.path.join(ROOT, "trainer", "train_pdiff_stub")


def _calls(r):
    out = []
    for f in ("aleppo_snapshot_take", "aleppo_policy_diff"):
        m = re.search(rf"stub: {f} calls: (\d+)", r.stderr)
        assert m, r.stderr[-2000:]
        out.append(int(m.group(1)))
    return tuple(out)


def _sequence(r):
    """the stand-in's record in order: ("take", source), ("diff", a, b, fresh) and ("ema",) for every aleppo_ema_update"""
    seq = []
    for line in r.stderr.splitlines():
        m = re.match(r"stub: aleppo_snapshot_take source=(\d+)$", line)
        if m:
            seq.append(("take", int(m.group(1))))
        m = re.match(r"stub: aleppo_policy_diff a=(\d+) b=(\d+) fresh=(\d)$", line)
        if m:
            seq.append(("diff", int(m.group(1)), int(m.group(2)), int(m.group(3))))
        if re.match(r"stub: aleppo_ema_update decay=", line):
            seq.append(("ema",))
    return seq


def _want(a, b, stat):
    return (4 * a + b + pdr.IDX[stat]) / 64.0


def test_trainer_keys_with_the_stub_library(pdiff_trainer, tmp_path):
    # name: (yaml, takes, comparisons, averaged)
    runs = (("absent", "", 0, 0, False), ("false", "log_policy_churn: false\n", 0, 0, False),
            ("true", "log_policy_churn: true\n", 4, 4, False),
            ("every2", "log_policy_churn: true\npolicy_churn_interval: 2\n", 2, 2, False),
            ("ema", "ema_decay: 0.9\n", 0, 0, False),
            ("averaged", "log_policy_churn: true\npolicy_churn_interval: 2\npolicy_churn_averaged: true\nema_decay: 0.9\n",
             2, 4, True))
    tags, blobs = {}, {}
    for name, extra, takes, diffs, averaged in runs:
        (tmp_path / name).mkdir()
        r = _run_trainer(pdiff_trainer, tmp_path / name, extra)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        assert _calls(r) == (takes, diffs), name  # the key off: the library is never called
        seq = _sequence(r)
        if not takes:
            assert not [s for s in seq if s[0] != "ema"], name
        else:  # per interval-th rollout: the take, (the update,) the EMA update, the comparison(s) - a take precedes every one
            per = [("take", LIVE)] + ([("ema",)] if averaged else []) + [("diff", SNAPSHOT, LIVE, 1)] + \
                  ([("diff", AVERAGED, LIVE, 0)] if averaged else [])
            other = [("ema",)] if averaged else []  # a rollout outside the interval
            every = 4 // takes
            want = []
            for k in range(4):
                want += per if (k + 1) % every == 0 else other
            assert seq == want, (name, seq)
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
        tags[name] = _scalar_bits(blobs[name])
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    assert not any(t.startswith(b"policy_churn") for t in tags["absent"]) and len(TAGS) == 7
    assert not any(t.startswith(b"policy_churn") for t in tags["ema"])
    for name, _, takes, _, averaged in runs:
        if not takes:
            continue
        base = "ema" if averaged else "absent"
        mine = TAGS | (EMA_TAGS if averaged else set())
        assert set(tags[name]) == set(tags[base]) | mine  # nothing else appears or goes
        for tag in tags[base]:  # (the stand-in is deterministic: the rest of the event file does not move)
            assert tags[base][tag] == tags[name][tag], tag
        for n, stat in NAMES.items():
            got = [_f(b) for b in tags[name][f"policy_churn/{n}".encode()]]
            assert got == [np.float32(_want(SNAPSHOT, LIVE, stat))] * takes and len(tags[name][b"mean_loss"]) == 4, n
        if averaged:
            for n, stat in EMA_NAMES.items():
                got = [_f(b) for b in tags[name][f"policy_churn/{n}".encode()]]
                assert got == [np.float32(_want(AVERAGED, LIVE, stat))] * takes, n
        assert b"log_policy_churn" in blobs[name] and b"policy_churn_interval" in blobs[name]  # the config dump, only when set
        assert (b"policy_churn_averaged" in blobs[name]) == averaged
    for name in ("absent", "false", "ema"):
        assert b"policy_churn" not in blobs[name]


@pytest.mark.parametrize("extra,message", [
    ("log_policy_churn: true\npolicy_churn_interval: 0\n", "policy_churn_interval must be positive"),
    ("log_policy_churn: true\npolicy_churn_interval: -2\n", "policy_churn_interval must be positive"),
    ("log_policy_churn: true\npolicy_churn_interval: some\n", "bad value for policy_churn_interval"),
    ("policy_churn_interval: 2\n", "policy_churn_interval needs log_policy_churn: true"),
    ("log_policy_churn: false\npolicy_churn_interval: 2\n", "policy_churn_interval needs log_policy_churn: true"),
    ("policy_churn_averaged: true\nema_decay: 0.9\n", "policy_churn_averaged needs log_policy_churn: true"),
    ("log_policy_churn: false\npolicy_churn_averaged: false\n", "policy_churn_averaged needs log_policy_churn: true"),
    ("log_policy_churn: true\npolicy_churn_averaged: true\n", "policy_churn_averaged needs ema_decay"),
])
def test_trainer_refuses_bad_keys(pdiff_trainer, tmp_path, extra, message):
    r = _run_trainer(pdiff_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == (0, 0)


def test_library_without_the_symbols_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without the two entry points)
    r = _run_trainer(plain, tmp_path, "log_policy_churn: true\n", 2)
    assert r.returncode == 1 and "aleppo_snapshot_take / aleppo_policy_diff are missing" in r.stderr, r.stderr
    assert "Rollout" not in r.stdout
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
