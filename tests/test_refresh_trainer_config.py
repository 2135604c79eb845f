"""The trainer's recompute_advantages key on the host-only stand-in (tests/stub/aleppo_stub_refresh.cc, which records the
order of the update's calls and counts the refreshes): where aleppo_refresh_advantages goes in the epoch loop, how often, how
it composes with target_kl, the scalars, and the refusal against a library without the entry point.  No GPU."""
import os
import re
import struct
import subprocess

import pytest

import trainer_helpers
from conftest import ROOT
from shared_fixtures import stub_trainer  # noqa: F401

TAGS = [b"refresh/explained_variance", b"refresh/value_change_std", b"refresh/value_change_maxabs"]
LINE = re.compile(r"stub: (aleppo_finish_rollout|aleppo_train epochs=\d+|aleppo_refresh_advantages set=\d+ stats=\d+)")


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _run_trainer(binary, d, extra, rollouts=3):
    os.makedirs(d / "tb", exist_ok=True)
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def refresh_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_refresh_stub"])
    return os.path.join(ROOT, "trainer", "train_refresh_stub")


def _updates(r):
    """the calls of every update, in order: [["train", "refresh", ...], ...], one list per trained rollout; the refreshes
    checked against the stand-in's own count"""
    m = re.search(r"stub: aleppo_refresh_advantages calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    updates = []
    for line in LINE.findall(r.stderr):
        if line == "aleppo_finish_rollout":
            updates.append([])
        else:
            updates[-1].append(line)
    assert sum(c.startswith("aleppo_refresh") for u in updates for c in u) == int(m.group(1))
    return [u for u in updates if u]  # (a rollout that is finished but not trained on has no update)


TRAIN1, REFRESH = "aleppo_train epochs=1", "aleppo_refresh_advantages set=0 stats=13"


@pytest.mark.parametrize("epochs", [1, 2, 4])
def test_one_refresh_in_front_of_every_epoch_but_the_first(refresh_trainer, tmp_path, epochs):
    r = _run_trainer(refresh_trainer, tmp_path, f"recompute_advantages: true\nnum_epochs: {epochs}\n")
    assert r.returncode == 0, r.stderr[-2000:]
    updates = _updates(r)
    assert len(updates) == 3
    want = [TRAIN1] + [REFRESH, TRAIN1] * (epochs - 1)  # train, refresh, train, ...: never a trailing refresh
    assert all(u == want for u in updates), updates
    tags = _scalar_bits(trainer_helpers.events(tmp_path / "tb"))
    for tag, value in zip(TAGS, (0.5, 0.25, 0.75)):  # (the stand-in's figures; an update of one epoch has no refresh to log)
        assert [_f(b) for b in tags.get(tag, [])] == ([value] * 3 if epochs > 1 else []), tag
    assert len(tags[b"mean_loss"]) == 3


def test_target_kl_stop_leaves_no_trailing_refresh(refresh_trainer, tmp_path):
    """the stand-in's approx-KL is 0.01 per aleppo_train call of the update: target_kl 0.015 stops after the second epoch"""
    r = _run_trainer(refresh_trainer, tmp_path, "recompute_advantages: true\nnum_epochs: 4\ntarget_kl: 0.015\n")
    assert r.returncode == 0, r.stderr[-2000:]
    updates = _updates(r)
    assert len(updates) == 3 and all(u == [TRAIN1, REFRESH, TRAIN1] for u in updates), updates
    tags = _scalar_bits(trainer_helpers.events(tmp_path / "tb"))
    assert [_f(b) for b in tags[b"update_epochs"]] == [2.0] * 3
    assert len(tags[TAGS[0]]) == 3
    # ... and a target the first epoch already exceeds: one epoch, no refresh at all
    (tmp_path / "first").mkdir()
    r = _run_trainer(refresh_trainer, tmp_path / "first", "recompute_advantages: true\nnum_epochs: 4\ntarget_kl: 0.005\n")
    assert r.returncode == 0 and all(u == [TRAIN1] for u in _updates(r)), r.stderr[-2000:]
    assert not set(TAGS) & set(_scalar_bits(trainer_helpers.events(tmp_path / "first" / "tb")))


def test_key_off_never_calls_and_logs_the_same_bits(refresh_trainer, tmp_path):
    blobs, runs = {}, {}
    for name, extra in (("absent", ""), ("false", "recompute_advantages: false\n"), ("true", "recompute_advantages: true\n")):
        (tmp_path / name).mkdir()
        runs[name] = _run_trainer(refresh_trainer, tmp_path / name, extra)
        assert runs[name].returncode == 0, runs[name].stderr[-2000:]
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
    tags = {k: _scalar_bits(b) for k, b in blobs.items()}
    for name in ("absent", "false"):
        assert all(u == ["aleppo_train epochs=2"] for u in _updates(runs[name])), name  # one call of num_epochs, as ever
        assert "aleppo_refresh_advantages set" not in runs[name].stderr
        assert not set(TAGS) & set(tags[name]) and b"recompute_advantages" not in blobs[name]
    assert tags["absent"] == tags["false"] and b"mean_loss" in tags["absent"]
    assert set(tags["true"]) == set(tags["absent"]) | set(TAGS) and b"recompute_advantages" in blobs["true"]
    for tag in tags["absent"]:  # (the stand-in is deterministic: the other scalars do not move - but for the approx-KL,
        if tag != b"mean_approx_kl":  # which this stand-in makes a function of the update's aleppo_train calls)
            assert tags["absent"][tag] == tags["true"][tag], tag


def test_library_without_the_entry_point_refuses_the_key(stub_trainer, tmp_path):
    r = _run_trainer(stub_trainer, tmp_path, "recompute_advantages: true\n", 2)
    assert r.returncode == 1 and "no aleppo_refresh_advantages" in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    (tmp_path / "off").mkdir()
    off = _run_trainer(stub_trainer, tmp_path / "off", "recompute_advantages: false\n", 2)
    assert off.returncode == 0, off.stderr[-2000:]
    (tmp_path / "plain").mkdir()
    plain = _run_trainer(stub_trainer, tmp_path / "plain", "", 2)
    assert _scalar_bits(trainer_helpers.events(tmp_path / "off" / "tb")) == \
        _scalar_bits(trainer_helpers.events(tmp_path / "plain" / "tb"))
