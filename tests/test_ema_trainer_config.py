"""The trainer's ema_decay / ema_warmup / eval_averaged keys on the host-only stand-in (tests/stub/aleppo_stub_ema.cc, which
keeps the average by the header's rule, records every update's decay and counts its calls): the decay of every update, the
call count, the scalars and the hparams, the checkpoint's optional section 7 and its resume, the option of eval_averaged,
and every start-up refusal.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ema_ref as er
import trainer_helpers
from conftest import ROOT

TAGS = [b"ema_decay", b"ema_distance", b"ema_relative_distance"]
CALL = re.compile(r"stub: aleppo_ema_update decay=(\S+) updates=(\d+)")
H, A = 32, 4
N_PARAMS = 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64 + H * 3136 + H + A * H + A + H + 1


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _run_trainer(binary, d, extra, rollouts=4, env=None):
    os.makedirs(d / "tb", exist_ok=True)
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def ema_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_ema_stub"])
    return os.path.join(ROOT, "trainer", "train_ema_stub")


def _calls(r):
    """[(decay as printed, updates after the call)] of a run, checked against the stand-in's own count"""
    m = re.search(r"stub: aleppo_ema_update calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    recorded = [(d, int(u)) for d, u in CALL.findall(r.stderr)]
    assert len(recorded) == int(m.group(1))
    return recorded


def _sections(blob):
    """{id: bytes} of a checkpoint file (little-endian: magic, version, the 40-byte shape, sections, the end mark)"""
    assert blob[:8] == b"ALEPPOCK" and blob[-8:] == b"ALEPPOEN" and struct.unpack("<I", blob[8:12])[0] == 1
    pos, out = 12 + 40, {}
    while pos < len(blob) - 8:
        sid, n = struct.unpack("<IQ", blob[pos:pos + 12])
        out[sid] = blob[pos + 12:pos + 12 + n]
        pos += 12 + n
    assert pos == len(blob) - 8
    return out


def test_decays_calls_scalars_and_hparams(ema_trainer, tmp_path):
    g17 = lambda x: "%.17g" % x
    runs = (("absent", "", None), ("plain", "ema_decay: 0.9\n", [g17(0.9)] * 4),
            ("warmup", "ema_decay: 0.9\nema_warmup: true\n", [g17(0.1), g17(2 / 11), g17(3 / 12), g17(4 / 13)]),
            ("zero", "ema_decay: 0\n", [g17(0.0)] * 4))
    tags, blobs, ckpts = {}, {}, {}
    for name, extra, want in runs:
        d = tmp_path / name
        d.mkdir()
        r = _run_trainer(ema_trainer, d, extra + f"checkpoint_path: {d / 'run.ckpt'}\n", 4)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        calls = _calls(r)
        blobs[name] = trainer_helpers.events(d / "tb")
        tags[name] = _scalar_bits(blobs[name])
        ckpts[name] = _sections((d / "run.ckpt").read_bytes())
        if want is None:  # the key absent: no call, no open, no tag, no hparams entry, no section 7
            assert calls == [] and "aleppo_ema_open" not in r.stderr
            assert not set(TAGS) & set(tags[name]) and b"ema_" not in blobs[name]
            assert sorted(ckpts[name]) == [1, 2, 3, 4, 5, 6]
            continue
        # one update per trained rollout (the warm rollout trains nothing), with the decays of the rule, to the last digit
        assert [c[0] for c in calls] == want and [c[1] for c in calls] == [1, 2, 3, 4], (name, calls)
        assert r.stderr.count("stub: aleppo_ema_open") == 1
        assert r.stderr.index("stub: aleppo_ema_open") < r.stderr.index("stub: aleppo_ema_update decay")
        assert [_f(b) for b in tags[name][b"ema_decay"]] == [float(np.float32(float(w))) for w in want], name
        dist, rel = [[_f(b) for b in tags[name][t]] for t in TAGS[1:]]
        assert len(dist) == len(rel) == 4 and all(np.isfinite(dist)) and all(np.isfinite(rel))
        if name == "zero":  # decay 0: the average IS the parameters after every update
            assert dist == [0.0] * 4 and rel == [0.0] * 4
        else:
            assert all(x > 0 for x in dist) and all(x > 0 for x in rel)
        assert b"ema_decay" in blobs[name] and (b"ema_warmup" in blobs[name]) == (name == "warmup")
        assert set(tags[name]) == set(tags["absent"]) | set(TAGS)  # nothing else appears or goes
        for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
            assert tags["absent"][tag] == tags[name][tag], tag
        # section 7: the averaged parameters in reference order, then u64 updates; the other sections are the run's without
        assert sorted(ckpts[name]) == [1, 2, 3, 4, 5, 6, 7] and len(ckpts[name][7]) == N_PARAMS * 4 + 8
        assert struct.unpack("<Q", ckpts[name][7][-8:])[0] == 4
        for sid in range(1, 7):
            assert ckpts[name][sid] == ckpts["absent"][sid], (name, sid)
        avg, live = np.frombuffer(ckpts[name][7][:-8], np.float32), np.frombuffer(ckpts[name][1], np.float32)
        assert np.array_equal(avg, live) == (name == "zero")
    # the two non-trivial averages differ from each other (the decays reached the rule)
    assert ckpts["plain"][7] != ckpts["warmup"][7]


def test_the_checkpointed_average_is_the_rule_on_the_checkpointed_parameters(ema_trainer, tmp_path):
    """checkpoints after every rollout: section 7 of rollout k is the restatement's update of section 7 of rollout k - 1
    and section 1 of rollout k, bit for bit, with the warm-up decays"""
    prev = None
    for k in (1, 2, 3):
        d = tmp_path / f"k{k}"
        d.mkdir()
        r = _run_trainer(ema_trainer, d, f"ema_decay: 0.9\nema_warmup: true\ncheckpoint_path: {d / 'run.ckpt'}\n"
                         "checkpoint_interval: 1\n", 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT=str(k)))
        assert r.returncode == 0 and f"stopped after the checkpoint of rollout {k}" in r.stdout, r.stderr[-2000:]
        sec = _sections((d / "run.ckpt").read_bytes())
        avg, live = np.frombuffer(sec[7][:-8], np.float32), np.frombuffer(sec[1], np.float32)
        if prev is not None:  # (deterministic: the same run, stopped one rollout later)
            want = er.update(prev, live, er.warmup_decay(0.9, k - 1))
            assert np.array_equal(want.view(np.uint32), avg.view(np.uint32)), k
            assert not np.array_equal(avg, live)
        prev = avg


def test_resume_is_byte_identical_section_seven_included(ema_trainer, tmp_path):
    keys = "ema_decay: 0.9\nema_warmup: true\n"
    full, part = tmp_path / "full", tmp_path / "part"
    full.mkdir()
    part.mkdir()
    r = _run_trainer(ema_trainer, full, keys + f"checkpoint_path: {full / 'run.ckpt'}\ncheckpoint_interval: 2\n", 4)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    ck = part / "run.ckpt"
    ckeys = keys + f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n"
    p = _run_trainer(ema_trainer, part, ckeys, 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert p.returncode == 0 and "stopped after the checkpoint of rollout 2" in p.stdout, p.stderr[-2000:]
    assert [c[1] for c in _calls(p)] == [1, 2]
    assert struct.unpack("<Q", _sections(ck.read_bytes())[7][-8:])[0] == 2
    res = _run_trainer(ema_trainer, part, ckeys + f"resume: {ck}\n", 4)
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert "resumed the averaged parameters at update 2, verified" in res.stdout
    assert "stub: aleppo_ema_import updates=2" in res.stderr
    # the warm-up goes on at n = 2, 3: the decays of the uninterrupted run's last two updates
    assert _calls(res) == [("%.17g" % (3 / 12), 3), ("%.17g" % (4 / 13), 4)]
    assert ck.read_bytes() == (full / "run.ckpt").read_bytes()
    assert 7 in _sections(ck.read_bytes())


def test_resume_without_the_section_and_a_section_without_the_key(ema_trainer, tmp_path):
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir()
    new.mkdir()
    ck = old / "run.ckpt"
    base = f"checkpoint_path: {ck}\ncheckpoint_interval: 1\n"
    p = _run_trainer(ema_trainer, old, base, 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="3"))
    assert p.returncode == 0 and sorted(_sections(ck.read_bytes())) == [1, 2, 3, 4, 5, 6], p.stderr[-2000:]
    live3 = np.frombuffer(_sections(ck.read_bytes())[1], np.float32).copy()
    # with the key, from a file without the section: the average starts at the resumed parameters, and the run says so
    res = _run_trainer(ema_trainer, old, base + f"resume: {ck}\nema_decay: 0.5\n", 4)
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert "has no averaged parameters (section 7): the average starts at the resumed parameters" in res.stderr
    assert "aleppo_ema_import" not in res.stderr and _calls(res) == [("%.17g" % 0.5, 1)]
    sec = _sections(ck.read_bytes())
    assert struct.unpack("<Q", sec[7][-8:])[0] == 1
    # one update at 0.5 from the parameters the file of rollout 3 held, towards those of rollout 4: the rule, bit for bit
    avg, live4 = np.frombuffer(sec[7][:-8], np.float32), np.frombuffer(sec[1], np.float32)
    assert not np.array_equal(live3, live4)
    assert np.array_equal(er.update(live3, live4, 0.5).view(np.uint32), avg.view(np.uint32))
    # without the key, from a file with the section: ignored, and the file written next has none
    ck7 = new / "run.ckpt"
    keys7 = f"checkpoint_path: {ck7}\ncheckpoint_interval: 2\n"
    p = _run_trainer(ema_trainer, new, keys7 + "ema_decay: 0.9\n", 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert p.returncode == 0 and 7 in _sections(ck7.read_bytes()), p.stderr[-2000:]
    res = _run_trainer(ema_trainer, new, keys7 + f"resume: {ck7}\n", 4)
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert _calls(res) == [] and "aleppo_ema_open" not in res.stderr and "averaged parameters" not in res.stdout + res.stderr
    assert sorted(_sections(ck7.read_bytes())) == [1, 2, 3, 4, 5, 6]
    # a section of the wrong size is refused
    p = _run_trainer(ema_trainer, new, keys7 + "ema_decay: 0.9\n", 2)
    assert p.returncode == 0, p.stderr[-2000:]
    blob = ck7.read_bytes()
    at = blob.rindex(struct.pack("<IQ", 7, N_PARAMS * 4 + 8))
    bad = blob[:at] + struct.pack("<IQ", 7, N_PARAMS * 4) + blob[at + 12:-16] + blob[-8:]
    (new / "bad.ckpt").write_bytes(bad)
    res = _run_trainer(ema_trainer, new, f"resume: {new / 'bad.ckpt'}\nema_decay: 0.9\n", 4)
    assert res.returncode == 1 and "section 7" in res.stderr and "corrupt" in res.stderr, res.stderr[-2000:]


@pytest.mark.parametrize("device", [False, True])
def test_eval_averaged_sets_the_option_before_the_first_evaluation(ema_trainer, tmp_path, device):
    extra = "ema_decay: 0.9\neval_averaged: true\neval_interval: 2\neval_environments: 2\neval_episodes: 2\n"
    if device:
        extra += "device_evaluation: true\n"
    r = _run_trainer(ema_trainer, tmp_path, extra, 2)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    assert r.stderr.count("stub: aleppo_set_option ALEPPO_OPT_EVAL_PARAMS value=1") == 1
    at = r.stderr.index("stub: aleppo_set_option ALEPPO_OPT_EVAL_PARAMS value=1")
    assert r.stderr.index("stub: aleppo_ema_open") < at < r.stderr.index("stub: aleppo_ema_update decay")
    blob = trainer_helpers.events(tmp_path / "tb")
    assert b"eval_averaged" in blob and b"eval/episode_return_mean" in blob
    # without the key the option is never set
    (tmp_path / "off").mkdir()
    r = _run_trainer(ema_trainer, tmp_path / "off", "ema_decay: 0.9\neval_interval: 2\neval_environments: 2\neval_episodes: 2\n", 2)
    assert r.returncode == 0 and "ALEPPO_OPT_EVAL_PARAMS" not in r.stderr, r.stderr[-2000:]
    assert b"eval_averaged" not in trainer_helpers.events(tmp_path / "off" / "tb")


@pytest.mark.parametrize("extra,message", [
    ("ema_warmup: true\n", "ema_warmup needs ema_decay"),
    ("ema_warmup: false\n", "ema_warmup needs ema_decay"),
    ("eval_averaged: true\neval_interval: 2\n", "eval_averaged needs ema_decay"),
    ("ema_decay: 0.9\neval_averaged: true\n", "eval_averaged needs eval_interval > 0"),
    ("ema_decay: 1\n", "ema_decay must be in [0, 1)"),
    ("ema_decay: 1.5\n", "ema_decay must be in [0, 1)"),
    ("ema_decay: -0.1\n", "ema_decay must be in [0, 1)"),
    ("ema_decay: nan\n", "ema_decay"),
    ("ema_decay: inf\n", "ema_decay"),
    ("ema_decay: often\n", "bad value for ema_decay"),
])
def test_trainer_refuses_bad_keys(ema_trainer, tmp_path, extra, message):
    r = _run_trainer(ema_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == [] and "aleppo_ema_open" not in r.stderr


def test_library_without_the_entry_points_refuses_the_key(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_tsan"])
    plain = os.path.join(ROOT, "trainer", "train_tsan")  # (the stand-in without the averaged parameters)
    r = _run_trainer(plain, tmp_path, "ema_decay: 0.9\n", 2)
    assert r.returncode == 1 and "aleppo_ema_open is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
