"""The trainer's recycle_dormant keys on the host-only stand-in (tests/stub/aleppo_stub_recycle.cc, which counts its calls
and records their arguments): the defaults, the interval's call count, the key as a function of the rollout index, the
logged counts, and every start-up refusal.  No GPU."""
import os
import re
import struct
import subprocess

import pytest

import recycle_ref as rr
import trainer_helpers
from conftest import ROOT

TAGS = [f"recycle/{l}/units".encode() for l in rr.LAYERS] + [b"recycle/total"]
CALL = re.compile(r"stub: aleppo_recycle_dormant tau=(\S+) layers=(\d+) key=([0-9a-f]{16}) flags=(\d+) batch=(\d) mask_out=(\d)")


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _run_trainer(binary, d, extra, rollouts=4, env=None):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def recycle_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_recycle_stub"])
    return os.path.join(ROOT, "trainer", "train_recycle_stub")


def _calls(r):
    m = re.search(r"stub: aleppo_recycle_dormant calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    recorded = [dict(tau=float(t), layers=int(l), key=int(k, 16), flags=int(f), batch=int(b), mask_out=int(mo))
                for t, l, k, f, b, mo in CALL.findall(r.stderr)]
    assert len(recorded) == int(m.group(1))
    return recorded


def _seed(cfg_text):
    m = re.findall(r"(?m)^seed:\s*(\d+)", cfg_text)
    return int(m[-1]) if m else 42  # (the last one given counts; none: Config's default)


def test_trainer_keys_with_the_stub_library(recycle_trainer, tmp_path):
    # name, keys, rollouts, the 0-based rollout indices that recycle, tau, layer bits
    runs = (("absent", "", 4, [], None, None), ("false", "recycle_dormant: false\n", 4, [], None, None),
            ("defaults", "recycle_dormant: true\n", 4, [], None, None),  # recycle_interval 64: none of 4 rollouts
            ("every1", "recycle_dormant: true\nrecycle_interval: 1\n", 4, [0, 1, 2, 3], 0.025, 15),
            ("every2", "recycle_dormant: true\nrecycle_interval: 2\nrecycle_tau: 0.1\nrecycle_layers: [conv2, fc]\n", 5,
             [1, 3], 0.1, 10),
            ("plain list", "recycle_dormant: true\nrecycle_interval: 3\nrecycle_layers: conv1\nseed: 7\n", 4, [2], 0.025, 1))
    tags, blobs = {}, {}
    for name, extra, rollouts, when, tau, bits in runs:
        d = tmp_path / name.replace(" ", "_")
        d.mkdir()
        r = _run_trainer(recycle_trainer, d, extra, rollouts)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        calls = _calls(r)
        seed = _seed((d / "d.yaml").read_text())
        assert [c["key"] for c in calls] == [rr.splitmix64(seed ^ i) for i in when], name
        for c in calls:  # the batch source, no flags, no mask asked for
            assert (c["tau"], c["layers"], c["flags"], c["batch"], c["mask_out"]) == (tau, bits, 0, 1, 0), (name, c)
        blobs[name] = trainer_helpers.events(d / "tb")
        tags[name] = _scalar_bits(blobs[name])
        f = lambda b: struct.unpack("<f", struct.pack("<I", b))[0]
        if when:
            # the stand-in reports l + 1 units for every asked-for layer l
            want = [l + 1 if bits >> l & 1 else 0 for l in range(4)]
            for tag, w in zip(TAGS, want + [sum(want)]):
                assert [f(b) for b in tags[name][tag]] == [float(w)] * len(when), (name, tag)
        else:
            assert not set(TAGS) & set(tags[name]), name
        assert (b"recycle_dormant" in blobs[name]) == (name not in ("absent", "false"))  # the hparams flag, only when set
    assert set(tags["absent"]) == set(tags["false"]) == set(tags["defaults"]) and b"mean_loss" in tags["absent"]
    assert set(tags["every1"]) == set(tags["absent"]) | set(TAGS)  # nothing else appears or goes
    for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
        assert tags["absent"][tag] == tags["every1"][tag], tag


def test_the_default_interval_is_64_rollouts(recycle_trainer, tmp_path):
    """ReDo's 1000 gradient steps at the benched configuration's 16 minibatch steps per rollout"""
    r = _run_trainer(recycle_trainer, tmp_path, "recycle_dormant: true\n", 64)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    calls = _calls(r)
    seed = _seed((tmp_path / "d.yaml").read_text())
    assert len(calls) == 1 and calls[0]["key"] == rr.splitmix64(seed ^ 63)
    assert calls[0]["tau"] == 0.025 and calls[0]["layers"] == 15


@pytest.mark.parametrize("extra,message", [
    ("recycle_interval: 2\n", "recycle_interval needs recycle_dormant: true"),
    ("recycle_tau: 0.1\n", "recycle_tau needs recycle_dormant: true"),
    ("recycle_layers: [fc]\n", "recycle_layers needs recycle_dormant: true"),
    ("recycle_dormant: false\nrecycle_tau: 0.1\n", "recycle_tau needs recycle_dormant: true"),
    ("recycle_dormant: true\nrecycle_tau: -0.1\n", "recycle_tau must be finite and non-negative"),
    ("recycle_dormant: true\nrecycle_tau: sometimes\n", "bad value for recycle_tau"),
    ("recycle_dormant: true\nrecycle_tau: nan\n", "recycle_tau"),
    ("recycle_dormant: true\nrecycle_interval: 0\n", "recycle_interval must be positive"),
    ("recycle_dormant: true\nrecycle_interval: -3\n", "recycle_interval must be positive"),
    ("recycle_dormant: true\nrecycle_layers: [conv1, conv4]\n", "recycle_layers: unknown layer 'conv4'"),
    ("recycle_dormant: true\nrecycle_layers: []\n", "recycle_layers"),
    ("recycle_dormant: true\nrecycle_layers: [fc,,conv1]\n", "recycle_layers: unknown layer ''"),
])
def test_trainer_refuses_bad_keys(recycle_trainer, tmp_path, extra, message):
    r = _run_trainer(recycle_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == []


def test_world_size_above_one_is_refused_at_start_up(recycle_trainer, tmp_path):
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = _run_trainer(recycle_trainer, tmp_path, "recycle_dormant: true\nrecycle_interval: 1\n", 2, env=env)
    assert r.returncode == 1 and "recycle_dormant needs WORLD_SIZE 1" in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == []


def test_library_without_the_symbol_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without aleppo_recycle_dormant)
    r = _run_trainer(plain, tmp_path, "recycle_dormant: true\n", 2)
    assert r.returncode == 1 and "aleppo_recycle_dormant is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
