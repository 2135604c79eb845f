"""The trainer's record_saliency keys on the host-only stand-in (tests/stub/aleppo_stub_saliency.cc, which counts its
calls, records their arguments and scores by a closed formula of (sample, gy, gx)): the defaults, the interval's call
count, the arguments, every byte of the y4m files - the zero-maximum case included - and every start-up refusal.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import saliency_ref as sr
import trainer_helpers
from conftest import ROOT

CALL = re.compile(r"stub: aleppo_saliency first=(-?\d+) n=(-?\d+) stride=(\d+) planes=(\d+) sigma_mask=(\S+) sigma_blur=(\S+) "
                  r"batch=(\d) outputs=(\d)")
HEADER = b"YUV4MPEG2 W84 H84 F15:1 Ip A1:1 C444 XALEPPO_Y=channel0_newest\n"
T = 32  # debug.yaml's horizon


def _run_trainer(binary, d, extra, rollouts=4, env=None):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d / "video"), "g", str(cfg)],
                          capture_output=True, text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def sal_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_sal_stub"])
    return os.path.join(ROOT, "trainer", "train_sal_stub")


def _calls(r):
    m = re.search(r"stub: aleppo_saliency calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    recorded = [dict(first=int(f), n=int(n), stride=int(s), planes=int(p), sigma_mask=float(a), sigma_blur=float(b),
                     batch=int(ba), outputs=int(o)) for f, n, s, p, a, b, ba, o in CALL.findall(r.stderr)]
    assert len(recorded) == int(m.group(1))
    return recorded


def _files(d):
    v = d / "video"
    return sorted(os.listdir(v)) if v.exists() else []


def _expected_frames(stride):
    """the U and V planes [T, 84, 84] the stand-in's formula gives: S_policy = (s + 1) p, S_value = (s + 1) (P - 1 - p)"""
    G = sr.grid(stride)
    P = G * G
    p = np.arange(P, dtype=np.float32).reshape(G, G)
    s = np.arange(1, T + 1, dtype=np.float32)[:, None, None]
    pol, val = s * p, s * (P - 1 - p)
    return (sr.uv_bytes(sr.upsample(pol, stride), float(pol.max())), sr.uv_bytes(sr.upsample(val, stride), float(val.max())))


def _check_file(path, stride):
    blob = open(path, "rb").read()
    assert blob.startswith(HEADER)
    frame = 6 + 3 * 7056
    assert len(blob) == len(HEADER) + T * frame  # T frames, nothing else
    frames = np.frombuffer(blob, np.uint8, offset=len(HEADER)).reshape(T, frame)
    assert (frames[:, :6] == np.frombuffer(b"FRAME\n", np.uint8)).all()
    yuv = frames[:, 6:].reshape(T, 3, 84, 84)
    assert not yuv[:, 0].any()  # (the stand-in's batch read returns zeros)
    u, v = _expected_frames(stride)
    assert np.array_equal(yuv[:, 1], u) and np.array_equal(yuv[:, 2], v)
    return yuv


def test_trainer_keys_with_the_stub_library(sal_trainer, tmp_path):
    # name, keys, rollouts, the 1-based rollouts that write a file, (stride, sigma_mask, sigma_blur)
    runs = (("absent", "", 3, [], None), ("false", "record_saliency: false\n", 3, [], None),
            ("defaults", "record_saliency: true\n", 3, [1, 2, 3], (5, 5.0, 3.0)),
            ("every2", "record_saliency: true\nsaliency_interval: 2\nsaliency_stride: 12\nsaliency_sigma_mask: 2.5\n"
                       "saliency_sigma_blur: 1\n", 5, [2, 4], (12, 2.5, 1.0)),
            ("one point", "record_saliency: true\nsaliency_interval: 3\nsaliency_stride: 84\n", 3, [3], (84, 5.0, 3.0)))
    blobs = {}
    for name, extra, rollouts, when, k in runs:
        d = tmp_path / name.replace(" ", "_")
        d.mkdir()
        r = _run_trainer(sal_trainer, d, extra, rollouts)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        calls = _calls(r)
        assert len(calls) == len(when), name
        for c in calls:  # environment 0's T samples of the batch, all planes, no raw outputs
            assert c == dict(first=0, n=T, stride=k[0], planes=15, sigma_mask=k[1], sigma_blur=k[2], batch=1, outputs=0), (name, c)
        assert _files(d) == sorted(f"saliency_{n}.y4m" for n in when), name  # (no .part left behind)
        for n in when:
            yuv = _check_file(d / "video" / f"saliency_{n}.y4m", k[0])
            if k[0] == 84:  # one grid point: both maxima are zero, so both planes are 128
                assert (yuv[:, 1:] == 128).all()
            else:  # the largest score of the file is in the last frame: 255 there, and nowhere in the first frame
                assert yuv[-1, 1].max() == 255 and yuv[-1, 2].max() == 255 and yuv[0, 1].max() < 255 and yuv[:, 1:].min() == 128
        blobs[name] = trainer_helpers.events(d / "tb")
        assert (b"record_saliency" in blobs[name]) == (name not in ("absent", "false"))  # the hparams flag, only when set


@pytest.mark.parametrize("extra,message", [
    ("saliency_interval: 2\n", "saliency_interval needs record_saliency: true"),
    ("saliency_stride: 7\n", "saliency_stride needs record_saliency: true"),
    ("saliency_sigma_mask: 4\n", "saliency_sigma_mask needs record_saliency: true"),
    ("saliency_sigma_blur: 2\n", "saliency_sigma_blur needs record_saliency: true"),
    ("record_saliency: false\nsaliency_stride: 7\n", "saliency_stride needs record_saliency: true"),
    ("record_saliency: true\nsaliency_interval: 0\n", "saliency_interval must be positive"),
    ("record_saliency: true\nsaliency_interval: -2\n", "saliency_interval must be positive"),
    ("record_saliency: true\nsaliency_stride: 1\n", "saliency_stride must be in [2, 84]"),
    ("record_saliency: true\nsaliency_stride: 85\n", "saliency_stride must be in [2, 84]"),
    ("record_saliency: true\nsaliency_stride: wide\n", "bad value for saliency_stride"),
    ("record_saliency: true\nsaliency_sigma_mask: 0.25\n", "saliency_sigma_mask must be in [0.5, 16]"),
    ("record_saliency: true\nsaliency_sigma_mask: 16.5\n", "saliency_sigma_mask must be in [0.5, 16]"),
    ("record_saliency: true\nsaliency_sigma_mask: nan\n", "saliency_sigma_mask"),
    ("record_saliency: true\nsaliency_sigma_blur: 0.1\n", "saliency_sigma_blur must be in [0.5, 10]"),
    ("record_saliency: true\nsaliency_sigma_blur: 11\n", "saliency_sigma_blur must be in [0.5, 10]"),
    ("record_saliency: true\nsaliency_sigma_blur: soft\n", "bad value for saliency_sigma_blur"),
])
def test_trainer_refuses_bad_keys(sal_trainer, tmp_path, extra, message):
    r = _run_trainer(sal_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == [] and _files(tmp_path) == []


def test_library_without_the_symbol_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without aleppo_saliency)
    r = _run_trainer(plain, tmp_path, "record_saliency: true\n", 2)
    assert r.returncode == 1 and "aleppo_saliency is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
