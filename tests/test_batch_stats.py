"""ALEPPO_F_BATCH_STATS (include/aleppo.h): explained variance and the mean / std of the values, returns, advantages and
residuals of the batch a context holds, reduced on the device when read.  CPU: the reference's known answers, the header
against the Python mirror, the trainer's log_batch_stats key on the host-only library stand-in.  GPU: the field through
the C ABI against tests/batch_stats_ref.py (its derived bound), its determinism, its errors, and that reading it changes
nothing else."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import batch_stats_ref as br
import hashfill as hf
import oracle_lib as orc
from trainer_helpers import debug_cfg as _debug_cfg, events as _events, header_const as const
from shared_fixtures import pkg, stub_trainer, trainer  # noqa: F401
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_TAGS = (b"explained_variance", b"mean_value", b"std_value", b"mean_return", b"std_return", b"mean_advantage",
            b"std_advantage")


# ------------------------------------------------------------------ CPU
def _planes(seed, N, masked=0.1):
    v = hf.hf_range(seed, (N,), -1, 2)
    r = hf.hf_range(seed + 1, (N,), -2, 3)
    a = hf.hf_range(seed + 2, (N,), -1, 1)
    m = (hf.hf_unit(seed + 3, N) >= np.float32(masked)).astype(np.uint8)
    return v, r, a, m


def test_reference_known_answers():
    v, r, a, m = _planes(7000, 1000)
    s, _ = br.reference(r, r, a, m)  # v = R
    assert s["explained_variance"] == 1.0 and s["residual_mean"] == 0.0 and s["residual_std"] == 0.0
    s, _ = br.reference(np.full_like(r, 0.25), r, a, m)  # v constant, R varying
    assert abs(s["explained_variance"]) < 1e-12 and s["value_std"] == 0.0 and s["value_mean"] == 0.25
    # v = R + c: the residual is the constant -c up to the rounding of R + c to float32
    c = np.float32(0.5)
    s, _ = br.reference(r + c, r, a, m)
    assert abs(s["explained_variance"] - 1.0) < 1e-12 and abs(s["residual_mean"] + 0.5) < 1e-6
    # v = 2 R exactly (a power-of-two multiple is exact in float32): d = -R, var(d) = var(R)
    s, _ = br.reference(2 * r, r, a, m)
    assert s["explained_variance"] == 0.0
    np.testing.assert_array_equal((2 * r).astype(np.float64), 2 * r.astype(np.float64))
    s, b = br.reference(v, np.full_like(r, 1.5), a, m)  # constant R
    assert np.isnan(s["explained_variance"]) and s["return_std"] == 0.0 and s["return_mean"] == 1.5
    s, b = br.reference(v, r, a, np.zeros_like(m))  # all masked
    assert s["count"] == 0 and np.isnan(s["explained_variance"])
    assert all(s[k] == 0.0 for k in br.NAMES[2:])
    s, _ = br.reference(v, r, a, m)
    assert s["count"] == m.sum() and 0 < s["count"] < 1000
    np.testing.assert_allclose(s["advantage_std"], np.std(a[m != 0].astype(np.float64)))
    d = r.astype(np.float64) - v.astype(np.float64)
    np.testing.assert_allclose(s["explained_variance"], 1 - np.var(d[m != 0]) / np.var(r[m != 0].astype(np.float64)))


@pytest.mark.parametrize("N", [1, 512, 5000, 65536 + 77, 524288])
def test_one_pass_sum_in_the_device_order_stays_inside_the_bound(N):
    """the order the kernels sum in, restated in numpy, against the two-pass reference: far inside the derived bound"""
    v, r, a, m = _planes(7100 + N % 97, N)
    m[0] = 1
    stats, bounds = br.reference(v, r, a, m)
    got = br.one_pass_in_device_order(v, r, a, m)
    if N > 1:
        br.assert_close(got, stats, bounds, f"N={N}")
        worst = max(abs(got[k] - stats[k]) / bounds[k] for k in br.NAMES[1:])
        assert worst < 0.05, worst  # (the bound is a worst case: a fraction of it is used)
    else:
        assert all(got[k] == stats[k] or (np.isnan(got[k]) and np.isnan(stats[k])) for k in br.NAMES)


def test_header_constants_and_python_mirror():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()

    assert const("ALEPPO_F_BATCH_STATS") == pkg.FIELDS["batch_stats"] == 13
    m = re.search(r"(?m)^#define ALEPPO_BATCH_STATS_COUNT (\d+)", hdr)
    assert m and int(m.group(1)) == pkg.BATCH_STATS_COUNT == 10 == len(br.NAMES)
    for i, name in enumerate(br.NAMES):
        assert const("ALEPPO_BS_" + name.upper()) == pkg.BATCH_STATS[name] == i
    assert len(pkg.BATCH_STATS) == 10
    assert hasattr(pkg.Engine, "batch_stats")
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _run_trainer(binary, d, extra, rollouts, env=None):
    os.makedirs(d / "tb")
    cfg = _debug_cfg(d, extra, rollouts)
    r = subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return _events(d / "tb")


def test_trainer_key_with_the_stub_library(stub_trainer, tmp_path):
    blobs = {}
    for name, extra in (("absent", ""), ("false", "log_batch_stats: false\n"), ("true", "log_batch_stats: true\n")):
        (tmp_path / name).mkdir()
        blobs[name] = _run_trainer(stub_trainer, tmp_path / name, extra, 3)
    tags = {k: _scalar_bits(b) for k, b in blobs.items()}
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    assert not set(NEW_TAGS) & set(tags["absent"])
    assert set(tags["true"]) == set(tags["absent"]) | set(NEW_TAGS)  # nothing else appears or goes
    for tag in NEW_TAGS:
        assert len(tags["true"][tag]) == 3 == len(tags["true"][b"mean_loss"]), tag  # once per trained rollout
    assert b"log_batch_stats" in blobs["true"]  # the hparams flag, only when set
    assert b"log_batch_stats" not in blobs["absent"] and b"log_batch_stats" not in blobs["false"]
    for tag in tags["absent"]:  # (the stand-in is deterministic: the other scalars do not move)
        assert tags["absent"][tag] == tags["true"][tag], tag


# ------------------------------------------------------------------ GPU
class _DeviceBytes:
    """device copy of a numpy array (no torch in the test process)"""

    def __init__(self, arr):
        self.hip = ctypes.CDLL("libamdhip64.so")
        arr = np.ascontiguousarray(arr)
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(arr.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes), 1) == 0

    @property
    def addr(self):
        return self.ptr.value

    def free(self):
        self.hip.hipFree(self.ptr)


def _flags(seed, T, E, p_term=0.02, p_trunc=0.01):
    """slot protocol of the rollout: a terminated / truncated slot is followed by one episode-start slot (about 3 % of
    the slots of a long rollout, beside the E start slots of slot 0)"""
    rng = np.random.default_rng(seed)
    te, tr, st = (np.zeros((T, E), np.uint8) for _ in range(3))
    start = np.ones(E, np.uint8)
    for t in range(T):
        u = rng.random(E)
        st[t] = start
        te[t] = (u < p_term) & (start == 0)
        tr[t] = (u >= p_term) & (u < p_term + p_trunc) & (start == 0)
        start = (te[t] | tr[t]).astype(np.uint8)
    return te, tr, st


def _rollout(pkg, E, T, seed, prec=None, A=4, H=32, **kw):
    """an engine holding a finished rollout: hash-filled frames (a block of environments, byte-permuted across the
    rest), random rewards and flags"""
    eb = min(E, 32)
    base = hf.hf_bytes(seed, (T, eb, 84, 84))
    frames = np.concatenate([base ^ np.uint8(37 * k % 256) for k in range((E + eb - 1) // eb)], axis=1)[:, :E]
    dev = _DeviceBytes(frames)
    te, tr, st = _flags(seed + 1, T, E)
    rew = hf.hf_range(seed + 2, (T * E,), -2, 2).reshape(T, E)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec is None else prec, seed=3, **kw)
    eng.load_params(hf.fill_params(seed + 3, H, A))
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
    eng.finish_rollout()
    dev.free()
    return eng


def _ref_of_engine(eng):
    b = {k: eng.read_batch(k) for k in ("values", "returns", "advantages", "masks")}
    return br.reference(b["values"], b["returns"], b["advantages"], b["masks"]), b


def _bits(stats):
    return struct.pack("<10d", *[stats[k] for k in br.NAMES])


@pytest.mark.gpu
@pytest.mark.parametrize("E,T,prec,H", [(16, 32, "fp32", 32), (130, 41, "fp32", 32), (4096, 5, "fp32", 32),
                                        (128, 128, "bf16", 512), (1024, 65, "bf16", 64)])
def test_rollout_batch_vs_reference(pkg, E, T, prec, H):
    """(1024, 65): 66 560 samples, 17 partials for the second stage, the last chunk partly filled"""
    eng = _rollout(pkg, E, T, 7200 + E, prec=pkg.BF16 if prec == "bf16" else pkg.FP32, H=H)
    got = eng.batch_stats()
    (stats, bounds), b = _ref_of_engine(eng)
    eng.close()
    assert 0 < stats["count"] < E * T and stats["count"] == b["masks"].sum()  # (the mask matters)
    assert stats["value_std"] > 0 and np.isfinite(stats["explained_variance"])
    br.assert_close(got, stats, bounds, f"rollout {E}x{T} {prec}")


@pytest.mark.gpu
@pytest.mark.parametrize("E,T", [(16, 32), (130, 41)])
def test_fp16_rollout_planes_vs_reference_on_the_rounded_planes(pkg, E, T):
    eng = _rollout(pkg, E, T, 7300 + E, rollout_precision=pkg.ROLLOUT_FP16)
    got = eng.batch_stats()
    (stats, bounds), b = _ref_of_engine(eng)
    eng.close()
    for k in ("values", "returns", "advantages"):  # what read_batch returns IS the stored fp16 value
        np.testing.assert_array_equal(b[k], b[k].astype(np.float16).astype(np.float32))
    br.assert_close(got, stats, bounds, f"fp16 planes {E}x{T}")


def _caller_engine(pkg, E, T, v, r, a, m, A=4, H=32, values=True, **kw):
    N = len(r)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, **kw)
    eng.load_params(hf.fill_params(7401, H, A))
    obs = hf.hf_bytes(7402, (N, 4, 84, 84))
    actions = (hf.hf_u32(7403, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(7404, (N, A), -1, 1))
    eng.set_batch(obs, actions, old_lp, a, r, m, values=v if values else None)
    return eng


CALLER_CASES = ("generic", "short", "v_equals_R", "constant_R", "all_masked", "one_sample")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CALLER_CASES)
def test_caller_batch(pkg, case):
    E, T = 24, 16
    N = 300 if case == "short" else E * T  # (short: fewer samples than E*T - the batch's own count is used)
    v, r, a, m = _planes(7400, N)
    if case == "v_equals_R":
        v = r.copy()
    elif case == "constant_R":
        r = np.full(N, 1.5, np.float32)
    elif case == "all_masked":
        m = np.zeros(N, np.uint8)
    elif case == "one_sample":
        m = np.zeros(N, np.uint8)
        m[N // 3] = 1
    eng = _caller_engine(pkg, E, T, v, r, a, m)
    got = eng.batch_stats()
    eng.close()
    stats, bounds = br.reference(v, r, a, m)
    for plane in (v, r, a):  # |mean| at most 3 std on every plane that varies: the bound stays small
        x = plane[m != 0].astype(np.float64)
        assert x.size < 2 or np.var(x) == 0 or abs(x.mean()) <= 3 * x.std()
    br.assert_close(got, stats, bounds, case)
    if case == "v_equals_R":
        assert got["explained_variance"] == 1.0 and got["residual_std"] == 0.0 and got["residual_mean"] == 0.0
    if case == "constant_R":
        assert np.isnan(got["explained_variance"]) and got["return_std"] == 0.0 and got["return_mean"] == 1.5
    if case == "all_masked":
        assert got["count"] == 0 and np.isnan(got["explained_variance"])
        assert all(got[k] == 0.0 for k in br.NAMES[2:])
    if case == "one_sample":
        assert got["count"] == 1 and np.isnan(got["explained_variance"])
        assert got["value_mean"] == float(v[N // 3]) and got["return_mean"] == float(r[N // 3])
        assert all(got[k + "_std"] == 0.0 for k in ("value", "return", "advantage", "residual"))


@pytest.mark.gpu
def test_reads_are_deterministic_and_survive_the_update(pkg):
    E, T, epochs, M = 64, 20, 2, 4
    eng = _rollout(pkg, E, T, 7500)
    first, second = eng.batch_stats(), eng.batch_stats()
    assert _bits(first) == _bits(second)
    for opt in (pkg.OPT_MINIBATCH_SHUFFLE, pkg.OPT_VALUE_CLIP, pkg.OPT_ADV_NORM_MINIBATCH):
        eng.set_option(opt, 1)
    m = eng.train(2.5e-4, epochs, M)
    assert np.isfinite(m["loss"]).all()
    assert (eng.sample_order(epochs) != np.arange(E * T)).any()  # (the update did shuffle)
    assert _bits(eng.batch_stats()) == _bits(first)
    eng.close()
    # a caller batch: before / after an update that clips values (val_n is both the update's and the read's source)
    v, r, a, mk = _planes(7510, E * T)
    eng = _caller_engine(pkg, E, T, v, r, a, mk)
    first = eng.batch_stats()
    for opt in (pkg.OPT_MINIBATCH_SHUFFLE, pkg.OPT_VALUE_CLIP, pkg.OPT_ADV_NORM_MINIBATCH):
        eng.set_option(opt, 1)
    eng.train(2.5e-4, epochs, M)
    assert _bits(eng.batch_stats()) == _bits(first)
    eng.close()


@pytest.mark.gpu
def test_one_rank_communicator_path_is_bit_identical(pkg):
    """the data-parallel path (sums all-reduced as doubles, then finalised) with a 1-rank RCCL communicator and
    ALEPPO_OPT_FORCE_COMM against the same engine without the option"""
    E, T = 130, 41  # (two chunks, the second partly filled)
    eng = _rollout(pkg, E, T, 7600)
    plain = eng.batch_stats()
    eng.comm_init(pkg.Engine.comm_unique_id())
    eng.set_option(pkg.OPT_FORCE_COMM, 1)
    forced = eng.batch_stats()
    eng.set_option(pkg.OPT_FORCE_COMM, 0)
    again = eng.batch_stats()
    (stats, bounds), _ = _ref_of_engine(eng)
    eng.close()
    assert _bits(plain) == _bits(forced) == _bits(again)
    br.assert_close(forced, stats, bounds, "1-rank communicator")


@pytest.mark.gpu
def test_reading_the_statistics_changes_nothing_else(pkg):
    E, T, epochs, M = 32, 16, 2, 4
    out = []
    for read in (False, True):
        eng = _rollout(pkg, E, T, 7700)
        eng.set_option(pkg.OPT_VALUE_CLIP, 1)
        if read:
            eng.batch_stats()
            eng.batch_stats()
        m = eng.train(2.5e-4, epochs, M)
        B = E * T // M
        planes = {k: eng.read_train_metric(k, epochs, M, B) for k in pkg.METRIC_FIELDS if k != "kl"}
        out.append((m, eng.export_params(), eng.state_dict(), eng.train_diagnostics(epochs, M), planes))
        eng.close()
    (m0, p0, sd0, d0, pl0), (m1, p1, sd1, d1, pl1) = out
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    np.testing.assert_array_equal(p0, p1)
    assert set(sd0) == set(sd1) and len(sd0) >= 3
    for k in sd0:  # parameters, Adam moments, step
        np.testing.assert_array_equal(np.asarray(sd0[k]), np.asarray(sd1[k]), err_msg=k)
    for k in d0:
        np.testing.assert_array_equal(d0[k], d1[k], err_msg=k)
    for k in pl0:
        np.testing.assert_array_equal(pl0[k], pl1[k], err_msg=k)


@pytest.mark.gpu
def test_whole_batch_advantage_normalisation_shows_in_the_advantage_statistics_only(pkg):
    E, T = 64, 32
    got = []
    for norm in (False, True):
        eng = _rollout(pkg, E, T, 7800, advantage_norm=norm)
        got.append(eng.batch_stats())
        (stats, bounds), _ = _ref_of_engine(eng)
        br.assert_close(got[-1], stats, bounds, f"advantage_norm={norm}")
        eng.close()
    off, on = got
    for k in br.NAMES:
        if not k.startswith("advantage"):
            assert struct.pack("<d", off[k]) == struct.pack("<d", on[k]), k
    n = on["count"]
    assert n > 100
    # the normalised plane: mean 0, unbiased std 1, so population std sqrt((n - 1) / n); the normalisation sums in fp32,
    # hence the loose figure - it checks the wiring, not the arithmetic
    assert abs(on["advantage_mean"]) <= 1e-3
    assert abs(on["advantage_std"] - np.sqrt((n - 1) / n)) <= 1e-3
    assert abs(off["advantage_std"] - 1.0) > 1e-2 or abs(off["advantage_mean"]) > 1e-2


@pytest.mark.gpu
def test_error_cases(pkg):
    E, T, A, H = 8, 8, 4, 32
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    eng.load_params(hf.fill_params(7900, H, A))
    out = np.zeros(10, np.float64)

    def read(nbytes):
        return pkg.lib().aleppo_read_batch(eng._ctx, pkg.FIELDS["batch_stats"], out.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_size_t(nbytes))

    with pytest.raises(pkg.AleppoError, match="no batch"):  # before any batch
        eng.batch_stats()
    v, r, a, m = _planes(7901, E * T)
    obs = hf.hf_bytes(7902, (E * T, 4, 84, 84))
    actions = (hf.hf_u32(7903, E * T) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(7904, (E * T, A), -1, 1))
    eng.set_batch(obs, actions, old_lp, a, r, m)
    with pytest.raises(pkg.AleppoError, match="aleppo_set_batch_values"):  # a caller batch without values
        eng.batch_stats()
    eng.set_batch_values(v)
    for nbytes in (0, 8, 72, 88, 40):  # wrong byte counts
        assert read(nbytes) == pkg.ERR_INVALID_ARGUMENT
    assert read(80) == pkg.OK and out[0] == m.sum()
    eng.set_batch(obs, actions, old_lp, a, r, m)  # (a new caller batch forgets the values)
    with pytest.raises(pkg.AleppoError, match="aleppo_set_batch_values"):
        eng.batch_stats()
    eng.close()
    # while a step is armed: refused like every other call; after the release the rollout finishes normally
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    eng.load_params(hf.fill_params(7900, H, A))
    frames = hf.hf_bytes(7905, (T, E * 7056))
    starts = np.zeros((T, E), np.uint8)
    starts[0] = 1
    zeros = np.zeros(E, np.uint8)
    rew = hf.hf_range(7906, (T, E), -1, 1)
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    for t in range(T):  # the armed loop of test_gpu_at_size.py: act, arm, the "emulator" fills the buffers, release
        eng.act()
        eng.arm_step(fbuf, sbuf)
        if t == 3:
            with pytest.raises(pkg.AleppoError, match="armed"):
                eng.batch_stats()
        ctypes.memmove(fbuf, frames[t].ctypes.data, E * 7056)
        ctypes.memmove(sbuf, starts[t].ctypes.data, E)
        eng.release_step(rew[t], zeros, zeros)
    eng.finish_rollout()
    got = eng.batch_stats()
    (stats, bounds), _ = _ref_of_engine(eng)
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
    assert got["count"] == E * (T - 1)
    br.assert_close(got, stats, bounds, "after an armed step")


@pytest.mark.gpu
def test_trainer_on_the_device(trainer, tmp_path):
    tags = {}
    for name, extra in (("off", ""), ("on", "log_batch_stats: true\n")):
        (tmp_path / name).mkdir()
        tags[name] = _scalar_bits(_run_trainer(trainer, tmp_path / name, extra, 5))
    assert set(tags["on"]) == set(tags["off"]) | set(NEW_TAGS) and not set(NEW_TAGS) & set(tags["off"])
    f32 = lambda bits: np.array(bits, np.uint32).view(np.float32)  # noqa: E731
    for tag in NEW_TAGS:
        assert len(tags["on"][tag]) == 5, tag
        print(tag, f32(tags["on"][tag]))
    ev = f32(tags["on"][b"explained_variance"])
    assert (np.isfinite(ev) | np.isnan(ev)).all() and (ev[np.isfinite(ev)] <= 1.0).all()
    assert np.isfinite(f32(tags["on"][b"mean_return"])).all()
    for tag in (b"std_value", b"std_return", b"std_advantage"):
        assert (f32(tags["on"][tag]) >= 0).all(), tag
    assert b"mean_loss" in tags["off"] and len(tags["off"][b"mean_loss"]) == 5
    for tag in tags["off"]:  # deterministic: true - the run's other scalars are bit-identical
        assert tags["off"][tag] == tags["on"][tag], tag


# ------------------------------------------------------------------ two ranks, real RCCL (needs >= 2 GPUs)
_DP_SCRIPT = r'''
import os, sys
root, rank, idfile, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import time
import numpy as np
import hashfill as hf, oracle_lib as orc
from __graft_entry__ import load_package
pkg = load_package()
WORLD, EG, T, H, A = 2, 40, 128, 32, 4
if rank == 0:
    open(idfile + ".tmp", "wb").write(pkg.Engine.comm_unique_id()); os.replace(idfile + ".tmp", idfile)
t0 = time.time()
while not os.path.exists(idfile):
    assert time.time() - t0 < 120
    time.sleep(0.05)
uid = open(idfile, "rb").read()
NL = EG * T
N = WORLD * NL
v = hf.hf_range(8000, (N,), -1, 2); r = hf.hf_range(8001, (N,), -2, 3); a = hf.hf_range(8002, (N,), -1, 1)
m = (hf.hf_unit(8003, N) >= np.float32(0.1 + 0.3 * (np.arange(N) >= NL))).astype(np.uint8)  # uneven counts across ranks
rows = slice(rank * NL, (rank + 1) * NL)
eng = pkg.Engine(EG, T, A, H, precision=pkg.FP32, device=rank, world_size=WORLD, rank=rank)
eng.comm_init(uid)
eng.load_params(hf.fill_params(8004, H, A))
obs = np.zeros((NL, 4, 84, 84), np.uint8); actions = np.zeros(NL, np.int64)
old_lp = orc.log_softmax(np.zeros((NL, A), np.float32))
eng.set_batch(obs, actions, old_lp, a[rows], r[rows], m[rows], values=v[rows])
s = eng.batch_stats()
s2 = eng.batch_stats()
assert s == s2 or (np.isnan(s["explained_variance"]) and np.isnan(s2["explained_variance"]))
np.save(os.path.join(outdir, f"stats{rank}.npy"), np.array([s[k] for k in pkg.BATCH_STATS]))
eng.close()
print("DP_RANK_OK", rank)
'''


def _gpu_count():
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


@pytest.mark.gpu
def test_two_rank_statistics_are_those_of_the_concatenated_planes(tmp_path):
    """Two processes, one GPU each, real RCCL: both ranks read the statistics of the union of their samples, equal to the
    reference over the concatenated planes.  Skips on a one-GPU box."""
    if _gpu_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    script = tmp_path / "dp_rank.py"
    script.write_text(_DP_SCRIPT)
    idfile = str(tmp_path / "nccl_id.bin")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), idfile, str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=420)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"DP_RANK_OK {r}" in o, o[-4000:]
    N = 2 * 40 * 128
    v, r_, a = hf.hf_range(8000, (N,), -1, 2), hf.hf_range(8001, (N,), -2, 3), hf.hf_range(8002, (N,), -1, 1)
    m = (hf.hf_unit(8003, N) >= np.float32(0.1 + 0.3 * (np.arange(N) >= N // 2))).astype(np.uint8)
    stats, bounds = br.reference(v, r_, a, m)
    s0, s1 = np.load(tmp_path / "stats0.npy"), np.load(tmp_path / "stats1.npy")
    assert s0.tobytes() == s1.tobytes()  # every rank finalises the same all-reduced sums
    br.assert_close(dict(zip(br.NAMES, s0)), stats, bounds, "two ranks")
