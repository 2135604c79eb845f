"""aleppo_tensor_stats: per-tensor parameter, gradient and update norms reduced on the device.

CPU (not marked gpu): the header's constants against the Python mirror, the reference's known answers
(tests/tensor_stats_ref.py), the fp32 restatement of the update expression against its bound, and the trainer's
log_tensor_stats key on the host-only stand-in (tests/stub/aleppo_stub_tensor_stats.cc).
GPU: the call through the C ABI against the float64 reference built from the engine's own exports at the bounds derived
in tensor_stats_ref.py - after load_params, after updates, from imported hashed moments at t = 10^6, under a clip factor
below 1, with poisoned parameters - and its isolation: a context that reads the statistics computes what its twin
computes that never does."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adam_ref as ar
import hashfill as hf
import tensor_stats_ref as tr
import trainer_helpers
from conftest import ROOT
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

LR = 2.5e-4
U = ar.U


# ------------------------------------------------------------------ CPU: constants
def test_header_constants_match_the_python_mirror():
    pkg = load_package()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)

    const = functools.partial(trainer_helpers.header_const, stripped=True)

    assert const("ALEPPO_TENSOR_STATS_ROWS") == pkg.TENSOR_STATS_ROWS == tr.ROWS == 13
    assert const("ALEPPO_TENSOR_STATS_COLS") == pkg.TENSOR_STATS_COLS == tr.COLS == 10
    assert const("ALEPPO_TS_SEC_PARAMS") == pkg.TS_SEC_PARAMS == tr.SEC_PARAMS == 1
    assert const("ALEPPO_TS_SEC_STEP") == pkg.TS_SEC_STEP == tr.SEC_STEP == 2
    for i, name in enumerate(tr.STATS):
        assert const("ALEPPO_TS_" + name.upper()) == pkg.TENSOR_STATS[name] == i
    assert len(pkg.TENSOR_STATS) == 10
    assert list(pkg.TENSOR_NAMES) == list(ar.NAMES) + ["total"]
    assert "aleppo_tensor_stats" in pkg.EXPORTS and hasattr(pkg.Engine, "tensor_stats")
    assert re.search(r"int aleppo_tensor_stats\(aleppo_ctx \*ctx, int sections, double \*out, size_t count\);", hdr)
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


# ------------------------------------------------------------------ CPU: the reference's known answers
def test_reference_known_answers():
    pkg = load_package()  # (the reference's rows and columns are the library's)
    assert tr.NAMES == list(pkg.TENSOR_NAMES) and {n: i for i, n in enumerate(tr.STATS)} == pkg.TENSOR_STATS
    H, A = 32, 3
    offs = ar.param_offsets(H, A)
    n = int(offs[-1])
    params = hf.fill_params(8100, H, A)
    g = hf.hf_range(8101, (n,), -1, 1)
    zeros = np.zeros(n, np.float32)
    ref, rtol, atol = tr.reference(H, A, params, g, zeros, zeros, 3, LR)
    assert ref[12, tr.SIZE] == n == ref[:12, tr.SIZE].sum() and ref[11, tr.SIZE] == 1  # the sizes sum to param_count
    assert not ref[:, tr.UPDATE_NORM].any() and not ref[:, tr.UPDATE_MAXABS].any()  # all-zero moments: zero update
    assert not ref[:, tr.UPDATE_RATIO].any() and not ref[:, tr.STEP_NONFINITE].any()
    assert ref[11, tr.PARAM_NORM] == abs(float(params[-1])) == ref[11, tr.PARAM_MAXABS]  # value.b is one element
    assert ref[11, tr.GRAD_NORM] == abs(float(g[-1]))
    np.testing.assert_allclose(ref[12, tr.PARAM_NORM], np.linalg.norm(params.astype(np.float64)), rtol=1e-12)
    np.testing.assert_allclose(ref[6, tr.GRAD_NORM], np.linalg.norm(g[offs[6]:offs[7]].astype(np.float64)), rtol=1e-12)
    assert not tr.check(ref, ref, rtol, atol, 3)
    # one NaN in conv3.w: counted once in row 4 and row 12, excluded from the norms
    bad = params.copy()
    i = int(offs[4]) + 777
    bad[i] = np.nan
    ref2, _, _ = tr.reference(H, A, bad)
    assert ref2[4, tr.PARAM_NONFINITE] == 1 == ref2[12, tr.PARAM_NONFINITE] and ref2[:, tr.PARAM_NONFINITE].sum() == 2
    want = np.linalg.norm(np.delete(params[offs[4]:offs[5]], 777).astype(np.float64))
    np.testing.assert_allclose(ref2[4, tr.PARAM_NORM], want, rtol=1e-12)
    assert np.isfinite(ref2).all() and ref2[4, tr.PARAM_NORM] < ref[4, tr.PARAM_NORM]
    assert not ref2[:, tr.GRAD_NORM:].any()  # PARAMS alone: the step columns are 0
    # a NaN moment poisons the step group of that element only: counted once, g and u both left out
    m, v = ar.hashed_moments(8102, n)
    v = np.maximum(v, np.float32(1e-20))
    m2 = m.copy()
    j = int(offs[8]) + 5
    m2[j] = np.nan
    a, _, _ = tr.reference(H, A, params, g, m, v, 7, LR)
    b, _, _ = tr.reference(H, A, params, g, m2, v, 7, LR)
    assert b[8, tr.STEP_NONFINITE] == 1 == b[12, tr.STEP_NONFINITE] and not a[:, tr.STEP_NONFINITE].any()
    assert b[8, tr.GRAD_NORM] < a[8, tr.GRAD_NORM] and np.array_equal(a[:8], b[:8]) and np.array_equal(a[9:12], b[9:12])
    # the checker: a norm one part in 10^9 off is rejected, and so is a ratio one ulp off
    dev = a.copy()
    dev[6, tr.PARAM_NORM] *= 1 + 1e-9
    assert [f[:2] for f in tr.check(dev, *tr.reference(H, A, params, g, m, v, 7, LR), 3)] == [("fc.w", "param_norm")]
    dev = a.copy()
    dev[3, tr.UPDATE_RATIO] = np.nextafter(dev[3, tr.UPDATE_RATIO], 1)
    assert [f[0] for f in tr.check_ratio(dev)] == ["conv2.b"] and not tr.check_ratio(a)


def test_fp32_restatement_of_the_update_within_its_bound():
    """s (m / (sqrt(v) / c + eps)) in plain numpy float32 against the float64 evaluation on adam_ref's hashed inputs (|m| in
    1e-12 .. 1, v in 1e-24 .. 1, a fifth of them zero): at most 4.2u per element at t = 1, 2 and 10^6, under the 10u bound"""
    assert load_package().TENSOR_STATS["update_norm"] == tr.UPDATE_NORM  # (the column this bound is for)
    _, m, v, _ = ar.hashed_step_inputs(11, 1_700_000)
    worst = {}
    for t in (1, 2, 10 ** 6):
        u64 = tr.update_f64(m, v, t, LR)
        u32 = tr.update_f32(m, v, t, LR).astype(np.float64)
        assert np.isfinite(u64).all() and (u64 == 0).sum() > m.size // 8
        err = np.abs(u32 - u64)
        assert (err[u64 == 0] == 0).all()
        nz = u64 != 0
        assert np.abs(u64[nz]).min() > 2.0 ** -100  # (nothing near the subnormal range: the bound's absolute term idles)
        worst[t] = float((err[nz] / (U * np.abs(u64[nz]))).max())
    print("fp32 restatement of u, worst error in units of u |u_64|:", worst)
    for t, x in worst.items():
        assert x <= 4.2, (t, x)
        assert x > 1.0, (t, x)  # (the inputs do exercise the roundings)


# ------------------------------------------------------------------ CPU: the trainer's key on the stand-in
TAGS = [f"tensor_stats/{n}/{s}".encode() for n in list(ar.NAMES) + ["total"] for s in ("grad_norm", "param_norm",
                                                                                          "update_ratio")]
TAGS.append(b"tensor_stats/nonfinite")


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _run_trainer(binary, d, extra, rollouts=3):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def tstats_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_tstats_stub"])
    return os.path.join(ROOT, "trainer", "train_tstats_stub")


def test_trainer_key_with_the_stub_library(tstats_trainer, tmp_path):
    blobs = {}
    for name, extra in (("absent", ""), ("false", "log_tensor_stats: false\n"), ("true", "log_tensor_stats: true\n")):
        (tmp_path / name).mkdir()
        r = _run_trainer(tstats_trainer, tmp_path / name, extra)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
    tags = {k: _scalar_bits(b) for k, b in blobs.items()}
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    assert not set(TAGS) & set(tags["absent"]) and len(TAGS) == 40
    assert set(tags["true"]) == set(tags["absent"]) | set(TAGS)  # nothing else appears or goes
    for tag in TAGS:
        assert len(tags["true"][tag]) == 3 == len(tags["true"][b"mean_loss"]), tag  # once per trained rollout
    assert b"log_tensor_stats" in blobs["true"]  # the hparams flag of the config dump, only when set
    assert b"log_tensor_stats" not in blobs["absent"] and b"log_tensor_stats" not in blobs["false"]
    for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
        assert tags["absent"][tag] == tags["true"][tag], tag
    # the stand-in's made-up gradient norm of row k is 1 / (k + 1); its parameters are real and move by lr / 2 per update
    f = lambda bits: struct.unpack("<f", struct.pack("<I", bits))[0]
    assert f(tags["true"][b"tensor_stats/conv2.w/grad_norm"][0]) == np.float32(1 / 3)
    pn = [f(b) for b in tags["true"][b"tensor_stats/total/param_norm"]]
    assert all(x > 0 for x in pn) and len(set(pn)) == 3
    assert [f(b) for b in tags["true"][b"tensor_stats/nonfinite"]] == [0.0, 0.0, 0.0]


def test_library_without_the_symbol_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without aleppo_tensor_stats)
    r = _run_trainer(plain, tmp_path, "log_tensor_stats: true\n")
    assert r.returncode == 1 and "aleppo_tensor_stats is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "").returncode == 0


# ------------------------------------------------------------------ GPU
def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


@functools.lru_cache(maxsize=None)
def _obs(seed, n):
    a = hf.hf_bytes(seed, (n, 4, 84, 84))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _batch(seed, n, A):
    """a hashed batch as in test_optimizer_step: (obs, actions, old log-probs, advantages, returns, masks)"""
    import oracle_lib as orc
    return (_obs(seed + 1, n), (hf.hf_u32(seed + 2, n) % np.uint32(A)).astype(np.int64),
            orc.log_softmax(hf.hf_range(seed + 3, (n, A), -1, 1)), hf.hf_range(seed + 4, (n,), -1, 1),
            hf.hf_range(seed + 5, (n,), -1, 1), (hf.hf_unit(seed + 6, n) >= np.float32(0.1)).astype(np.uint8))


def _call(pkg, eng, sections, count=130, null=False):
    """the C entry point itself: (status, float64 [13, 10] pre-filled with -7 so that "nothing is written" shows)"""
    out = np.full((13, 10), -7.0, np.float64)
    rc = pkg.lib().aleppo_tensor_stats(eng._ctx, C.c_int(sections), None if null else out.ctypes.data_as(C.c_void_p),
                                       C.c_size_t(count))
    return rc, out


def _read(pkg, eng, sections):
    rc, out = _call(pkg, eng, sections)
    assert rc == pkg.OK, (rc, sections)
    return out


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_all(pkg, eng, H, A, t, lr, title):
    """all three section sets against the reference built from the three exports; prints the worst ratios to bound"""
    sd = eng.state_dict()
    assert int(sd["step"]) == t
    g = eng.export_grads()
    ref, rtol, atol = tr.reference(H, A, sd["params"], g, sd["exp_avg"], sd["exp_avg_sq"], t, lr)
    both = _read(pkg, eng, 3)
    print(title, "worst |device - reference| / bound:", {k: "%.3g" % x for k, x in tr.worst(both, ref, rtol, atol).items()})
    assert not tr.check(both, ref, rtol, atol, 3), tr.check(both, ref, rtol, atol, 3)[:6]
    assert not tr.check_ratio(both), tr.check_ratio(both)[:6]
    assert np.array_equal(_bits64(both), _bits64(_read(pkg, eng, 3)))  # two reads: the same bits
    for sections in (1, 2):
        one = _read(pkg, eng, sections)
        assert not tr.check(one, ref, rtol, atol, sections), (sections, tr.check(one, ref, rtol, atol, sections)[:6])
        cols = slice(1, 4) if sections == 1 else slice(4, 10)  # what a section reports does not depend on the other
        assert np.array_equal(_bits64(one[:, cols]), _bits64(both[:, cols])), sections
    return both, sd, g


def _norm_cross_check(both, metrics, max_norm):
    """row 12's GRAD_NORM against coef * the reported pre-clip norm of the last minibatch: (37 / 2 + 2) u relative - the
    bound of test_optimizer_step.test_reported_norm for the reported norm plus one rounding for the product with coef"""
    norm = metrics["grad_norm"].ravel()[-1]
    coef = ar.clip_coef(max_norm, norm)
    want = float(coef) * float(norm)
    err = abs(both[12, tr.GRAD_NORM] / want - 1)
    rtol = (37 / 2 + 2) * U
    print(f"  total grad norm {both[12, tr.GRAD_NORM]:.10g} vs coef * reported {want:.10g}: rel {err:.3g}/{rtol:.3g}")
    assert err <= rtol
    return coef


def _consistency(both, p0, p1, H, A):
    """one step between two exports: p0 - p in float64 equals u to within p's own rounding, 2u |p| per element, so per row
    | ||p0 - p|| - UPDATE_NORM | <= 2u ||p|| + 10u UPDATE_NORM"""
    offs = ar.param_offsets(H, A)
    d = p0.astype(np.float64) - p1.astype(np.float64)
    worst = 0.0
    for k in range(13):
        sl = slice(int(offs[k]), int(offs[k + 1])) if k < 12 else slice(None)
        moved, pn = np.linalg.norm(d[sl]), np.linalg.norm(p1[sl].astype(np.float64))
        bound = 2 * U * pn + 10 * U * both[k, tr.UPDATE_NORM]
        worst = max(worst, abs(moved - both[k, tr.UPDATE_NORM]) / bound)
        assert abs(moved - both[k, tr.UPDATE_NORM]) <= bound, (tr.NAMES[k], moved, both[k, tr.UPDATE_NORM], bound)
    print(f"  ||p0 - p|| against UPDATE_NORM, worst ratio to bound {worst:.3g}")


# A % 4 = 1, 3, 0, 2: the 16-byte group of the stacked head bias that straddles action.b and value.b; H % 64 = 32: pads
# after every head and fc tensor; A = 18: the 256-thread head; (512, 6) bf16: the flagship shape, 392 chunks of fc.w
SHAPES = [(32, 1, 256), (32, 3, 256), (32, 4, 256), (96, 18, 520)]
MATRIX = [(prec, H, A, n) for prec in ("fp32", "bf16") for H, A, n in SHAPES] + [("bf16", 512, 6, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,H,A,n", MATRIX)
def test_sections_against_the_reference(pkg, prec, H, A, n):
    """after load_params PARAMS is valid and STEP is ALEPPO_ERR_RUNTIME; after train(lr, 1, 2) (steps 1-2) and a further
    train(lr, 2, 2) (steps 3-6) both sections against the reference built from the three exports, with the reported-norm
    cross-check; then ONE step between two exports (train(lr, 1, 1), step 7) for the p0 - p consistency check - a call of
    several steps leaves no export in front of its last step"""
    eng = pkg.Engine(n // 8, 8, A, H, precision=_prec(pkg, prec))
    params = hf.fill_params(8200 + A, H, A)
    eng.load_params(params)
    ref, rtol, atol = tr.reference(H, A, params)
    got = _read(pkg, eng, 1)
    assert not tr.check(got, ref, rtol, atol, 1), tr.check(got, ref, rtol, atol, 1)[:6]
    assert got[12, tr.SIZE] == eng.param_count
    for sections in (2, 3):
        rc, out = _call(pkg, eng, sections)
        assert rc == pkg.ERR_RUNTIME and (out == -7).all(), (rc, sections)
    eng.set_batch(*_batch(8210, n, A))
    m = eng.train(LR, 1, 2)
    both, _, _ = _check_all(pkg, eng, H, A, 2, LR, f"tensor stats {prec} H={H} A={A} t=2")
    _norm_cross_check(both, m, 0.5)
    assert both[12, tr.GRAD_NORM] > 0 and both[12, tr.UPDATE_NORM] > 0 and not both[:, tr.STEP_NONFINITE].any()
    eng.set_batch(*_batch(8220, n, A))
    m = eng.train(LR, 2, 2)
    both, sd, _ = _check_all(pkg, eng, H, A, 6, LR, f"tensor stats {prec} H={H} A={A} t=6")
    _norm_cross_check(both, m, 0.5)
    eng.train(LR / 2, 1, 1)
    both, sd1, _ = _check_all(pkg, eng, H, A, 7, LR / 2, f"tensor stats {prec} H={H} A={A} t=7")
    _consistency(both, sd["params"], sd1["params"], H, A)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec,H,A", [("fp32", 32, 3), ("bf16", 96, 18)])
def test_update_columns_at_large_t_from_imported_moments(pkg, prec, H, A):
    """adam_ref.hashed_moments (|m| in 1e-12 .. 1, v in 1e-24 .. 1, a fifth zero) imported at step 10^6 - 1: the import
    makes STEP ALEPPO_ERR_RUNTIME, one train brings it back, and the update columns hold at t = 10^6; it is one step from
    exported state, so the p0 - p consistency check runs here too"""
    n = 256
    eng = pkg.Engine(n // 8, 8, A, H, precision=_prec(pkg, prec))
    params = hf.fill_params(8300, H, A)
    eng.load_params(params)
    eng.set_batch(*_batch(8310, n, A))
    eng.train(LR, 1, 1)
    assert _call(pkg, eng, 2)[0] == pkg.OK
    m0, v0 = ar.hashed_moments(8320, params.size)
    eng.load_state_dict(dict(params=params, exp_avg=m0, exp_avg_sq=v0, step=10 ** 6 - 1))
    assert _call(pkg, eng, 2)[0] == pkg.ERR_RUNTIME and _call(pkg, eng, 1)[0] == pkg.OK
    eng.train(LR, 1, 1)
    both, sd, _ = _check_all(pkg, eng, H, A, 10 ** 6, LR, f"tensor stats {prec} H={H} A={A} t=1e6")
    _consistency(both, params, sd["params"], H, A)
    eng.close()


@pytest.mark.gpu
def test_grad_columns_under_a_clip_factor_below_one(pkg):
    """a gradient-norm limit of 1e-3: coef < 1, and GRAD_MAXABS of every row is the maximum of aleppo_export_grads' elements
    bit for bit (the kernel multiplies the raw gradient with the very coef the export uses)"""
    H, A, n = 96, 18, 256
    eng = pkg.Engine(n // 8, 8, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(8400, H, A))
    eng.set_hyper(max_grad_norm=1e-3)
    eng.set_batch(*_batch(8410, n, A))
    m = eng.train(LR, 1, 2)
    both, _, g = _check_all(pkg, eng, H, A, 2, LR, "tensor stats, limit 1e-3")
    coef = _norm_cross_check(both, m, 1e-3)
    assert coef < 1e-2
    offs = ar.param_offsets(H, A)
    for k in range(12):
        want = np.float64(np.abs(g[offs[k]:offs[k + 1]]).max())
        assert _bits64(both[k, tr.GRAD_MAXABS]) == _bits64(want), tr.NAMES[k]
    assert _bits64(both[12, tr.GRAD_MAXABS]) == _bits64(np.float64(np.abs(g).max()))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,A", [(32, 1), (32, 3), (32, 4), (96, 18)])
def test_nonfinite_parameters_are_attributed_to_their_tensor(pkg, H, A):
    """a NaN in action.b's last element, an Inf in value.b and a NaN in the last element of fc.w, loaded and read without a
    forward pass: the counts land in rows 9, 11 and 6 and nowhere else, row 12 says 3, and every norm and maximum is the
    reference's over the finite elements (the straddling bias group and the element in front of a pad)"""
    offs = ar.param_offsets(H, A)
    params = hf.fill_params(8500, H, A)
    params[offs[10] - 1] = np.nan   # action.b, last element
    params[offs[12] - 1] = np.inf   # value.b
    params[offs[7] - 1] = np.nan    # fc.w, last element
    eng = pkg.Engine(8, 8, A, H, precision=pkg.FP32)
    eng.load_params(params)
    got = _read(pkg, eng, 1)
    ref, rtol, atol = tr.reference(H, A, params)
    want = np.zeros(13)
    want[[9, 11, 6]] = 1
    want[12] = 3
    assert np.array_equal(ref[:, tr.PARAM_NONFINITE], want)
    assert np.array_equal(got[:, tr.PARAM_NONFINITE], want), got[:, tr.PARAM_NONFINITE]
    assert not tr.check(got, ref, rtol, atol, 1), tr.check(got, ref, rtol, atol, 1)[:6]
    assert np.isfinite(got).all() and got[11, tr.PARAM_NORM] == 0  # (value.b's only element is the Inf)
    assert _call(pkg, eng, 2)[0] == pkg.ERR_RUNTIME
    eng.close()


@pytest.mark.gpu
def test_import_of_a_nan_moment_invalidates_the_step_section(pkg):
    """the step group's rule: after one clean train, import_optimizer (here with a NaN moment) replaces what the step is
    recomputed from, so STEP is ALEPPO_ERR_RUNTIME and nothing is written; PARAMS stays valid"""
    H, A, n = 32, 3, 256
    eng = pkg.Engine(n // 8, 8, A, H, precision=pkg.FP32)
    eng.load_params(hf.fill_params(8600, H, A))
    eng.set_batch(*_batch(8610, n, A))
    eng.train(LR, 1, 1)
    assert _call(pkg, eng, 3)[0] == pkg.OK
    sd = eng.state_dict()
    sd["exp_avg"][5] = np.nan
    m, v = sd["exp_avg"], sd["exp_avg_sq"]
    eng._c(pkg.lib().aleppo_import_optimizer(eng._ctx, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                             C.c_int64(1), C.c_size_t(m.size)))
    for sections in (2, 3):
        rc, out = _call(pkg, eng, sections)
        assert rc == pkg.ERR_RUNTIME and (out == -7).all()
    assert _call(pkg, eng, 1)[0] == pkg.OK
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_reading_changes_nothing(pkg, prec):
    """twins on the same batches: X reads the statistics (every section set, twice) between its updates, Y never does.
    aleppo_state_digest, aleppo_export_grads and the next train's metrics and digest are bit-identical"""
    H, A, n = 96, 6, 256
    res = []
    for reads in (True, False):
        eng = pkg.Engine(n // 8, 8, A, H, precision=_prec(pkg, prec))
        eng.load_params(hf.fill_params(8700, H, A))
        out = []
        if reads:
            _read(pkg, eng, 1)
        for i in range(3):
            eng.set_batch(*_batch(8710 + i, n, A))
            m = eng.train(LR, 1, 2)
            if reads:
                for sections in (3, 1, 2, 3):
                    _read(pkg, eng, sections)
            out.append((m, eng.state_digest(), eng.export_grads()))
        res.append(out)
        eng.close()
    for (mx, dx, gx), (my, dy, gy) in zip(*res):
        assert dx == dy
        assert np.array_equal(gx.view(np.uint32), gy.view(np.uint32))
        for k in mx:
            assert np.array_equal(mx[k].view(np.uint32), my[k].view(np.uint32)), k


@pytest.mark.gpu
def test_a_read_between_replays_does_not_recapture(pkg):
    """ALEPPO_OPT_UPDATE_GRAPH: the first update runs eagerly, the second captures, later ones replay; with reads of every
    section set between them the replay count (aleppo_get_option) advances by exactly one per update - no re-capture -
    and the statistics hold against the reference after every replay"""
    H, A, n = 96, 6, 256
    eng = pkg.Engine(n // 8, 8, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(8800, H, A))
    eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    eng.set_batch(*_batch(8810, n, A))
    counts = []
    for i in range(5):
        eng.train(LR, 1, 2)
        _check_all(pkg, eng, H, A, 2 * (i + 1), LR, f"tensor stats, captured update {i}")
        counts.append(eng.get_option(pkg.OPT_UPDATE_GRAPH))
    eng.close()
    assert counts == [0, 1, 2, 3, 4], counts


@pytest.mark.gpu
def test_errors(pkg):
    """sections 0 and 4, a null out, count 129: ALEPPO_ERR_INVALID_ARGUMENT and nothing written; while a step is armed
    ALEPPO_ERR_RUNTIME, and after the release the read succeeds"""
    E, T, H, A = 8, 8, 32, 4
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    params = hf.fill_params(8900, H, A)
    eng.load_params(params)
    for sections, count, null in ((0, 130, False), (4, 130, False), (7, 130, False), (-1, 130, False), (1, 130, True),
                                  (1, 129, False), (3, 131, False)):
        rc, out = _call(pkg, eng, sections, count, null)
        assert rc == pkg.ERR_INVALID_ARGUMENT and (out == -7).all(), (sections, count, null, rc)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.tensor_stats(4)
    with pytest.raises(pkg.AleppoError, match="step section"):
        eng.tensor_stats("step")
    d = eng.tensor_stats("params")
    assert set(d) == set(pkg.TENSOR_NAMES) and set(d["fc.w"]) == set(pkg.TENSOR_STATS)
    assert d["total"]["size"] == eng.param_count and d["value.b"]["param_norm"] == abs(float(params[-1]))
    assert d["fc.w"]["grad_norm"] == 0.0 and eng.tensor_stats("params", raw=True).shape == (13, 10)
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(8905, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    rc, out = _call(pkg, eng, 1)
    assert rc == pkg.ERR_RUNTIME and (out == -7).all()
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    ref, rtol, atol = tr.reference(H, A, params)
    got = _read(pkg, eng, 1)
    assert not tr.check(got, ref, rtol, atol, 1)
    eng.synchronize()
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
