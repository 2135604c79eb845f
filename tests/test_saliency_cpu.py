"""aleppo_saliency without a device: the two integer tables through aleppo_saliency_tables (host only, no context)
against numpy's double, what it refuses, the header against the Python mirror, and the numpy restatement's own known
answers (tests/saliency_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hashfill as hf
import saliency_ref as sr
from conftest import ROOT
from __graft_entry__ import build

SETTINGS = [(5.0, 3.0, 5), (2.0, 1.0, 12), (10.0, 10.0, 7), (0.5, 0.5, 2), (16.0, 10.0, 84), (3.3, 2.7, 9)]


@pytest.fixture(scope="module")
def pkg():
    return build()


@pytest.mark.parametrize("sigma_mask,sigma_blur,stride", SETTINGS)
def test_tables_against_numpy(pkg, sigma_mask, sigma_blur, stride):
    g, w, R = pkg.saliency_tables(stride, sigma_mask, sigma_blur)
    rg, rw, rR = sr.tables(sigma_mask, sigma_blur)
    assert g.dtype == w.dtype == np.uint16 and g.shape == w.shape == (84,)
    assert R == rR == int(4 * sigma_blur + 0.5) and 2 <= R <= 40
    assert int(g[0]) == 4096 and int(w[0]) + 2 * int(w[1:].sum()) == 4096  # exactly
    assert not w[R + 1:].any() and (np.diff(g.astype(int)) <= 0).all() and (np.diff(w.astype(int)) <= 0).all()
    # libm and numpy may differ in the last bit of exp: one unit at a tie (the centre tap carries the taps' residue: 2R of them)
    assert np.abs(g.astype(int) - rg.astype(int)).max() <= 1
    assert np.abs(w[1:].astype(int) - rw[1:].astype(int)).max() <= 1
    assert abs(int(w[0]) - int(rw[0])) <= 2 * int(np.abs(w[1:].astype(int) - rw[1:].astype(int)).sum())


def test_default_tables_are_the_documented_ones(pkg):
    g, w, R = pkg.saliency_tables()
    assert (pkg.SALIENCY_STRIDE, pkg.SALIENCY_SIGMA_MASK, pkg.SALIENCY_SIGMA_BLUR, pkg.SALIENCY_PLANES) == (5, 5.0, 3.0, 15)
    assert R == 12 and pkg.saliency_grid() == 17 and pkg.saliency_grid(12) == 7 and pkg.saliency_grid(84) == 1
    g2, w2, R2 = np.zeros(84, np.uint16), np.zeros(84, np.uint16), C.c_int32()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert pkg.lib().aleppo_saliency_tables(None, ptr(g2), ptr(w2), C.byref(R2)) == pkg.OK  # NULL: the defaults
    assert np.array_equal(g, g2) and np.array_equal(w, w2) and R2.value == 12
    assert int(g[5]) == round(4096 * np.exp(-0.5)) and int(g[83]) == 0


@pytest.mark.parametrize("kw", [dict(stride=1), dict(stride=85), dict(stride=0), dict(stride=-5),
                                dict(sigma_mask=0.49), dict(sigma_mask=16.5), dict(sigma_mask=float("nan")),
                                dict(sigma_mask=float("inf")), dict(sigma_blur=0.4), dict(sigma_blur=10.01),
                                dict(sigma_blur=float("nan")), dict(sigma_blur=-3.0), dict(planes=0), dict(planes=16),
                                dict(planes=-1)])
def test_invalid_parameters_are_refused_and_nothing_is_written(pkg, kw):
    with pytest.raises(pkg.AleppoInvalidArgument, match="saliency"):
        pkg.saliency_tables(**kw)
    k = dict(sr.DEFAULTS, **kw)
    cfg = pkg.SaliencyConfig(k["stride"], k["planes"], k["sigma_mask"], k["sigma_blur"])
    g, w, R = np.full(84, 7, np.uint16), np.full(84, 7, np.uint16), C.c_int32(-7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert pkg.lib().aleppo_saliency_tables(C.byref(cfg), ptr(g), ptr(w), C.byref(R)) == pkg.ERR_INVALID_ARGUMENT
    assert (g == 7).all() and (w == 7).all() and R.value == -7


def test_null_outputs_and_a_null_context_are_refused(pkg):
    lib = pkg.lib()
    g, w, R = np.full(84, 7, np.uint16), np.full(84, 7, np.uint16), C.c_int32(-7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, ptr(w), C.byref(R)), (ptr(g), None, C.byref(R)), (ptr(g), ptr(w), None)):
        assert lib.aleppo_saliency_tables(None, *args) == pkg.ERR_INVALID_ARGUMENT
    assert (g == 7).all() and (w == 7).all() and R.value == -7
    obs = np.zeros((1, 4, 84, 84), np.uint8)
    pol, val = np.full((1, 17, 17), -7, np.float32), np.full((1, 17, 17), -7, np.float32)
    rc = lib.aleppo_saliency(None, ptr(obs), C.c_int64(0), C.c_int64(1), None, ptr(pol), ptr(val), None)
    assert rc == pkg.ERR_INVALID_ARGUMENT and (pol == -7).all() and (val == -7).all()
    out = np.full((1, 1, 4, 84, 84), 9, np.uint8)
    rc = lib.aleppo_saliency_perturbed(None, ptr(obs), C.c_int64(0), C.c_int64(1), None, C.c_int64(0), C.c_int64(1), ptr(out))
    assert rc == pkg.ERR_INVALID_ARGUMENT and (out == 9).all()


def test_header_against_the_python_mirror(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", hdr)
    assert ("typedef struct { int32_t stride; int32_t planes; double sigma_mask; double sigma_blur; } "
            "aleppo_saliency_config;") in flat
    assert [f[0] for f in pkg.SaliencyConfig._fields_] == ["stride", "planes", "sigma_mask", "sigma_blur"]
    assert C.sizeof(pkg.SaliencyConfig) == 24 and pkg.SaliencyConfig.sigma_mask.offset == 8
    assert pkg.SaliencyConfig.planes.offset == 4 and pkg.SaliencyConfig.sigma_blur.offset == 16
    assert ("int aleppo_saliency_tables(const aleppo_saliency_config *cfg, uint16_t mask_g[84], uint16_t blur_w[84], "
            "int32_t *radius);") in flat
    assert ("int aleppo_saliency(aleppo_ctx *ctx, const uint8_t *observations, int64_t first, int64_t n, "
            "const aleppo_saliency_config *cfg, float *policy, float *value, float *outputs);") in flat
    assert ("int aleppo_saliency_perturbed(aleppo_ctx *ctx, const uint8_t *observations, int64_t first, int64_t n, "
            "const aleppo_saliency_config *cfg, int64_t position_first, int64_t position_count, uint8_t *out);") in flat
    for name in ("aleppo_saliency_tables", "aleppo_saliency", "aleppo_saliency_perturbed"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    for name in ("saliency", "saliency_perturbed"):
        assert hasattr(pkg.Engine, name)
    for i, name in enumerate(("sal_blur", "sal_perturb", "sal_score")):
        m = re.search(rf"\bALEPPO_K_{name.upper()}\s*=\s*(\d+)", hdr)
        assert m and int(m.group(1)) == pkg.KERNEL_CLASSES[name] == 23 + i
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


@pytest.mark.parametrize("sigma_mask,sigma_blur,stride", [(5.0, 3.0, 5), (2.0, 1.0, 12), (10.0, 10.0, 7)])
def test_the_restatement_keeps_its_invariants(pkg, sigma_mask, sigma_blur, stride):
    """with the library's tables: a constant plane is unchanged at every point, no partial sum overflows 32 bits (blur asserts
    it), every point changes a half-saturated random stack in at least 133 bytes, and only in the planes named"""
    g, w, R = pkg.saliency_tables(stride, sigma_mask, sigma_blur)
    const = np.stack([np.full((84, 84), v, np.uint8) for v in (0, 77, 200, 255)])[None]
    assert np.array_equal(sr.blur(const, w, R), const)
    P = sr.grid(stride) ** 2
    out = sr.perturbed(const, g, w, R, stride)
    assert out.shape == (1, P, 4, 84, 84) and (out == const[:, None]).all()
    rnd = sr.half_saturated(hf.hf_bytes(8800, (1, 4, 84, 84)), hf.hf_unit(8801, 4 * 7056).reshape(1, 4, 84, 84))
    out = sr.perturbed(rnd, g, w, R, stride)
    changed = (out != rnd[:, None]).reshape(P, -1).sum(1)
    assert changed.min() >= 133, changed.min()
    one = sr.perturbed(rnd, g, w, R, stride, planes=4)
    assert np.array_equal(one[:, :, 2], out[:, :, 2]) and (one[:, :, [0, 1, 3]] == rnd[:, None][:, :, [0, 1, 3]]).all()


def test_the_restatement_known_answers():
    # one bright pixel in the corner, taps (2, 1) / 4 with R = 1 in 4096ths: the reflection doubles the corner's own weight
    w = np.zeros(84, np.uint16)
    w[:2] = (2048, 1024)
    I = np.zeros((84, 84), np.uint8)
    I[0, 0] = 255
    B = sr.blur(I, w, 1)
    # horizontally the corner sees itself twice (x = -1 reflects to 0): 3/4, its neighbour 1/4; likewise vertically
    assert [int(B[0, 0]), int(B[0, 1]), int(B[1, 0]), int(B[1, 1]), int(B[0, 2])] == [143, 48, 48, 16, 0]
    I2 = np.zeros((84, 84), np.uint8)
    I2[83, 83] = 255
    assert np.array_equal(sr.blur(I2, w, 1), B[::-1, ::-1])
    g = np.zeros(84, np.uint16)
    g[:2] = (4096, 2048)
    m = sr.mask(g, 12, 8)  # G = 7: point (1, 1), centre (12, 12)
    assert int(m[12, 12]) == 256 and int(m[12, 13]) == 128 and int(m[13, 13]) == 64 and int(m[12, 14]) == 0 and m.sum() == 256 + 4 * 128 + 4 * 64
    s_pol, s_val = sr.scores(np.array([[[1.0, 2.0, 3.0], [1.0, 4.0, 2.0], [1.0, 2.0, 3.0]]]))
    assert s_pol.tolist() == [[2.0, 0.0]] and s_val.tolist() == [[0.5, 0.0]]
    up = sr.upsample(np.arange(49).reshape(7, 7), 12)
    assert up.shape == (84, 84) and up[0, 0] == 0 and up[5, 6] == 1 and up[6, 5] == 7 and up[83, 83] == 48 and up[77, 78] == 48
    assert sr.uv_bytes([0.0, 0.5, 1.0], 1.0).tolist() == [128, 192, 255] and sr.uv_bytes([3.0], 0.0).tolist() == [128]
    assert sr.uv_bytes([3.0], float("nan")).tolist() == [128] and sr.uv_bytes([3.0], float("inf")).tolist() == [128]
