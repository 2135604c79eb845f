"""Gradient probes, the part that needs no GPU: the header against the Python mirror, the host reference of
aleppo_grad_gram (grad_probe_ref.py) with its derived bound - a plain float64 dot stays inside it, three planted faults do
not - and the three host helpers of the wrapper on synthetic Grams."""
import ctypes as C
import math

import numpy as np
import pytest

import grad_probe_ref as gp
import hashfill as hf
from trainer_helpers import header_const as const
from __graft_entry__ import load_package

H, A = 32, 5


def _vectors(seed, k, H=H, A=A, scale=1.0):
    n = sum(gp.sizes(H, A))
    return [hf.hf_range(seed + i, (n,), -scale, scale * (1 + 0.5 * i)) for i in range(k)]


def test_header_constants_match_the_python_mirror():
    pkg = load_package()
    assert const("ALEPPO_GRAD_SLOTS", stripped=True) == pkg.GRAD_SLOTS == 4
    assert const("ALEPPO_GRAD_SRC_EXP_AVG", stripped=True) == pkg.GRAD_SRC_EXP_AVG == 0
    assert const("ALEPPO_GRAD_SRC_PARAM_DELTA", stripped=True) == pkg.GRAD_SRC_PARAM_DELTA == 1
    assert const("ALEPPO_ABI_VERSION", stripped=True) == pkg.ABI_VERSION == 2  # (not bumped: only additions)
    assert C.sizeof(pkg.GradProbeConfig) == 16 and pkg.GradProbeConfig.reserved.offset == 12
    for name in ("aleppo_grad_probe", "aleppo_grad_take", "aleppo_grad_export", "aleppo_grad_import", "aleppo_grad_gram"):
        assert name in pkg.EXPORTS
    assert pkg.GRAM_NAMES == gp.NAMES + ("all",) and len(pkg.GRAM_NAMES) == pkg.TENSOR_STATS_ROWS
    for m in ("grad_probe", "grad_take", "grad_vector", "load_grad", "grad_gram", "grad_cosines", "gradient_noise_scale",
              "gradient_interference"):
        assert hasattr(pkg.Engine, m), m


def test_reference_cuts_the_tensors_and_sums_exactly():
    x = _vectors(100, 2)
    g, nf = gp.gram(x, H, A)
    assert g.shape == (13, 2, 2) and not nf.any()
    spans = gp.bounds(H, A)
    assert spans[0] == (0, 8192) and spans[-1][1] == x[0].size and spans[8][1] - spans[8][0] == A * H
    b, e = spans[9]  # action.b: few enough elements to add exactly by hand
    from fractions import Fraction
    want = sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(x[0][b:e], x[1][b:e]))
    assert g[9, 0, 1] == float(want) == g[9, 1, 0]
    # row 12 is the whole model, and a one-element tensor is one exact product with the bound 0
    assert g[12, 0, 0] == math.fsum(x[0].astype(np.float64) ** 2)
    assert g[11, 0, 1] == float(x[0][-1]) * float(x[1][-1]) and gp.bound(x, H, A)[11, 0, 1] == 0.0


def _numpy_gram(x, H, A):
    d = np.stack(x).astype(np.float64)
    spans = gp.bounds(H, A) + [(0, d.shape[1])]
    return np.stack([d[:, b:e] @ d[:, b:e].T for b, e in spans])


@pytest.mark.parametrize("H,A", [(32, 1), (32, 5), (96, 18)])
def test_a_float64_dot_stays_inside_the_bound(H, A):
    x = _vectors(200 + H + A, 3, H, A)
    worst = gp.check(_numpy_gram(x, H, A), np.zeros(13, np.int64), x, H, A)
    print(f"H={H} A={A}: numpy float64 dot, largest |error| / bound = {worst:.3g}")
    assert worst < 1.0


def test_planted_faults_fail_the_bound():
    x = _vectors(300, 2)
    good, nf = gp.gram(x, H, A)
    gp.check(good, nf, x, H, A)
    spans = gp.bounds(H, A) + [(0, x[0].size)]
    # 1. the products formed in fp32
    d32 = np.stack(x)
    fp32 = np.stack([[[math.fsum((d32[i, b:e] * d32[j, b:e]).astype(np.float64)) for j in range(2)] for i in range(2)]
                     for b, e in spans])
    with pytest.raises(AssertionError):
        gp.check(fp32, nf, x, H, A)
    # 2. the value row of the stacked head weights attributed to action.w
    moved = good.copy()
    moved[8] += good[10]
    moved[10] = 0.0
    with pytest.raises(AssertionError):
        gp.check(moved, nf, x, H, A)
    # 3. an element next to a non-finite one dropped as well (its whole 16-byte group, say)
    y = [v.copy() for v in x]
    at = spans[2][0] + 1001
    y[1][at] = np.nan
    want, want_nf = gp.gram(y, H, A)
    assert want_nf[2] == 1 and want_nf[12] == 1 and want_nf.sum() == 2
    gp.check(want, want_nf, y, H, A)
    z = [v.copy() for v in y]
    for v in z:
        v[at + 1] = 0.0  # the neighbour's products vanish from every entry
    dropped, _ = gp.gram(z, H, A)
    with pytest.raises(AssertionError):
        gp.check(dropped, want_nf, y, H, A)
    # ... and a count in the wrong row is caught too
    with pytest.raises(AssertionError):
        gp.check(want, np.roll(want_nf[:12], 1).tolist() + [1], y, H, A)


# ------------------------------------------------------------------ the wrapper's host helpers
def test_cosines_are_nan_where_a_norm_is_zero():
    pkg = load_package()
    x = _vectors(400, 3)
    x[2][:] = 0.0  # an all-zero vector: every cosine with it is NaN
    b, e = gp.bounds(H, A)[3]
    x[0][b:e] = 0.0  # and one tensor of another
    g, _ = gp.gram(x, H, A)
    cos = pkg.Engine.grad_cosines(g)
    assert cos.shape == g.shape
    assert np.isnan(cos[:, 2, :]).all() and np.isnan(cos[:, :, 2]).all()
    assert np.isnan(cos[3, 0, 1]) and np.isnan(cos[3, 0, 0]) and cos[3, 1, 1] == 1.0
    d = np.stack(x).astype(np.float64)
    want = d[0] @ d[1] / math.sqrt((d[0] @ d[0]) * (d[1] @ d[1]))
    np.testing.assert_allclose(cos[12, 0, 1], want, rtol=1e-12)
    assert cos[12, 0, 1] == cos[12, 1, 0] and abs(cos[12, 0, 0] - 1.0) < 1e-15
    # the dict form of grad_gram goes in and comes out
    as_dict = {t: g[r] for r, t in enumerate(pkg.GRAM_NAMES)}
    as_dict["nonfinite"] = {t: 0 for t in pkg.GRAM_NAMES}
    cd = pkg.Engine.grad_cosines(as_dict)
    assert set(cd) == set(pkg.GRAM_NAMES)
    np.testing.assert_array_equal(cd["all"], cos[12])


def test_noise_scale_recovers_a_known_pair():
    """E |g_b|^2 = |G|^2 + S / b for g_b = G + noise / sqrt(b) (McCandlish et al. 2018, eq. A.1): from the two exact
    expectations the estimators return |G|^2 and S themselves"""
    pkg = load_package()
    rows = 13
    G2 = np.linspace(0.5, 3.0, rows)
    S = np.linspace(40.0, 900.0, rows)
    b_small, b_big = 61, 987
    g = np.zeros((rows, 2, 2))
    g[:, 0, 0] = G2 + S / b_small
    g[:, 1, 1] = G2 + S / b_big
    g[:, 0, 1] = g[:, 1, 0] = G2  # (not read)
    out = pkg.Engine.noise_scale_from_gram(g, b_small, b_big)
    np.testing.assert_allclose(out["g2"], G2, rtol=1e-12)
    np.testing.assert_allclose(out["s"], S, rtol=1e-12)
    np.testing.assert_allclose(out["b_simple"], S / G2, rtol=1e-12)
    as_dict = {t: g[r] for r, t in enumerate(pkg.GRAM_NAMES)}
    d = pkg.Engine.noise_scale_from_gram(as_dict, b_small, b_big)
    assert d["b_simple"]["all"] == out["b_simple"][12] and d["g2"]["fc.w"] == out["g2"][6]
    for bad in ((0, 5), (5, 5), (9, 4)):
        with pytest.raises(pkg.AleppoInvalidArgument):
            pkg.Engine.noise_scale_from_gram(g, *bad)


def test_interference_equals_the_bilinear_expansion():
    pkg = load_package()
    x = _vectors(500, 3)
    g, _ = gp.gram(x, H, A)
    d = np.stack(x).astype(np.float64)
    out = pkg.Engine.interference_from_gram(g)
    spans = gp.bounds(H, A) + [(0, d.shape[1])]
    pairs = dict(policy_value=(0, 1), policy_entropy=(0, 2), value_entropy=(1, 2))
    for r, (b, e) in enumerate(spans):
        for name, (i, j) in pairs.items():
            want = d[i, b:e] @ d[j, b:e] / math.sqrt((d[i, b:e] @ d[i, b:e]) * (d[j, b:e] @ d[j, b:e]))
            np.testing.assert_allclose(out["cosines"][name][r], want, rtol=1e-10, atol=1e-14)
        for i, term in enumerate(("policy", "value", "entropy")):
            np.testing.assert_allclose(out["norms"][term][r], np.linalg.norm(d[i, b:e]), rtol=1e-12)
    # the inner product of two combinations from the Gram alone: g(1, c_v, c_e) = g_pi + c_v g_v + c_e g_e against g_v,
    # and its squared norm
    c = np.array([1.0, 0.25, 0.03])
    full = c @ d
    combine = lambda a, b: np.einsum("i,rij,j->r", np.asarray(a, np.float64), g, np.asarray(b, np.float64))  # a^T G b
    got = combine(c, [0.0, 1.0, 0.0])
    np.testing.assert_allclose(got[12], full @ d[1], rtol=1e-10)
    np.testing.assert_allclose(combine(c, c)[12], full @ full, rtol=1e-10)
    b, e = spans[6]
    np.testing.assert_allclose(got[6], full[b:e] @ d[1, b:e], rtol=1e-10)
