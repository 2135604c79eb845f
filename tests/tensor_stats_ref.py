"""aleppo_tensor_stats, restated: the float64 reference built from what the C ABI exports, and the bounds a device answer
has to meet.  A plain helper module (no fixtures), shared by the CPU and GPU tests of tests/test_tensor_stats.py.

The reference works on the EXPORTED flat vectors (libtorch parameters() order): the parameters, aleppo_export_grads' g,
both moments and the step count; rows are the twelve tensors of adam_ref.NAMES and then the whole model.
    p, g      the exported fp32 elements
    u         = s (m / (sqrt(v) / c + eps)) in float64 on the fp32 m, v, s, c, eps, (s, c) = adam_ref.step_scalars(t, lr)
A non-finite p is counted (PARAM_NONFINITE) and left out of columns 1-2; an element whose g, m, v or u is non-finite is
counted once (STEP_NONFINITE) and left out of columns 4-8.

Bounds, derived, u = 2^-24, n = the row's size:
    sums of squares   the device adds exact double squares in some order; against math.fsum of the same squares the relative
                      error is at most n 2^-53 for any order of non-negative terms; the norm gets half of that plus 2^-53
                      (one correctly rounded root)
    SIZE, PARAM_MAXABS, GRAD_MAXABS, both counts: equal bits
    u per element     10u |u_64| + 2^-126: five roundings (root, quotient by c, sum with eps, quotient, product with s),
                      doubled by adam_ref's convention (room for a division or root that is not correctly rounded); the
                      absolute term covers results in the subnormal range
    UPDATE_MAXABS     relative 10u, plus 2^-126
    UPDATE_NORM       relative 10u plus the norm's summation term, plus sqrt(n) 2^-126
    UPDATE_RATIO      the quotient of the two REPORTED norms recomputed in double: equal bits (check_ratio)
"""
import math

import numpy as np

import adam_ref as ar

U = ar.U
ROWS, COLS = 13, 10
NAMES = list(ar.NAMES) + ["total"]
STATS = ("size", "param_norm", "param_maxabs", "param_nonfinite", "grad_norm", "grad_maxabs", "update_norm",
         "update_maxabs", "update_ratio", "step_nonfinite")
SIZE, PARAM_NORM, PARAM_MAXABS, PARAM_NONFINITE, GRAD_NORM, GRAD_MAXABS, UPDATE_NORM, UPDATE_MAXABS, UPDATE_RATIO, \
    STEP_NONFINITE = range(10)
SEC_PARAMS, SEC_STEP = 1, 2
TINY = 2.0 ** -126


def update_f64(m, v, t, lr):
    """u in float64 on fp32 moments and the float32 schedule scalars of step t"""
    s, c = ar.step_scalars(t, lr)
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return float(s) * (m / (np.sqrt(v) / float(c) + float(ar.EPS)))


def update_f32(m, v, t, lr):
    """kernels.hip adam_element's update expression in numpy float32, operation for operation"""
    s, c = ar.step_scalars(t, lr)
    m, v = np.asarray(m, np.float32), np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = s * (m / (np.sqrt(v) / c + ar.EPS))
    assert u.dtype == np.float32
    return u


def _sumsq(x):
    """math.fsum of the exact double squares of fp32 values"""
    x = np.asarray(x, np.float64)
    return math.fsum((x * x).tolist())


def _maxabs(x):
    return float(np.max(np.abs(x))) if x.size else 0.0


def reference(H, A, params, grads=None, exp_avg=None, exp_avg_sq=None, t=None, lr=None):
    """(ref, rtol, atol): float64 [13, 10] each.  Without the step inputs columns 4-9 are 0 (ALEPPO_TS_SEC_PARAMS alone).
    rtol / atol are the bounds of the module docstring per entry (0 / 0: equal bits; UPDATE_RATIO is left to check_ratio and
    holds the quotient of the reference's own norms for information)."""
    offs = ar.param_offsets(H, A)
    step = grads is not None
    ref, rtol, atol = (np.zeros((ROWS, COLS), np.float64) for _ in range(3))
    p = np.asarray(params, np.float32)
    assert p.size == offs[-1]
    if step:
        g, m, v = (np.asarray(a, np.float32) for a in (grads, exp_avg, exp_avg_sq))
        u = update_f64(m, v, t, lr)
        ok_s = np.isfinite(g) & np.isfinite(m) & np.isfinite(v) & np.isfinite(u)
    ok_p = np.isfinite(p)
    sq = np.zeros((12, 3))
    for k in range(12):
        sl = slice(int(offs[k]), int(offs[k + 1]))
        n = sl.stop - sl.start
        ref[k, SIZE] = n
        pk = p[sl][ok_p[sl]]
        sq[k, 0] = _sumsq(pk)
        ref[k, PARAM_MAXABS] = _maxabs(pk)
        ref[k, PARAM_NONFINITE] = n - pk.size
        if step:
            gk, uk = g[sl][ok_s[sl]], u[sl][ok_s[sl]]
            sq[k, 1], sq[k, 2] = _sumsq(gk), math.fsum((uk * uk).tolist())
            ref[k, GRAD_MAXABS], ref[k, UPDATE_MAXABS] = _maxabs(gk), _maxabs(uk)
            ref[k, STEP_NONFINITE] = n - gk.size
    ref[12, SIZE] = ref[:12, SIZE].sum()
    ref[12, PARAM_NONFINITE], ref[12, STEP_NONFINITE] = ref[:12, PARAM_NONFINITE].sum(), ref[:12, STEP_NONFINITE].sum()
    for col in (PARAM_MAXABS, GRAD_MAXABS, UPDATE_MAXABS):
        ref[12, col] = ref[:12, col].max()
    tot = [math.fsum(sq[:, j].tolist()) for j in range(3)]
    for k in range(13):
        s = sq[k] if k < 12 else tot
        n = ref[k, SIZE]
        summ = n * 2.0 ** -53 / 2 + 2.0 ** -53
        ref[k, PARAM_NORM] = math.sqrt(s[0])
        rtol[k, PARAM_NORM] = summ
        if step:
            ref[k, GRAD_NORM], ref[k, UPDATE_NORM] = math.sqrt(s[1]), math.sqrt(s[2])
            rtol[k, GRAD_NORM] = summ
            rtol[k, UPDATE_NORM], atol[k, UPDATE_NORM] = 10 * U + summ, math.sqrt(n) * TINY
            rtol[k, UPDATE_MAXABS], atol[k, UPDATE_MAXABS] = 10 * U, TINY
            with np.errstate(invalid="ignore", divide="ignore"):
                ref[k, UPDATE_RATIO] = np.float64(ref[k, UPDATE_NORM]) / np.float64(ref[k, PARAM_NORM])
    return ref, rtol, atol


def check(dev, ref, rtol, atol, sections):
    """failures of a device answer [13, 10] against reference(): list of (tensor, stat, device, reference, bound).  The
    columns of a section that was not requested must be 0; SIZE is always checked; UPDATE_RATIO: check_ratio."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == (ROWS, COLS)
    want = ref.copy()
    if not sections & SEC_PARAMS:
        want[:, PARAM_NORM:PARAM_NONFINITE + 1] = 0
    if not sections & SEC_STEP:
        want[:, GRAD_NORM:] = 0
    bad = []
    for k in range(ROWS):
        for col in range(COLS):
            if col == UPDATE_RATIO and sections & SEC_STEP:
                continue
            d, w = dev[k, col], want[k, col]
            bound = rtol[k, col] * abs(w) + atol[k, col] if w != 0 or atol[k, col] else 0.0
            if not abs(d - w) <= bound:
                bad.append((NAMES[k], STATS[col], float(d), float(w), float(bound)))
    return bad


def check_ratio(dev):
    """UPDATE_RATIO of a read of BOTH sections: the IEEE double quotient of the two reported norms, bit for bit (0 / 0 = NaN)"""
    dev = np.asarray(dev, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = dev[:, UPDATE_NORM] / dev[:, PARAM_NORM]
    return [(NAMES[k], float(dev[k, UPDATE_RATIO]), float(want[k])) for k in range(ROWS)
            if dev[k, UPDATE_RATIO].tobytes() != want[k].tobytes()]


def worst(dev, ref, rtol, atol):
    """{stat: largest |device - reference| / bound over the rows} for the bounded columns (printed by the tests)"""
    out = {}
    for col in (PARAM_NORM, GRAD_NORM, UPDATE_NORM, UPDATE_MAXABS):
        b = rtol[:, col] * np.abs(ref[:, col]) + atol[:, col]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(b > 0, np.abs(dev[:, col] - ref[:, col]) / b, 0.0)
        out[STATS[col]] = float(np.max(r))
    return out
