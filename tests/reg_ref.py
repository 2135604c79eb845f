"""The regularised optimizer step (ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF) and aleppo_shrink_perturb, restated.

A plain helper module (no fixtures).  It extends adam_ref's float64 step with the decoupled terms of include/aleppo.h.
With wd and la the two options' float32 values, f_wd = float32(lr * wd), f_an = float32(lr * la) (the products in double,
rounded once, as api_train.hip uploads them), p0 the parameter before the step and a the anchor's element:
    q = adam_ref's p                        (moments, clip factor and step size untouched)
    t1 = f_wd p0        t2 = f_an (p0 - a)
    p = q - (t1 + t2)
Without an anchor (la = 0) a reads as +0.

Bound, u = 2^-24, by adam_ref's rule - TWICE the plain count of fp32 roundings.  The plain count on top of q's own:
t1 one product (u |t1|); p0 - a and the product (2u |t2|); the sum r = t1 + t2 (u |r| <= u (|t1| + |t2|)); p = q - r
(u |p|); q's final rounding, which adam_ref charges to its result, is now an intermediate (u |q|):
    tol_p = 2u |p| + 2u |q| + (s / d) (tol_m + 16u |m|) + 4u |t1| + 6u |t2|
The moments keep adam_ref's bounds.  Where the bound is exactly 0 the device value must equal the reference exactly.

aleppo_shrink_perturb: p' = fl(fl(lam p) + fl(sg xi)) in float32, lam = float32(shrink), sg = float32(sigma), xi the draw of
aleppo_recycle_units (recycle_ref.reinit_values) at the element's index in the flat exported vector with
a_l = float32(sqrt(6 / fan_in)), fan_in = 256, 512, 576, 3136 for the trunk weights and H for the action and value weight
rows; xi = 0 for the six biases."""
import numpy as np

import adam_ref as ar
import hashfill as hf
import recycle_ref as rr

U = ar.U
QUANTITIES = ar.QUANTITIES


def f32_option(x):
    """the float32 an option holds after Engine.set_regularization(x)"""
    return np.float32(x)


def factors(lr, wd, la):
    """(f_wd, f_an) as float32: the two slots of the device hyper block of one aleppo_train(lr, ...) call"""
    return np.float32(float(lr) * float(f32_option(wd))), np.float32(float(lr) * float(f32_option(la)))


def _anchor(anchor, like):
    return np.zeros_like(np.asarray(like, np.float64)) if anchor is None else np.asarray(anchor, np.float64)


def reference_step(p0, m0, v0, g, t, lr, wd=0.0, la=0.0, anchor=None):
    """step t in float64 and its bounds: dict of p, q, m, v, t1, t2 and tol_p, tol_m, tol_v (float64 arrays)"""
    ref = ar.reference_step(p0, m0, v0, g, t, lr)
    f_wd, f_an = factors(lr, wd, la)
    p0 = np.asarray(p0, np.float64)
    q = ref["p"]
    t1 = float(f_wd) * p0
    t2 = float(f_an) * (p0 - _anchor(anchor, p0))
    p = q - (t1 + t2)
    # (ref["tol_p"] is 2u |q| + (s / d) (tol_m + 16u |m|))
    tol_p = ref["tol_p"] + 2 * U * np.abs(p) + 4 * U * np.abs(t1) + 6 * U * np.abs(t2)
    return dict(p=p, q=q, m=ref["m"], v=ref["v"], t1=t1, t2=t2, tol_p=tol_p, tol_m=ref["tol_m"], tol_v=ref["tol_v"])


def reg_element_f32(p0, m0, v0, g, t, lr, wd=0.0, la=0.0, anchor=None):
    """kernels.hip adam_element then reg_element in numpy float32, operation for operation (no fused multiply-add):
    (p, m, v)"""
    q, m, v = ar.adam_element_f32(p0, m0, v0, g, t, lr)
    f_wd, f_an = factors(lr, wd, la)
    p0 = np.asarray(p0, np.float32)
    a = np.zeros_like(p0) if anchor is None else np.asarray(anchor, np.float32)
    r = f_wd * p0 + f_an * (p0 - a)
    p = q - r
    assert p.dtype == r.dtype == np.float32
    return p, m, v


def ratios(before, after, g, t, lr, wd=0.0, la=0.0, anchor=None):
    """per element |device - reference| / bound for m, v, p (float64 arrays), as adam_ref.ratios: a zero bound with an equal
    value gives 0, with any difference inf"""
    p0, m0, v0 = before
    ref = reference_step(p0, m0, v0, g, t, lr, wd, la, anchor)
    out = {}
    for q, got in zip(("p", "m", "v"), after):
        diff = np.abs(np.asarray(got, np.float64) - ref[q])
        tol = ref["tol_" + q]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(tol > 0, diff / tol, np.where(diff == 0, 0.0, np.inf))
        out[q] = np.where(np.isfinite(np.asarray(got, np.float64)), r, np.inf)
    return out


def check_step(before, after, g, t, lr, offsets, wd=0.0, la=0.0, anchor=None):
    """adam_ref.check_step for the regularised step: before / after = (params, exp_avg, exp_avg_sq) exported around
    optimizer step t, g the exported (scaled) gradient, anchor the exported anchor (None: none).  An adam_ref.StepCheck."""
    r = ratios(before, after, g, t, lr, wd, la, anchor)
    res = ar.StepCheck()
    for k, name in enumerate(ar.NAMES):
        res.add(name, {q: r[q][offsets[k]:offsets[k + 1]] for q in QUANTITIES})
    return res


def hashed_anchor(seed, n):
    """float32 [n] uniform in +-0.1, like hashed_step_inputs' p0"""
    return hf.hf_range(seed, (n,), -0.1, 0.1)


# ---- shrink and perturb
def draw(key, index, a):
    """a * (float32(k) * 2^-23) in float32 for the flat-vector elements `index`: recycle_ref.reinit_values with the bound
    given as a float32 instead of a layer name"""
    i = np.asarray(index, np.uint64)
    r = rr._splitmix64_np(np.uint64(rr.splitmix64(int(key) & rr.M64)) ^ i)
    k = (r >> np.uint64(40)).astype(np.int64) - 8388608
    w = np.float32(a) * (k.astype(np.float32) * np.float32(2.0 ** -23))
    assert w.dtype == np.float32
    return w


def perturbation(key, H, A):
    """xi, float32 [param_count] in the flat exported order: the draw for the four trunk weights (a_l of recycle_ref) and the
    action and value weight rows (fan_in = H), +0 for the six biases"""
    offs = ar.param_offsets(H, A)
    xi = np.zeros(int(offs[-1]), np.float32)
    bounds = {0: rr.bound("conv1"), 2: rr.bound("conv2"), 4: rr.bound("conv3"), 6: rr.bound("fc"),
              8: np.float32(np.sqrt(6.0 / H)), 10: np.float32(np.sqrt(6.0 / H))}
    for k, a in bounds.items():
        idx = np.arange(int(offs[k]), int(offs[k + 1]), dtype=np.uint64)
        xi[int(offs[k]):int(offs[k + 1])] = draw(key, idx, a)
    return xi


def shrink_perturb(params, shrink, sigma, key, H, A):
    """the parameters after aleppo_shrink_perturb(shrink, sigma, key): a new float32 array, three fp32 operations per
    element"""
    p = np.asarray(params, np.float32)
    lam, sg = np.float32(shrink), np.float32(sigma)
    a = lam * p
    b = sg * perturbation(key, H, A)
    out = a + b
    assert out.dtype == a.dtype == b.dtype == np.float32
    return out
