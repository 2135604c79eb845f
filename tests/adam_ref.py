"""One clip + Adam step, restated: the float64 reference, its per-element fp32 rounding bounds, an fp32 restatement
of the kernel's adam_element, and the checker the CPU and GPU tests of tests/test_optimizer_step.py share.

A plain helper module (no fixtures).  The tail of every update is elementwise fp32 arithmetic on values the C ABI
exports: the parameters and both moments before a step, the step count, and aleppo_export_grads - the already scaled
gradient g, "the bits the kernel multiplied into its update".  The moments and parameters after the step follow from
those in any precision to a handful of fp32 roundings; bf16 noise of the gradient does not enter.

The step, with the scalars as the host builds them (api_train.hip, upload_call_scalars): beta1 / beta2 / eps the
float32 values of 0.9 / 0.999 / 1e-5, s = float32(lr / (1 - beta1^t)), c = float32(sqrt(1 - beta2^t)):
    m = beta1 m0 + (1 - beta1) g
    v = beta2 v0 + (1 - beta2) g^2
    d = sqrt(v) / c + eps
    p = p0 - s m / d

Bounds, u = 2^-24 (half an fp32 ulp, relative).  The plain count of adam_element's roundings:
    m: two products and a sum                                     -> 3u (|beta1 m0| + |(1 - beta1) g|)
    v: g^2, two products, a sum, all terms >= 0                   -> 4u v
    d: v's 3u halved by the root, the root, the quotient, the sum -> 4.5u d, so m / d carries 5.5u |m| + tol_m,
       the product with s one more, and p's own rounding u |p|    -> u |p| + (s / d) (3u (...) + 8u |m|)
The bounds are TWICE that count - room for fused multiply-adds and for a division or square root that is not
correctly rounded:
    tol_m = 4u (|beta1 m0| + |(1 - beta1) g|)
    tol_v = 6u v
    tol_p = 2u |p| + (s / d) (tol_m + 16u |m|)
Where a bound is exactly 0 (m0 = g = 0, or v0 = g = 0) the device value must equal the reference exactly.
A numpy fp32 restatement of the step stays within 0.5 of each (test_fp32_restatement_within_half_of_every_bound)."""
import numpy as np

import hashfill as hf

U = 2.0 ** -24
BETA1, BETA2, EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-5)
NAMES = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
         "value.w", "value.b"]
QUANTITIES = ("m", "v", "p")


def param_offsets(H, A):
    """the 13 edges of the 12 tensors in the flat vector of libtorch's parameters() order"""
    return np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in hf.param_shapes(H, A)])]).astype(np.int64)


def step_scalars(t, lr):
    """(s, c) of optimizer step t as float32: the two device scalars of the step's schedule slot"""
    b1, b2, t = float(BETA1), float(BETA2), float(t)
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(np.sqrt(1.0 - b2 ** t))


def clip_coef(max_norm, norm):
    """min(1, max_norm / (norm + 1e-6)) in float32, as adam_kernel and aleppo_export_grads form it"""
    coef = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(min(coef, np.float32(1.0)))


def adam_f64(p0, m0, v0, g, s, c, eps=EPS, beta1=BETA1, beta2=BETA2):
    """the step in float64 on fp32 inputs: (p, m, v, d)"""
    p0, m0, v0, g = (np.asarray(a, np.float64) for a in (p0, m0, v0, g))
    b1, b2 = float(beta1), float(beta2)
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * g * g
    d = np.sqrt(v) / float(c) + float(eps)
    return p0 - float(s) * m / d, m, v, d


def reference_step(p0, m0, v0, g, t, lr):
    """step t in float64 and its bounds: dict of p, m, v and tol_p, tol_m, tol_v (float64 arrays)"""
    s, c = step_scalars(t, lr)
    p, m, v, d = adam_f64(p0, m0, v0, g, s, c)
    b1 = float(BETA1)
    tol_m = 4 * U * (np.abs(b1 * np.asarray(m0, np.float64)) + np.abs((1.0 - b1) * np.asarray(g, np.float64)))
    tol_v = 6 * U * v
    tol_p = 2 * U * np.abs(p) + (float(s) / d) * (tol_m + 16 * U * np.abs(m))
    return dict(p=p, m=m, v=v, tol_p=tol_p, tol_m=tol_m, tol_v=tol_v)


def adam_element_f32(p0, m0, v0, g, t, lr):
    """kernels.hip adam_element in numpy float32, operation for operation (g already scaled): (p, m, v)"""
    p0, m0, v0, g = (np.asarray(a, np.float32) for a in (p0, m0, v0, g))
    s, c = step_scalars(t, lr)
    omb1, omb2 = np.float32(1.0) - BETA1, np.float32(1.0) - BETA2
    m = m0 * BETA1 + omb1 * g
    v = v0 * BETA2 + omb2 * (g * g)
    denom = np.sqrt(v) / c + EPS
    p = p0 - s * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def ratios(before, after, g, t, lr):
    """per element |device - reference| / bound for m, v, p -> {"m": ..., "v": ..., "p": ...} (float64 arrays).
    before / after: (p, m, v) around the step.  A zero bound with an equal value gives 0, with any difference inf."""
    p0, m0, v0 = before
    ref = reference_step(p0, m0, v0, g, t, lr)
    out = {}
    for q, got in zip(("p", "m", "v"), after):
        diff = np.abs(np.asarray(got, np.float64) - ref[q])
        tol = ref["tol_" + q]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(tol > 0, diff / tol, np.where(diff == 0, 0.0, np.inf))
        out[q] = np.where(np.isfinite(np.asarray(got, np.float64)), r, np.inf)
    return out


class StepCheck:
    """the checker's result: report[tensor][q] = (worst ratio to bound, flat index inside the tensor), failures lists
    (tensor, q, ratio, index) of every ratio above 1, worst[q] = (ratio, tensor, index) over all tensors"""

    def __init__(self):
        self.report, self.failures = {}, []
        self.worst = {q: (0.0, None, -1) for q in QUANTITIES}

    def add(self, name, r):
        self.report[name] = {}
        for q in QUANTITIES:
            if r[q].size == 0:
                continue
            i = int(np.argmax(r[q]))
            x = float(r[q][i])
            self.report[name][q] = (x, i)
            if not x <= 1.0:
                self.failures.append((name, q, x, i))
            if not x <= self.worst[q][0]:
                self.worst[q] = (x, name, i)

    def merge(self, other):
        for q in QUANTITIES:
            if not other.worst[q][0] <= self.worst[q][0]:
                self.worst[q] = other.worst[q]
        self.failures += other.failures

    def summary(self, title):
        return "%s %s" % (title, {q: "%.3g/1 at %s[%d]" % self.worst[q] for q in QUANTITIES})


def check_step(before, after, g, t, lr, offsets):
    """before / after: (params, exp_avg, exp_avg_sq) exported around optimizer step t, g: the exported (scaled)
    gradient of that step, offsets: param_offsets(H, A).  Every element of all 12 tensors; fails (result.failures)
    on any ratio above 1."""
    r = ratios(before, after, g, t, lr)
    res = StepCheck()
    for k, name in enumerate(NAMES):
        res.add(name, {q: r[q][offsets[k]:offsets[k + 1]] for q in QUANTITIES})
    return res


# ---- hashed optimizer states (closed-form in (seed, index), like hashfill)
def _log_uniform(seed, n, lo_exp, hi_exp):
    return np.power(10.0, lo_exp + (hi_exp - lo_exp) * hf.hf_unit(seed, n).astype(np.float64))


def _sign(seed, n):
    return np.where(hf.hf_u32(seed, n) & np.uint32(1), -1.0, 1.0)


def hashed_moments(seed, n, g=None):
    """(m0, v0) float32 [n]: |m0| log-uniform in 1e-12 .. 1 with a hashed sign, v0 log-uniform in 1e-24 .. 1; both zero
    on one element in five; with g given, m0 = -0.11 g on (a hashed) half of the elements - cancellation in m"""
    m0 = _sign(seed, n) * _log_uniform(seed + 1, n, -12, 0)
    v0 = _log_uniform(seed + 2, n, -24, 0)
    if g is not None:
        m0 = np.where(hf.hf_u32(seed + 3, n) & np.uint32(1), -0.11 * np.asarray(g, np.float64), m0)
    zero = hf.hf_u32(seed + 4, n) % np.uint32(5) == 0
    return np.where(zero, 0.0, m0).astype(np.float32), np.where(zero, 0.0, v0).astype(np.float32)


def hashed_step_inputs(seed, n):
    """(p0, m0, v0, g) float32 [n] for the CPU tests: |g| log-uniform in 1e-12 .. 10 with a hashed sign and every
    third g zero, the moments of hashed_moments (zero moments, cancellation against g), p0 uniform in +-0.1"""
    g = _sign(seed, n) * _log_uniform(seed + 1, n, -12, 1)
    g = np.where(np.arange(n) % 3 == 0, 0.0, g).astype(np.float32)
    m0, v0 = hashed_moments(seed + 10, n, g)
    return hf.hf_range(seed + 20, (n,), -0.1, 0.1), m0, v0, g
