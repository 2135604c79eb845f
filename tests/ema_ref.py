"""numpy restatement of aleppo_ema_update (include/aleppo.h): the three-operation fp32 rule and the six statistics in
float64, on flat vectors in any order (the rule is element-wise; the alignment pads of the private layout are zero, stay
zero and add nothing to a sum of squares, so the exported vectors give the same figures).  Two PLANTED wrong forms of the
rule - what a compiler's contraction or a tidy-minded rewrite would produce - are here so that a test can show that the
bit-for-bit check tells them from the rule."""
import numpy as np

STATS = ("updates", "decay", "norm", "param_norm", "distance", "relative_distance")
U = 2.0 ** -53  # the unit roundoff of binary64


def scalars(decay):
    """(d, w) as the library forms them, once, on the host: d = (float)decay, w = (float)(1.0 - decay) with the
    subtraction in double"""
    decay = float(decay)
    return np.float32(decay), np.float32(1.0 - decay)


def valid(decay):
    decay = float(decay)
    return bool(np.isfinite(decay) and 0.0 <= decay < 1.0)


def update(e, p, decay):
    """a = d * e; b = w * p; e' = a + b - three fp32 operations, each rounded"""
    d, w = scalars(decay)
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    a = d * e
    b = w * p
    assert a.dtype == np.float32 and b.dtype == np.float32
    return a + b


def update_fma(e, p, decay):
    """PLANTED: the contracted form.  Both products are exact in float64 (24 x 24 bits), their sum is rounded to float64
    and then once to float32 - fma(d, e, w * p) up to the rare double-rounding case, and never the two roundings of the
    products"""
    d, w = scalars(decay)
    s = np.float64(d) * np.asarray(e, np.float64) + np.float64(w) * np.asarray(p, np.float64)
    return s.astype(np.float32)


def update_lerp(e, p, decay):
    """PLANTED: e + w (p - e), the two-operand interpolation, in fp32"""
    _, w = scalars(decay)
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    return e + w * (p - e)


def stats(e, p, updates, decay):
    """the six doubles after an update that left the average e beside the parameters p (decay: of that update; None: no
    update yet - open, import)"""
    e64, p64 = np.asarray(e, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    s_e, s_p, s_d = float(np.sum(e64 * e64)), float(np.sum(p64 * p64)), float(np.sum((p64 - e64) ** 2))
    d = 0.0 if decay is None else float(scalars(decay)[0])
    return dict(updates=float(updates), decay=d, norm=np.sqrt(s_e), param_norm=np.sqrt(s_p), distance=np.sqrt(s_d),
                relative_distance=np.sqrt(s_d / s_p) if s_p > 0 else 0.0)


def padded_count(H, A):
    """elements of the private layout: every tensor padded to a multiple of 64 floats"""
    sizes = ((A + 1) * H, A + 1, H * 3136, H, 64 * 576, 64, 64 * 512, 64, 32 * 256, 32)
    return sum((s + 63) // 64 * 64 for s in sizes)


def stat_bounds(n):
    """relative bounds on |device - stats()| for the three norms and for the ratio, n the padded element count.  A sum of
    squares: each term carries at most 3 roundings (the difference, the product, nothing else) and the sum n - 1 more, in
    either order, so each side is within (n + 2) U of the exact sum and the two sides within 2 (n + 2) U of each other.
    A root halves a relative error and adds one rounding on each side: (n + 2) U + 2 U.  The ratio: two such sums and one
    quotient rounding on each side, 4 (n + 2) U + 2 U, halved by the root, plus its two roundings."""
    return (n + 4) * U, (2 * n + 7) * U


def warmup_decay(ema_decay, n):
    """the trainer's ema_warmup rule (TensorFlow / timm): the decay of update n, n the updates so far"""
    return min(float(ema_decay), (1.0 + n) / (10.0 + n))
