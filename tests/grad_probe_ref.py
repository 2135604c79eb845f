"""The host reference of aleppo_grad_gram and its error bound.  A plain helper module (no fixtures), used by
test_grad_probe_cpu.py and test_grad_probe.py.

gram(vectors, H, A): flat float32 vectors in libtorch parameters() order are cut into the 12 tensors; entry [r][i][j] is
math.fsum of the products x_i[e] * x_j[e] over tensor r, formed in float64 - exact, 24 + 24 significand bits fit in 53 -
so the entry is the correctly rounded exact sum.  An element index at which any of the vectors is NaN / Inf is left out of
every entry and counted once in nonfinite[r]; row 12 is the whole model (fsum over all its elements, the counts added).

bound(vectors, H, A): what a device sum of the same n_r exact terms in ANY fixed order may differ from that by.  Each of
the n_r - 1 additions rounds once, relatively by at most u = 2^-53, and the partial sums are bounded by sum |x_i x_j| up
to a factor (1 + u)^(n_r - 1); to first order in u (Higham 2002, Accuracy and Stability of Numerical Algorithms, eq. 4.4:
|E| <= (n - 1) u sum |t_k| + O(u^2)):
    |device - exact| <= (n_r - 1) * 2^-53 * sum |x_i x_j|
The partial sum that addition k rounds is bounded by the sum of the |t| it has gathered so far, not by the whole of
sum |t_k|, so the first-order bound is never attained on more than two terms; that slack also covers the second-order term
(a relative n_r u < 2^-32 of the bound) and the reference's own single rounding of the exact sum.  A tensor of one element
has the bound 0: one exact product, no addition.  Derived, not measured."""
import math

import numpy as np

NAMES = ("conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
         "value.w", "value.b")
U = 2.0 ** -53


def sizes(H, A):
    return [32 * 4 * 8 * 8, 32, 64 * 32 * 4 * 4, 64, 64 * 64 * 3 * 3, 64, H * 3136, H, A * H, A, H, 1]


def bounds(H, A):
    """[(begin, end)] of the 12 tensors in a flat vector"""
    edges = np.concatenate([[0], np.cumsum(sizes(H, A))])
    return [(int(edges[r]), int(edges[r + 1])) for r in range(12)]


def _stack(vectors, H, A):
    x = np.stack([np.asarray(v, np.float32).ravel() for v in vectors])
    assert x.shape[1] == sum(sizes(H, A)), "a flat vector in libtorch parameters() order"
    return x, np.isfinite(x).all(axis=0)


def gram(vectors, H, A):
    """(float64 [13, k, k], int64 [13]): the exact Gram per tensor, correctly rounded, and the left-out counts"""
    x, ok = _stack(vectors, H, A)
    k = x.shape[0]
    d = np.where(ok, x, np.float32(0)).astype(np.float64)
    g = np.zeros((13, k, k), np.float64)
    nf = np.zeros(13, np.int64)
    spans = bounds(H, A) + [(0, x.shape[1])]
    for r, (b, e) in enumerate(spans):
        nf[r] = int((~ok[b:e]).sum())
        for i in range(k):
            for j in range(i, k):
                g[r, i, j] = g[r, j, i] = math.fsum(d[i, b:e] * d[j, b:e])
    return g, nf


def bound(vectors, H, A):
    """float64 [13, k, k]: (n_r - 1) * 2^-53 * sum |x_i x_j| over the elements that enter (see the module docstring)"""
    x, ok = _stack(vectors, H, A)
    k = x.shape[0]
    d = np.abs(np.where(ok, x, np.float32(0)).astype(np.float64))
    out = np.zeros((13, k, k), np.float64)
    spans = bounds(H, A) + [(0, x.shape[1])]
    for r, (b, e) in enumerate(spans):
        for i in range(k):
            for j in range(i, k):
                out[r, i, j] = out[r, j, i] = (e - b - 1) * U * math.fsum(d[i, b:e] * d[j, b:e])
    return out


def check(got, got_nf, vectors, H, A):
    """assert a device (or planted) Gram against the reference at the derived bound; returns the largest |error| / bound"""
    want, nf = gram(vectors, H, A)
    lim = bound(vectors, H, A)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.array_equal(np.asarray(got_nf, np.int64), nf), (got_nf, nf)
    bad = err > lim
    assert not bad.any(), [(int(r), int(i), int(j), err[r, i, j], lim[r, i, j]) for r, i, j in np.argwhere(bad)[:8]]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(lim > 0, err / lim, 0.0)))
