"""Reference of ALEPPO_F_BATCH_STATS (include/aleppo.h): the definition in numpy float64, two-pass (np.mean, np.var), from
the four planes as stored - and, per statistic, the bound a one-pass double-precision reduction is held to.

The bound is derived, not tuned.  The inputs (float32 widened) are exact in double.  A double sum of N terms carries at most
N * 2^-53 relative error on sums of one sign, and var = Q / n - mean^2 amplifies it by 1 + mean^2 / var.  So for a plane x
    rel_x = 8 * N * 2^-53 * (1 + mean_x^2 / var_x)
means are held to rel_x * max(|mean_x|, std_x), stds to rel_x * std_x, and the explained variance 1 - var_d / var_R to
(rel_R + rel_d) absolute, times var_d / var_R where that is above 1.  A plane of zero variance has no such rel (mean^2 /
var is infinite): its statistics are held to EXACT equality (bound 0), which holds when its sums are exact in double, so
the tests use constants of few significant bits there.  Every test asserts bound <= MAX_BOUND before it uses a bound, so
that a bound cannot grow until it hides a fault."""
import numpy as np

NAMES = ("count", "explained_variance", "value_mean", "value_std", "return_mean", "return_std", "advantage_mean",
         "advantage_std", "residual_mean", "residual_std")
MAX_BOUND = 1e-6
CHUNK = 4096  # samples per workgroup of the device's first stage (a function of nothing but the sample count)


def _planes(values, returns, advantages, masks):
    v = np.asarray(values, np.float32).ravel().astype(np.float64)
    r = np.asarray(returns, np.float32).ravel().astype(np.float64)
    a = np.asarray(advantages, np.float32).ravel().astype(np.float64)
    m = np.asarray(masks).ravel() != 0
    assert v.shape == r.shape == a.shape == m.shape
    return v, r, a, m


def reference(values, returns, advantages, masks):
    """(stats, bounds): dicts over NAMES.  bounds["count"] is 0 (the count is exact)."""
    v, r, a, m = _planes(values, returns, advantages, masks)
    N = v.size
    v, r, a = v[m], r[m], a[m]
    n = int(m.sum())
    stats = dict(count=float(n))
    bounds = dict(count=0.0)
    if n == 0:
        for name in NAMES[2:]:
            stats[name] = 0.0
            bounds[name] = 0.0
        stats["explained_variance"] = float("nan")
        bounds["explained_variance"] = 0.0
        return stats, bounds
    rel, var = {}, {}
    for key, x in (("value", v), ("return", r), ("advantage", a), ("residual", r - v)):
        mean, var[key] = float(np.mean(x)), float(np.var(x))
        std = float(np.sqrt(var[key]))
        stats[key + "_mean"], stats[key + "_std"] = mean, std
        if var[key] == 0.0:  # a constant plane: exact (bound 0) - the tests use constants whose sums are exact in double
            rel[key] = 0.0
        else:
            rel[key] = 8.0 * N * 2.0 ** -53 * (1.0 + mean * mean / var[key])
        bounds[key + "_mean"] = rel[key] * max(abs(mean), std)
        bounds[key + "_std"] = rel[key] * std
    if var["return"] == 0.0:
        stats["explained_variance"] = float("nan")
        bounds["explained_variance"] = 0.0
    else:
        ratio = var["residual"] / var["return"]
        stats["explained_variance"] = 1.0 - ratio
        bounds["explained_variance"] = (rel["return"] + rel["residual"]) * max(1.0, ratio)
    return stats, bounds


def one_pass_in_device_order(values, returns, advantages, masks):
    """the same ten numbers the way the device sums them (aleppo.h): count, sum and sum of squares in double, chunks of
    CHUNK samples, 256 strided accumulators per chunk folded by a fixed tree (xor butterflies over 64 lanes, then
    (w0 + w1) + (w2 + w3)), chunks added in index order; then mean = S / n, var = max(0, Q / n - mean^2)."""
    v, r, a, m = _planes(values, returns, advantages, masks)
    d = r - v
    terms = np.stack([np.ones_like(v), v, v * v, r, r * r, a, a * a, d, d * d]) * m  # [9][N]
    N = v.size
    nblk = (N + CHUNK - 1) // CHUNK
    pad = np.zeros((9, nblk * CHUNK))
    pad[:, :N] = terms
    acc = np.zeros((9, nblk, 256))
    for k in range(CHUNK // 256):  # thread t adds samples t, t + 256, ... in turn
        acc += pad.reshape(9, nblk, CHUNK // 256, 256)[:, :, k, :]
    w = acc.reshape(9, nblk, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., np.arange(64) ^ o]
    w = w[..., 0]
    part = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])  # [9][nblk]
    sums = np.zeros(9)
    for b in range(nblk):
        sums += part[:, b]
    n = sums[0]
    out = dict(count=float(n))
    var = []
    for k, key in enumerate(("value", "return", "advantage", "residual")):
        S, Q = sums[1 + 2 * k], sums[2 + 2 * k]
        mean = S / n if n > 0 else 0.0
        var.append(max(0.0, Q / n - mean * mean) if n > 0 else 0.0)
        out[key + "_mean"], out[key + "_std"] = float(mean), float(np.sqrt(var[-1]))
    out["explained_variance"] = float(1.0 - var[3] / var[1]) if n > 0 and var[1] > 0 else float("nan")
    return out


def assert_close(got, stats, bounds, what=""):
    """every statistic of `got` (dict over NAMES) within its bound of the reference; prints each figure first"""
    for name in NAMES:
        g, w, b = got[name], stats[name], bounds[name]
        err = 0.0 if (np.isnan(g) and np.isnan(w)) else abs(g - w)
        print(f"{what} {name}: got {g!r} want {w!r} err {err:.3e} bound {b:.3e}")
    for name in NAMES:
        g, w, b = got[name], stats[name], bounds[name]
        assert b <= MAX_BOUND, (what, name, b)
        if np.isnan(w):
            assert np.isnan(g), (what, name, g)
        else:
            assert abs(g - w) <= b, (what, name, g, w, b)
