"""The numpy restatement of aleppo_saliency's definitions (include/aleppo.h): the grid, the two integer tables, the
separable reflected blur, the blended perturbed stacks and the scores.  A plain helper module (no fixtures).  The pixel
arithmetic is integer arithmetic, so `perturbed` is what the engine must return byte for byte; it takes the tables as an
argument (the library's own, from aleppo_saliency_tables), and `tables` is the same computation in numpy's double for the
test of the tables themselves."""
import numpy as np

W = 84
DEFAULTS = dict(stride=5, sigma_mask=5.0, sigma_blur=3.0, planes=15)


def grid(stride):
    """G: points per axis; point (gy, gx) has its centre at pixel (gy * stride, gx * stride)"""
    return (W + stride - 1) // stride


def tables(sigma_mask, sigma_blur):
    """(g uint16 [84], w uint16 [84] - w[0 .. R], zero beyond -, R) in numpy's double"""
    k = np.arange(W, dtype=np.float64)
    g = np.rint(4096.0 * np.exp(-k * k / (2.0 * sigma_mask * sigma_mask)))
    R = int(4.0 * sigma_blur + 0.5)
    e = np.exp(-(k[:R + 1] ** 2) / (2.0 * sigma_blur * sigma_blur))
    total = 0.0
    for j in range(-R, R + 1):
        total += e[abs(j)]
    w = np.zeros(W, np.int64)
    w[:R + 1] = np.rint(4096.0 * e / total).astype(np.int64)
    w[0] += 4096 - (w[0] + 2 * w[1:].sum())
    return g.astype(np.uint16), w.astype(np.uint16), R


def _reflect(i):
    i = np.where(i < 0, -1 - i, i)
    return np.where(i > W - 1, 2 * W - 1 - i, i)


def blur(planes_u8, w, R):
    """B of uint8 [..., 84, 84] planes: horizontal pass, then vertical, reflected; every partial sum is checked to fit 32 bits"""
    I = np.asarray(planes_u8).astype(np.uint64)
    taps = np.asarray(w, np.uint64)
    x = np.arange(W)
    hh = np.zeros(I.shape, np.uint64)
    for j in range(-R, R + 1):
        hh += taps[abs(j)] * I[..., :, _reflect(x + j)]
    v = np.zeros(I.shape, np.uint64)
    for j in range(-R, R + 1):
        v += taps[abs(j)] * hh[..., _reflect(x + j), :]
    assert int(hh.max(initial=0)) < 2 ** 32 and int(v.max(initial=0)) + 2 ** 23 < 2 ** 32
    return ((v + np.uint64(2 ** 23)) >> np.uint64(24)).astype(np.uint8)


def mask(g, stride, p):
    """m uint32 [84, 84] of position p = gy * G + gx, in [0, 256]"""
    G = grid(stride)
    cy, cx = (p // G) * stride, (p % G) * stride
    k = np.arange(W)
    gg = np.asarray(g, np.uint64)
    m = (gg[np.abs(k - cy)][:, None] * gg[np.abs(k - cx)][None, :] + np.uint64(2 ** 15)) >> np.uint64(16)
    assert int(m.max()) <= 256
    return m


def perturbed(obs, g, w, R, stride=5, planes=15, positions=None):
    """uint8 [n, len(positions), 4, 84, 84]: the stacks the forward pass sees (positions: default all G * G)"""
    obs = np.asarray(obs, np.uint8)
    G = grid(stride)
    positions = range(G * G) if positions is None else positions
    B = blur(obs, w, R).astype(np.uint64)
    I = obs.astype(np.uint64)
    out = np.empty((obs.shape[0], len(positions)) + obs.shape[1:], np.uint8)
    sel = np.array([(planes >> k) & 1 for k in range(4)], bool)
    for q, p in enumerate(positions):
        m = mask(g, stride, p)
        blend = ((I * (np.uint64(256) - m) + B * m + np.uint64(128)) >> np.uint64(8)).astype(np.uint8)
        out[:, q] = np.where(sel[None, :, None, None], blend, obs)
    return out


def scores(outputs):
    """(S_policy, S_value) float64 [n, P] from outputs [n, P + 1, A + 1] (row 0: the unperturbed logits and value)"""
    o = np.asarray(outputs, np.float64)
    d = o[:, :1, :] - o[:, 1:, :]
    return 0.5 * (d[..., :-1] ** 2).sum(-1), 0.5 * d[..., -1] ** 2


def score_bound(s_ref, terms):
    """|S - S_ref| allowed for a fp32 sum of `terms` squared fp32 differences, S_ref from the same fp32 inputs in float64: one
    rounding in the difference, one in the square, terms - 1 in the sum, each 2^-24 relative, then doubled (the rounded
    difference enters squared); the absolute term covers a square that underflows"""
    return 2.0 * (terms + 2) * 2.0 ** -24 * np.asarray(s_ref, np.float64) + 1e-37


def half_saturated(u8, unit):
    """random bytes with about half of the pixels saturated to 255 (unit: uniform [0, 1) of the same shape)"""
    return np.where(unit < 0.5, np.uint8(255), u8).astype(np.uint8)


def upsample(score, stride):
    """[.., G, G] scores -> [.., 84, 84]: pixel (y, x) takes grid point (min(G-1, (y + d/2) / d), min(G-1, (x + d/2) / d))"""
    G = grid(stride)
    i = np.minimum(G - 1, (np.arange(W) + stride // 2) // stride)
    return np.asarray(score)[..., i[:, None], i[None, :]]


def uv_bytes(score, maximum):
    """128 + rint(127 * S / max) as uint8; a zero or non-finite maximum gives 128"""
    s = np.asarray(score, np.float64)
    if not (np.isfinite(maximum) and maximum > 0):
        return np.full(s.shape, 128, np.uint8)
    return (128 + np.rint(127.0 * s / maximum)).astype(np.uint8)
