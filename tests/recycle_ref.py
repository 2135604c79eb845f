"""aleppo_recycle_units restated in numpy over the flat exported vectors (parameters, exp_avg, exp_avg_sq), bit for bit.

A plain helper module (no fixtures).  The table of include/aleppo.h, in the reference's tensor terms, with m1 .. m4 the
masks of conv1, conv2, conv3 and fc (mask: uint8 [160 + H] in the unit order of aleppo_activation_stats):
    conv1.w[o,c,kh,kw]   re-initialised if m1[o]
    conv2.w[o,c,kh,kw]   zero if m1[c], otherwise re-initialised if m2[o]
    conv3.w[o,c,kh,kw]   zero if m2[c], otherwise re-initialised if m3[o]
    fc.w[o, c*49 + p]    zero if m3[c], otherwise re-initialised if m4[o]
    the four biases [o]  zero if unit o is masked
    action.w[a,j], value.w[0,j]   zero if m4[j];   the head biases: never touched
Zero wins.  Both moments of every selected element become +0.0 unless keep_moments.  The re-initialised value of element i
of the flat vector: r = splitmix64(splitmix64(key) ^ i), k = (r >> 40) - 2^23, w = a_l * (float32(k) * 2^-23) in float32,
a_l = float32(sqrt(6 / fan_in))."""
import numpy as np

import adam_ref as ar

LAYERS = ("conv1", "conv2", "conv3", "fc")
ROWS = LAYERS + ("total",)
FAN_IN = dict(conv1=256, conv2=512, conv3=576, fc=3136)
LAYER_BITS = dict(conv1=1, conv2=2, conv3=4, fc=8)
M64 = (1 << 64) - 1


def first_units(H):
    return (0, 32, 96, 160, 160 + H)


def splitmix64(x):
    """the permutation of aleppo.h on a Python int"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _splitmix64_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def bound(layer):
    """a_l as float32"""
    return np.float32(np.sqrt(6.0 / FAN_IN[layer]))


def reinit_values(key, index, layer):
    """the re-initialised float32 values of the flat-vector elements `index` (any integer array) of `layer`'s weight"""
    i = np.asarray(index, np.uint64)
    r = _splitmix64_np(np.uint64(splitmix64(int(key) & M64)) ^ i)
    k = (r >> np.uint64(40)).astype(np.int64) - 8388608
    assert k.min(initial=0) >= -8388608 and k.max(initial=0) < 8388608
    w = bound(layer) * (k.astype(np.float32) * np.float32(2.0 ** -23))
    assert w.dtype == np.float32
    return w


def layer_masks(mask, H):
    m = np.asarray(mask, np.uint8).reshape(-1)
    assert m.shape == (160 + H,) and m.max(initial=0) <= 1
    f = first_units(H)
    return [m[f[l]:f[l + 1]].astype(bool) for l in range(4)]


def counts(mask, H):
    """{layer: masked units} over ROWS, as Engine.recycle_units returns it"""
    c = [int(m.sum()) for m in layer_masks(mask, H)]
    return dict(zip(ROWS, c + [sum(c)]))


def selection(mask, H, A):
    """(zero, reinit): bool [param_count] each, in the flat exported order; disjoint (zero wins)"""
    m1, m2, m3, m4 = layer_masks(mask, H)
    offs = ar.param_offsets(H, A)
    n = int(offs[-1])
    zero, reinit = np.zeros(n, bool), np.zeros(n, bool)

    def put(k, z, r=None):
        lo, hi = int(offs[k]), int(offs[k + 1])
        z = np.ascontiguousarray(z).reshape(-1)
        assert z.size == hi - lo, (k, z.size, hi - lo)
        zero[lo:hi] = z
        if r is not None:
            reinit[lo:hi] = np.ascontiguousarray(r).reshape(-1) & ~z

    none = np.zeros(4, bool)
    for k, (own, feed, khw) in enumerate(((m1, none, 64), (m2, m1, 16), (m3, m2, 9))):
        O, Cn = own.size, feed.size
        put(2 * k, np.broadcast_to(feed[None, :, None], (O, Cn, khw)), np.broadcast_to(own[:, None, None], (O, Cn, khw)))
        put(2 * k + 1, own)
    put(6, np.broadcast_to(m3[None, :, None], (H, 64, 49)), np.broadcast_to(m4[:, None, None], (H, 64, 49)))
    put(7, m4)
    put(8, np.broadcast_to(m4[None, :], (A, H)))
    put(10, m4)
    return zero, reinit


def apply(params, exp_avg, exp_avg_sq, mask, key, H, A, keep_moments=False):
    """the three vectors after aleppo_recycle_units(mask, key): new float32 arrays, the inputs are left alone"""
    p, m, v = (np.array(a, np.float32, copy=True) for a in (params, exp_avg, exp_avg_sq))
    offs = ar.param_offsets(H, A)
    assert p.shape == m.shape == v.shape == (int(offs[-1]),)
    zero, reinit = selection(mask, H, A)
    p[zero] = np.float32(0)
    for k, layer in zip((0, 2, 4, 6), LAYERS):
        idx = np.nonzero(reinit[int(offs[k]):int(offs[k + 1])])[0] + int(offs[k])
        p[idx] = reinit_values(key, idx, layer)
    assert not reinit[int(offs[7]):].any() and not (reinit & zero).any()
    if not keep_moments:
        sel = zero | reinit
        m[sel] = np.float32(0)
        v[sel] = np.float32(0)
    return p, m, v


def keyed_mask(seed, H, density=0.25):
    """a reproducible random mask: unit u is masked where a hash of (seed, u) falls below `density`"""
    import hashfill as hf
    return (hf.hf_unit(seed, 160 + H) < np.float32(density)).astype(np.uint8)
