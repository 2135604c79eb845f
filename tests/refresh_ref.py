"""Reference of aleppo_refresh_advantages (include/aleppo.h): what the call leaves in the advantage, return and mask planes
and in its thirteen statistics, from the fresh values and the planes as they stood at entry.

Planes: the oracle's fp32 GAE (oracle_lib.gae, the pinned op order of aleppo_finish_rollout's scan) on the stored rewards AS
THEY STAND, the stored flags and the fresh values as stored - rounded to IEEE half where the rollout planes are half;
returns = a + v_fresh in fp32; both rounded to half where the planes are half (the recursion keeps fp32); with
advantage_norm, orc.adv_norm on the stored advantages.  The statistics are batch_stats_ref's two-pass float64 definition
with v := the fresh values as stored and R, a := the planes at entry, extended by d' = v_fresh - v_collected; `rel`, the
bounds and MAX_BOUND are as they are there, and the d' plane gets the same treatment as the four others."""
import numpy as np

import batch_stats_ref as br
import oracle_lib as orc

EXTRA = ("value_change_mean", "value_change_std", "value_change_maxabs")
NAMES = br.NAMES + EXTRA
MAX_BOUND = br.MAX_BOUND
CHUNK = br.CHUNK


def half(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def stored(x, rt16):
    """x as a rollout plane holds it"""
    return half(x) if rt16 else np.asarray(x, np.float32)


def planes(rewards, fresh, fresh_next, term, trunc, start, *, gamma=0.99, lam=0.95, rt16=False, adv_norm=False):
    """(values, next_values, advantages, returns, masks) the call leaves; everything env-major [E, T] / [E]"""
    v, nv = stored(fresh, rt16), stored(fresh_next, rt16)
    adv = orc.gae(rewards, v, nv, term, trunc, start, gamma=gamma, lam=lam)
    ret = stored(adv + v, rt16)
    adv = stored(adv, rt16)
    masks = (1 - np.asarray(start, np.uint8)).astype(np.uint8)
    if adv_norm:
        adv = stored(orc.adv_norm(adv, masks).reshape(adv.shape), rt16)
    return v, nv, adv, ret, masks


def stats(fresh_stored, collected, returns_entry, advantages_entry, masks):
    """(stats, bounds): dicts over NAMES, two-pass float64; count and value_change_maxabs are exact (bound 0)"""
    s, b = br.reference(fresh_stored, returns_entry, advantages_entry, masks)
    m = np.asarray(masks).ravel() != 0
    N = m.size
    d = (np.asarray(fresh_stored, np.float32).ravel().astype(np.float64) -
         np.asarray(collected, np.float32).ravel().astype(np.float64))[m]
    if d.size == 0:
        s.update(dict.fromkeys(EXTRA, 0.0))
        b.update(dict.fromkeys(EXTRA, 0.0))
        return s, b
    mean, var = float(np.mean(d)), float(np.var(d))
    std = float(np.sqrt(var))
    rel = 0.0 if var == 0.0 else 8.0 * N * 2.0 ** -53 * (1.0 + mean * mean / var)
    s.update(value_change_mean=mean, value_change_std=std, value_change_maxabs=float(np.max(np.abs(d))))
    b.update(value_change_mean=rel * max(abs(mean), std), value_change_std=rel * std, value_change_maxabs=0.0)
    return s, b


def refresh(rewards, fresh, fresh_next, collected, term, trunc, start, returns_entry, advantages_entry, *, gamma=0.99,
            lam=0.95, rt16=False, adv_norm=False):
    """the definition: dict(values, next_values, advantages, returns, masks, stats, bounds)"""
    v, nv, adv, ret, masks = planes(rewards, fresh, fresh_next, term, trunc, start, gamma=gamma, lam=lam, rt16=rt16,
                                    adv_norm=adv_norm)
    s, b = stats(v, collected, returns_entry, advantages_entry, masks)
    return dict(values=v, next_values=nv, advantages=adv, returns=ret, masks=masks, stats=s, bounds=b)


def one_pass_in_device_order(fresh_stored, collected, returns_entry, advantages_entry, masks):
    """the thirteen numbers the way the device sums them: batch_stats_ref's restatement for the first ten, and S and Q of
    d' through the same chunks, strided accumulators and tree; the maximum is order-free"""
    out = br.one_pass_in_device_order(fresh_stored, returns_entry, advantages_entry, masks)
    m = (np.asarray(masks).ravel() != 0).astype(np.float64)
    d = (np.asarray(fresh_stored, np.float32).ravel().astype(np.float64) -
         np.asarray(collected, np.float32).ravel().astype(np.float64))
    terms = np.stack([m, d * m, d * d * m])
    N = d.size
    nblk = (N + CHUNK - 1) // CHUNK
    pad = np.zeros((3, nblk * CHUNK))
    pad[:, :N] = terms
    acc = np.zeros((3, nblk, 256))
    for k in range(CHUNK // 256):
        acc += pad.reshape(3, nblk, CHUNK // 256, 256)[:, :, k, :]
    w = acc.reshape(3, nblk, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., np.arange(64) ^ o]
    w = w[..., 0]
    part = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    sums = np.zeros(3)
    for k in range(nblk):
        sums += part[:, k]
    n = sums[0]
    mean = sums[1] / n if n > 0 else 0.0
    var = max(0.0, sums[2] / n - mean * mean) if n > 0 else 0.0
    out.update(value_change_mean=float(mean), value_change_std=float(np.sqrt(var)),
               value_change_maxabs=float(np.max(np.abs(d) * m)) if N else 0.0)
    return out


def assert_stats(got, want, bounds, what=""):
    """every statistic of `got` (dict over NAMES) within its bound; prints each figure first; count and max-abs exact"""
    for name in NAMES:
        g, w, b = got[name], want[name], bounds[name]
        err = 0.0 if (np.isnan(g) and np.isnan(w)) else abs(g - w)
        print(f"{what} {name}: got {g!r} want {w!r} err {err:.3e} bound {b:.3e}")
    for name in NAMES:
        g, w, b = got[name], want[name], bounds[name]
        assert b <= MAX_BOUND, (what, name, b)
        if np.isnan(w):
            assert np.isnan(g), (what, name, g)
        else:
            assert abs(g - w) <= b, (what, name, g, w, b)
    assert got["count"] == want["count"] and got["value_change_maxabs"] == want["value_change_maxabs"], what


# ------------------------------------------------------------------ the rows the tests run (the issue's table)
# name: (E, T, A, H, precision, fp16 planes, max_minibatch, reward scaling, advantage_norm)
ROWS = dict(
    fp32=(5, 7, 4, 32, "fp32", False, 16, False, False),         # chunks 16 / 16 / 3, T below one GAE chunk
    bf16=(3, 33, 6, 96, "bf16", False, 33, False, False),        # ragged top + two full 16-step GAE chunks
    fp16_planes=(65, 4, 18, 32, "bf16", True, 130, False, False),  # second GAE workgroup with one thread, half rounding
    reward_scale=(5, 7, 4, 32, "fp32", False, 16, True, False),  # rewards not rescaled
    adv_norm=(5, 7, 4, 32, "fp32", False, 16, False, True),      # returns bit-exact, advantages at the adv_norm bound
)


def row_flags(seed, E, T, p=0.08):
    """time-major (terminals, truncations, starts) [T, E] in the slot protocol (a terminated / truncated slot is followed
    by one start slot; slot 0 starts every environment), hashed, with a truncation at t = T - 1 (environment 0: the fresh
    bootstrap value matters), a terminal at t = T - 2 and so a start at t = T - 1 (environment 1), a terminal at t = 1
    (environment 2)"""
    import hashfill as hf
    assert E >= 3 and T >= 4
    u = hf.hf_unit(seed, T * E).reshape(T, E)
    te, tr = u < np.float32(p / 2), (u >= np.float32(p / 2)) & (u < np.float32(p))
    te[[T - 2, T - 1], 0] = tr[T - 2, 0] = False
    tr[T - 1, 0] = True
    te[[T - 3, T - 1], 1] = tr[[T - 3, T - 2, T - 1], 1] = False
    te[T - 2, 1] = True
    te[1, 2], tr[1, 2] = True, False
    st = np.zeros((T, E), bool)
    st[0] = True
    for t in range(T):
        te[t] &= ~st[t]
        tr[t] &= ~st[t] & ~te[t]
        if t + 1 < T:
            st[t + 1] = te[t] | tr[t]
    te, tr, st = (x.astype(np.uint8) for x in (te, tr, st))
    assert tr[T - 1, 0] and te[T - 2, 1] and st[T - 1, 1] and te[1, 2] and st[0].all() and (te + tr + st).max() == 1
    return te, tr, st


def row_rewards(seed, E, T):
    """time-major float32 [T, E] in [-2, 2]"""
    import hashfill as hf
    return hf.hf_range(seed, (T * E,), -2, 2).reshape(T, E)
