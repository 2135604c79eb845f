"""The reference of ALEPPO_OPT_ADV_NORM_MINIBATCH (per-minibatch advantage normalisation), composed from the CPU oracle's
pieces - the oracle itself has no such mode.  A plain helper module (no fixtures), used by test_adv_norm_minibatch.py.

Per minibatch, include/aleppo.h defines the statistics over the unmasked samples in float64:
    n = count, S = sum a, Q = sum a^2   (a = the advantage as stored, widened to fp32 and then to float64)
    mean = S / n,  var = max(0, (Q - S*S/n) / max(n - 1, 1)),  std = sqrt(var)
    mean_f = (float)mean,  inv_f = (float)(1 / (std + 1e-8));   n = 0: mean_f = 0, inv_f = 1, std = 0
and every sample of the minibatch, masked or not, trains on (a - mean_f) * inv_f computed in fp32.  The statistics
depend only on a minibatch's sample set, so the update is orc.train on host-normalised advantages: for contiguous
minibatches the slices are the same in every epoch (one orc.train call); for shuffled ones each epoch is gathered in the
engine's order (aleppo_read_sample_order), normalised per minibatch and trained as one epoch with the Adam state carried
(value_clip_ref.composed_train instead of orc.train with value clipping)."""
import numpy as np

import oracle_lib as orc
import value_clip_ref as vr


def stats(adv, masks):
    """(n, mean, std, mean_f, inv_f) of aleppo.h over the unmasked samples of one minibatch (float64; the last two fp32)"""
    a = np.asarray(adv, np.float32).astype(np.float64)[np.asarray(masks) != 0]
    n = a.size
    if n == 0:
        return 0, 0.0, 0.0, np.float32(0.0), np.float32(1.0)
    S, Q = float(np.sum(a)), float(np.sum(a * a))
    mean = S / n
    std = float(np.sqrt(max(0.0, (Q - S * S / n) / max(n - 1, 1))))
    return n, mean, std, np.float32(mean), np.float32(1.0 / (std + 1e-8))


def normalise64(adv, masks):
    """float64 (a - mean) / (std + 1e-8) of one minibatch with its float64 statistics (every sample)"""
    _, mean, std, _, _ = stats(adv, masks)
    return (np.asarray(adv, np.float32).astype(np.float64) - mean) / (std + 1e-8)


def normalise(adv, masks, M):
    """the advantages each of the M contiguous minibatches trains on: fp32 (a - mean_f) * inv_f, and the float64
    (mean, std) per minibatch [M]"""
    a = np.asarray(adv, np.float32).ravel()
    mk = np.asarray(masks).ravel()
    B = a.size // M
    out = np.empty_like(a)
    mean, std = np.zeros(M), np.zeros(M)
    for k in range(M):
        s = slice(k * B, (k + 1) * B)
        _, mean[k], std[k], mf, inv = stats(a[s], mk[s])
        out[s] = (a[s] - mf) * inv  # (fp32: the same two roundings as the device)
    return out, mean, std


def composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, order=None, vold=None,
                   emulate_bf16=False, floor=False, **kw):
    """the normalised update: orc.train's result dict (value_clip_ref.composed_train's with `vold`) plus adv_mean /
    adv_std [epochs, M] (float64).  order: the [epochs, N] sample order of a shuffled update (None: contiguous).
    floor (bf16): result["floor_run"] = the same update with fp32 sums, as bf16_check.emulated_train."""
    def run(p, o, a, ep, adam, sums):
        ob, ac, ol, re, mk = obs[o], actions[o], old_lp[o], ret[o], masks[o]
        if vold is not None:
            return vr.composed_train(p, H, A, ob, ac, ol, a, re, mk, ep, M, vold=vold[o], adam=adam,
                                     emulate_bf16=emulate_bf16, sums=sums, **kw)
        return orc.train(p, H, A, ob, ac, ol, a, re, mk, ep, M, adam=adam, emulate_bf16=emulate_bf16, sums=sums, **kw)

    N = np.asarray(obs).shape[0]
    orders = [np.arange(N)] if order is None else [np.asarray(o) for o in order]
    reps = epochs if order is None else 1  # epochs per oracle call
    out = {}
    for sums in (("double", "float32") if floor else ("double",)):
        p, adam, parts, mean, std = orc.cf(params), None, [], [], []
        for o in orders:
            a, mu, sd = normalise(np.asarray(adv, np.float32)[o], np.asarray(masks)[o], M)
            r = run(p, o, a, reps, adam, sums)
            p, adam = r["params"], r["adam"]
            parts.append(r)
            mean.append(np.broadcast_to(mu, (reps, M)))
            std.append(np.broadcast_to(sd, (reps, M)))
        res = dict(parts[-1])  # (params, last_grads, adam: after the last epoch)
        for k, v in parts[0].items():  # the [epochs, M, ...] results, epoch by epoch
            if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[:2] == (reps, M):
                res[k] = np.concatenate([q[k] for q in parts])
        res["adv_mean"], res["adv_std"] = np.concatenate(mean), np.concatenate(std)
        if sums == "double":
            out = res
        else:
            out["floor_run"] = res
    return out
