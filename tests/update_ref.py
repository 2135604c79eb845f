"""The reference of aleppo_train's opt-in update features - ALEPPO_OPT_VALUE_CLIP and the approx-KL / clip-fraction
diagnostics, ALEPPO_OPT_KL_PENALTY, ALEPPO_OPT_ADV_NORM_MINIBATCH, and a given (shuffled) sample order - composed from the
CPU oracle's pieces (oracle_lib: net_forward, ppo_loss, net_backward, clip_grad_norm, adam_step); the oracle itself has
none of these modes.  A plain helper module (no fixtures), used by test_value_clip.py, test_kl_penalty.py,
test_adv_norm_minibatch.py and test_hyper_schedule.py.

Per minibatch it is orc.train's loop (oracle.c oracle_train_ex) step for step, and there is one copy of it
(composed_train); with every option off every number is orc.train's (test_value_clip.py and test_kl_penalty.py pin that
bit for bit).

Value clipping.  With `vold` given, the value term of the loss and its gradient are replaced by the clipped ones of
include/aleppo.h, computed in float64 with the same select:
    d = v - v_old;  v_c = |d| <= c ? v : v_old + copysign(c, d);  l_u = (v - R)^2,  l_c = (v_c - R)^2
    value loss = 0.5 max(l_u, l_c);  dL/dv = l_u >= l_c ? v - R : 0

The KL penalty (the exact KL(pi_old || pi) and the beta KL penalty of the PPO paper's section 4).  Per sample, from the
oracle's fp32 logits in float64 (include/aleppo.h):
    lp = orc.log_softmax(logits),  p = exp(lp),  q_a = exp(olp_a),  S = sum_a q_a,  KL = sum_a q_a (olp_a - lp_a)
    total loss += beta KL;   dlogits_j += (mask / mask_count) beta (p_j S - q_j)
With beta = 0 nothing is added.

Per-minibatch advantage normalisation.  Per minibatch, include/aleppo.h defines the statistics over the unmasked samples
in float64:
    n = count, S = sum a, Q = sum a^2   (a = the advantage as stored, widened to fp32 and then to float64)
    mean = S / n,  var = max(0, (Q - S*S/n) / max(n - 1, 1)),  std = sqrt(var)
    mean_f = (float)mean,  inv_f = (float)(1 / (std + 1e-8));   n = 0: mean_f = 0, inv_f = 1, std = 0
and every sample of the minibatch, masked or not, trains on (a - mean_f) * inv_f computed in fp32.  The statistics
depend only on a minibatch's sample set, so the update is the plain one on host-normalised advantages: for contiguous
minibatches the slices are the same in every epoch; for shuffled ones each epoch is gathered in the engine's order
(aleppo_read_sample_order), normalised per minibatch and trained as one epoch with the Adam state carried."""
import numpy as np

import oracle_lib as orc

PLANES = ("total_losses", "ratio", "entropies", "value_losses", "clipped", "approx_kl", "clip_fraction", "kl")
MEANS = ("loss", "grad_norm", "mean_approx_kl", "mean_clip_fraction", "mean_kl")


def value_branch(values, returns, vold, clip):
    """float64 (value_losses, dL/dv, zero_gradient_branch) of the clipped value term, per sample"""
    v, R, vo = (np.asarray(x, np.float64) for x in (values, returns, vold))
    c = float(np.float32(clip))
    d = v - vo
    vc = np.where(np.abs(d) <= c, v, vo + np.copysign(c, d))
    lu, lc = (v - R) ** 2, (vc - R) ** 2
    return 0.5 * np.maximum(lu, lc), np.where(lu >= lc, v - R, 0.0), lu < lc


def diagnostics(logits, old_lp, actions, ratio, clip):
    """per-sample approx-KL (float64, from the oracle's fp32 log-softmax) and clip fraction (from the fp32 ratio)"""
    lp = orc.log_softmax(logits).astype(np.float64)
    idx = np.arange(len(actions))
    logr = lp[idx, actions] - np.asarray(old_lp, np.float64)[idx, actions]
    rho = np.exp(logr)
    kl = (rho - 1.0) - logr
    cf = (np.abs(np.asarray(ratio, np.float64) - 1.0) > float(np.float32(clip))).astype(np.float64)
    return kl, cf


def exact_kl(logits, old_lp):
    """float64 per-sample (KL, S, p, q) from the oracle's fp32 log-softmax of `logits` and the old log-probs as given"""
    lp = orc.log_softmax(logits).astype(np.float64)
    olp = np.asarray(old_lp, np.float32).astype(np.float64)
    q = np.exp(olp)
    return np.sum(q * (olp - lp), axis=1), np.sum(q, axis=1), np.exp(lp), q


def kl_grad(logits, old_lp, masks, nm, beta):
    """float64 [B, A]: the KL penalty's contribution to dL/dlogits, (mask / nm) beta (p_j S - q_j)"""
    _, S, p, q = exact_kl(logits, old_lp)
    w = np.where(np.asarray(masks) != 0, float(np.float32(beta)) / float(nm), 0.0)
    return w[:, None] * (p * S[:, None] - q)


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


@np.errstate(divide="ignore", invalid="ignore")  # (a minibatch without unmasked samples: 0 / 0, like orc.train's)
def _contiguous_epochs(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold, beta, lr, clip, c_v, c_e,
                       max_norm, adam, emulate_bf16, sums):
    """the minibatch loop: `epochs` epochs over the M contiguous slices of the batch as given"""
    params = orc.cf(params).copy()
    obs = orc.c8(obs)
    N = obs.shape[0]
    B = N // M
    actions = np.ascontiguousarray(actions, np.int64)
    old_lp, adv, ret, masks = orc.cf(old_lp), orc.cf(adv), orc.cf(ret), orc.c8(masks)
    if adam is None:
        adam = dict(m=np.zeros_like(params), v=np.zeros_like(params), step=0)
    m_, v_, step = orc.cf(adam["m"]).copy(), orc.cf(adam["v"]).copy(), int(adam["step"])
    out = {k: np.zeros((epochs, M, B), np.float32) for k in PLANES}
    for k in MEANS:
        out[k] = np.zeros((epochs, M), np.float32)
    out["zero_branch"] = np.zeros((epochs, M), np.int64)
    b32 = float(np.float32(beta))
    g = None
    for ep in range(epochs):
        for k in range(M):
            s = slice(k * B, (k + 1) * B)
            logits, values, acts = orc.net_forward(params, H, A, obs[s], want_acts=True, emulate_bf16=emulate_bf16,
                                                   sums=sums)
            o = orc.ppo_loss(logits, old_lp[s], actions[s], adv[s], values, ret[s], masks[s], clip, c_v, c_e)
            mk = masks[s] != 0
            nm = np.float32(mk.sum())
            loss = o["loss"]
            if vold is not None:
                lv, dv, zero = value_branch(values, ret[s], vold[s], clip)
                lv32 = lv.astype(np.float32)
                o["value_losses"] = lv32
                o["total_losses"] = (-o["clipped"] + np.float32(c_v) * lv32 - np.float32(c_e) * o["entropies"]).astype(
                    np.float32)
                o["dvalues"] = np.where(mk, float(np.float32(c_v)) * dv / float(nm), 0.0).astype(np.float32)
                loss = np.float32(np.sum(o["total_losses"].astype(np.float64)[mk]) / float(nm))
                out["zero_branch"][ep, k] = int((zero & mk).sum())
            kl, _, _, _ = exact_kl(logits, old_lp[s])
            if b32 != 0.0:
                o["total_losses"] = (o["total_losses"].astype(np.float64) + b32 * kl).astype(np.float32)
                loss = np.float32(np.sum(o["total_losses"].astype(np.float64)[mk]) / float(nm))
                o["dlogits"] = (o["dlogits"].astype(np.float64) + kl_grad(logits, old_lp[s], masks[s], nm, beta)).astype(
                    np.float32)
            akl, cfr = diagnostics(logits, old_lp[s], actions[s], o["ratio"], clip)
            out["loss"][ep, k] = loss
            for p in ("total_losses", "ratio", "entropies", "value_losses", "clipped"):
                out[p][ep, k] = o[p]
            out["approx_kl"][ep, k] = akl
            out["clip_fraction"][ep, k] = cfr
            out["kl"][ep, k] = kl
            out["mean_approx_kl"][ep, k] = np.sum(akl[mk]) / float(nm)
            out["mean_clip_fraction"][ep, k] = np.sum(cfr[mk]) / float(nm)
            out["mean_kl"][ep, k] = np.sum(kl[mk]) / float(nm)
            g = orc.net_backward(params, H, A, acts, o["dlogits"], o["dvalues"], emulate_bf16=emulate_bf16, sums=sums)
            out["grad_norm"][ep, k], g = orc.clip_grad_norm(g, H, A, max_norm)
            step += 1
            params, m_, v_ = orc.adam_step(params, g, m_, v_, lr, step)
    out.update(params=params, last_grads=g, adam=dict(m=m_, v=v_, step=step))
    return out


def composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, *, vold=None, beta=0.0,
                   adv_norm=False, order=None, lr=2.5e-4, clip=0.1, c_v=0.5, c_e=0.01, max_norm=0.5, adam=None,
                   emulate_bf16=False, sums="double", floor=False):
    """orc.train's result dict (params, loss, grad_norm, the [epochs, M, B] planes, last_grads, adam) plus the approx_kl
    / clip_fraction / kl planes, their masked means mean_approx_kl / mean_clip_fraction / mean_kl [epochs, M], zero_branch
    (the masked samples that took the zero-gradient value branch, per minibatch) and, with adv_norm, adv_mean / adv_std
    [epochs, M] (float64).
    vold: value clipping at `clip`; beta: the KL penalty's coefficient; adv_norm: per-minibatch advantage normalisation on
    the host (normalise); order: the [epochs, N] sample order of a shuffled update (None: contiguous), run as one epoch
    per order with the Adam state carried; floor (bf16): result["floor_run"] = the same update with fp32 sums (what
    bf16_check.Checker bounds its checks with, as bf16_check.emulated_train)."""
    orders = [slice(None)] if order is None else [np.asarray(o) for o in order]
    reps = epochs if order is None else 1  # epochs per contiguous pass
    p, ad, parts, mean, std = orc.cf(params), adam, [], [], []
    for o in orders:
        a = np.asarray(adv, np.float32)[o]
        if adv_norm:
            a, mu, sd = normalise(a, np.asarray(masks)[o], M)
            mean.append(np.broadcast_to(mu, (reps, M)))
            std.append(np.broadcast_to(sd, (reps, M)))
        r = _contiguous_epochs(p, H, A, np.asarray(obs)[o], np.asarray(actions)[o], np.asarray(old_lp)[o], a,
                               np.asarray(ret)[o], np.asarray(masks)[o], reps, M,
                               None if vold is None else np.asarray(vold)[o], beta, lr, clip, c_v, c_e, max_norm, ad,
                               emulate_bf16, sums)
        p, ad = r["params"], r["adam"]
        parts.append(r)
    out = dict(parts[-1])  # (params, last_grads, adam: after the last epoch)
    for k in PLANES + MEANS + ("zero_branch",):  # the [epochs, M, ...] results, epoch by epoch
        out[k] = np.concatenate([q[k] for q in parts])
    if adv_norm:
        out["adv_mean"], out["adv_std"] = np.concatenate(mean), np.concatenate(std)
    if floor:
        out["floor_run"] = composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold=vold,
                                          beta=beta, adv_norm=adv_norm, order=order, lr=lr, clip=clip, c_v=c_v, c_e=c_e,
                                          max_norm=max_norm, adam=adam, emulate_bf16=emulate_bf16, sums="float32")
    return out
