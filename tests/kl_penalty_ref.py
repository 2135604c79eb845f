"""The reference of ALEPPO_OPT_KL_PENALTY (the exact KL(pi_old || pi) and the beta KL penalty of the PPO paper's section
4), composed from the CPU oracle's pieces - the oracle itself has no KL term.  A plain helper module (no fixtures), used by
test_kl_penalty.py.

Per minibatch it is value_clip_ref.composed_train's loop (orc.train step for step; with `vold` the clipped value term),
and, per sample, from the oracle's fp32 logits in float64 (include/aleppo.h):
    lp = orc.log_softmax(logits),  p = exp(lp),  q_a = exp(olp_a),  S = sum_a q_a,  KL = sum_a q_a (olp_a - lp_a)
    total loss += beta KL;   dlogits_j += (mask / mask_count) beta (p_j S - q_j)
With beta = 0 nothing is added: every number is orc.train's (tests/test_kl_penalty.py pins that bit for bit).
Advantages normalised per minibatch (ALEPPO_OPT_ADV_NORM_MINIBATCH) are normalised on the host first, as in
adv_norm_ref.py; a shuffled update runs one epoch per sample order with the Adam state carried."""
import numpy as np

import adv_norm_ref as ar
import oracle_lib as orc
import value_clip_ref as vr

PLANES = vr.PLANES + ("kl",)


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


def _one_order(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, beta, vold, lr, clip, c_v, c_e,
               max_norm, adam, emulate_bf16, sums):
    """value_clip_ref.composed_train's loop with the KL term: `epochs` epochs over contiguous slices"""
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
    for k in ("loss", "grad_norm", "mean_approx_kl", "mean_clip_fraction", "mean_kl"):
        out[k] = np.zeros((epochs, M), np.float32)
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
                lv, dv, _ = vr.value_branch(values, ret[s], vold[s], clip)
                lv32 = lv.astype(np.float32)
                o["value_losses"] = lv32
                o["total_losses"] = (-o["clipped"] + np.float32(c_v) * lv32 - np.float32(c_e) * o["entropies"]).astype(
                    np.float32)
                o["dvalues"] = np.where(mk, float(np.float32(c_v)) * dv / float(nm), 0.0).astype(np.float32)
                loss = np.float32(np.sum(o["total_losses"].astype(np.float64)[mk]) / float(nm))
            kl, _, _, _ = exact_kl(logits, old_lp[s])
            if b32 != 0.0:
                o["total_losses"] = (o["total_losses"].astype(np.float64) + b32 * kl).astype(np.float32)
                loss = np.float32(np.sum(o["total_losses"].astype(np.float64)[mk]) / float(nm))
                o["dlogits"] = (o["dlogits"].astype(np.float64) + kl_grad(logits, old_lp[s], masks[s], nm, beta)).astype(
                    np.float32)
            akl, cfr = vr.diagnostics(logits, old_lp[s], actions[s], o["ratio"], clip)
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


def composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, beta=0.0, order=None, adv_norm=False,
                   vold=None, lr=2.5e-4, clip=0.1, c_v=0.5, c_e=0.01, max_norm=0.5, adam=None, emulate_bf16=False,
                   floor=False):
    """the penalised update: orc.train's result dict plus the approx_kl / clip_fraction / kl planes and their masked
    means mean_approx_kl / mean_clip_fraction / mean_kl [epochs, M].  order: the [epochs, N] sample order of a shuffled
    update (None: contiguous); adv_norm: per-minibatch advantage normalisation on the host (adv_norm_ref.normalise);
    vold: value clipping at `clip`.  floor (bf16): result["floor_run"] = the same update with fp32 sums, as
    bf16_check.emulated_train."""
    N = np.asarray(obs).shape[0]
    orders = [np.arange(N)] if order is None else [np.asarray(o) for o in order]
    reps = epochs if order is None else 1  # epochs per contiguous pass
    out = {}
    for sums in (("double", "float32") if floor else ("double",)):
        p, ad, parts = orc.cf(params), adam, []
        for o in orders:
            a = np.asarray(adv, np.float32)[o]
            if adv_norm:
                a = ar.normalise(a, np.asarray(masks)[o], M)[0]
            r = _one_order(p, H, A, np.asarray(obs)[o], np.asarray(actions)[o], np.asarray(old_lp)[o], a,
                           np.asarray(ret)[o], np.asarray(masks)[o], reps, M, beta,
                           None if vold is None else np.asarray(vold)[o], lr, clip, c_v, c_e, max_norm, ad,
                           emulate_bf16, sums)
            p, ad = r["params"], r["adam"]
            parts.append(r)
        res = dict(parts[-1])
        for k, v in parts[0].items():
            if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[:2] == (reps, M):
                res[k] = np.concatenate([q[k] for q in parts])
        if sums == "double":
            out = res
        else:
            out["floor_run"] = res
    return out
