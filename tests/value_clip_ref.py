"""The reference of ALEPPO_OPT_VALUE_CLIP and of the approx-KL / clip-fraction diagnostics, composed from the CPU
oracle's pieces (oracle_lib: net_forward, ppo_loss, net_backward, clip_grad_norm, adam_step) - the oracle itself has no
value-clipping mode.  A plain helper module (no fixtures), used by test_value_clip.py.

Per minibatch it is orc.train's loop (oracle.c oracle_train_ex) step for step; with `vold` given, the value term of the
loss and its gradient are replaced by the clipped ones of include/aleppo.h, computed in float64 with the same select:
    d = v - v_old;  v_c = |d| <= c ? v : v_old + copysign(c, d);  l_u = (v - R)^2,  l_c = (v_c - R)^2
    value loss = 0.5 max(l_u, l_c);  dL/dv = l_u >= l_c ? v - R : 0
Without `vold` every number is orc.train's (tests/test_value_clip.py pins that bit for bit)."""
import numpy as np

import oracle_lib as orc

PLANES = ("total_losses", "ratio", "entropies", "value_losses", "clipped", "approx_kl", "clip_fraction")


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


def composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold=None, lr=2.5e-4, clip=0.1,
                   c_v=0.5, c_e=0.01, max_norm=0.5, adam=None, emulate_bf16=False, sums="double", floor=False):
    """orc.train's result dict (params, loss, grad_norm, the [epochs, M, B] planes, last_grads, adam) plus approx_kl /
    clip_fraction planes, their masked means mean_approx_kl / mean_clip_fraction [epochs, M] and zero_branch (the masked
    samples that took the zero-gradient branch, per minibatch).  floor: also run the same update with fp32 sums
    (result["floor_run"], what bf16_check.Checker bounds its checks with)."""
    params0 = orc.cf(params)
    params = params0.copy()
    obs = orc.c8(obs)
    N = obs.shape[0]
    B = N // M
    actions = np.ascontiguousarray(actions, np.int64)
    old_lp, adv, ret, masks = orc.cf(old_lp), orc.cf(adv), orc.cf(ret), orc.c8(masks)
    if adam is None:
        adam = dict(m=np.zeros_like(params), v=np.zeros_like(params), step=0)
    m_, v_, step = orc.cf(adam["m"]).copy(), orc.cf(adam["v"]).copy(), int(adam["step"])
    out = {k: np.zeros((epochs, M, B), np.float32) for k in PLANES}
    for k in ("loss", "grad_norm", "mean_approx_kl", "mean_clip_fraction"):
        out[k] = np.zeros((epochs, M), np.float32)
    out["zero_branch"] = np.zeros((epochs, M), np.int64)
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
            kl, cfr = diagnostics(logits, old_lp[s], actions[s], o["ratio"], clip)
            out["loss"][ep, k] = loss
            for p in ("total_losses", "ratio", "entropies", "value_losses", "clipped"):
                out[p][ep, k] = o[p]
            out["approx_kl"][ep, k] = kl
            out["clip_fraction"][ep, k] = cfr
            out["mean_approx_kl"][ep, k] = np.sum(kl[mk]) / float(nm)
            out["mean_clip_fraction"][ep, k] = np.sum(cfr[mk]) / float(nm)
            g = orc.net_backward(params, H, A, acts, o["dlogits"], o["dvalues"], emulate_bf16=emulate_bf16, sums=sums)
            out["grad_norm"][ep, k], g = orc.clip_grad_norm(g, H, A, max_norm)
            step += 1
            params, m_, v_ = orc.adam_step(params, g, m_, v_, lr, step)
    out.update(params=params, last_grads=g, adam=dict(m=m_, v=v_, step=step))
    if floor:
        out["floor_run"] = composed_train(params0, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold=vold,
                                          lr=lr, clip=clip, c_v=c_v, c_e=c_e, max_norm=max_norm, adam=adam,
                                          emulate_bf16=emulate_bf16, sums="float32")
    return out
