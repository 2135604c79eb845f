"""One layer of the backward pass, exactly: a float64 reference per stored gradient and the element-wise checks built on it.

A plain helper module (no fixtures) in the style of tests/layer_ref.py, whose im2col, Layer, interval, mismatches,
fp32_check, FLOOR_FACTOR and U it uses; shared by tests/test_backward_ref_cpu.py (the checker has room and teeth) and
tests/test_gpu_backward.py (the engine).  Every quantity starts from the stored tensors of whoever is being checked -
aleppo_export_backward's a1 / a2 / a3 / h / dh / dz3 / dz2 / dz1, all exact in float64 - and the fp32 master parameters
(conv and fc weights rounded with round_bf16 for the bf16 model: the rounding points are the table in oracle/oracle.h).
Nothing propagates: a legitimate one-ulp flip in dz3 is an INPUT of the conv3 checks, not an error of them.

Data gradients (dgrad).  X = fc, conv3, conv2 gives the stored gradient in front of it (dz3, dz2, dz1):
    z  = W_b^T dz_X          float64; for the convolutions by im2col of dz_X, dilated by the stride and padded by k - 1,
                             against the flipped kernels (one matmul per block of samples)
    Sa = |W_b|^T |dz_X|      the sum of the term magnitudes
    K                        the number of terms OF THAT ELEMENT: a border pixel has fewer (counted by the same im2col on
                             an indicator image), fc has H
    gate = a_(l-1) > 0       from the exported activation; exact, so behind a closed gate every element is exactly 0
and two float32 evaluations, "blas" and "chunks", as layer_ref.evaluate makes them.  Checks: bf16 contexts (a) every
element inside bf16(gate (z -+ eps)), eps = 2 K u Sa + 4 u |z|, signed, and (b) per input channel the count of elements
that differ from bf16(gate z), cap FLOOR_FACTOR x max(what the two float32 evaluations show, 2); fp32 contexts (c).

Weight and bias gradients (wgrad).
    dW_l[oc][k] = scale * sum over (sample, position) of dz_l a_(l-1)      scale = fp32(1/255) for conv1 (bytes), else 1
    db_l[oc]    = sum over (sample, position) of the SAME stored dz_l
in float64 (the im2col of a_(l-1) in blocks of samples), compared with aleppo_export_grads under a clip factor of exactly
1.  Check (c) on every element, K the number of (sample, position) terms, R the larger of the two float32 evaluations'
max |z32 - z| / (u Sa) - "blas" one float32 matmul over the axis, "chunks" float32 matmuls over layer_ref.CHUNK
consecutive rows added one after the other.  R is never taken from the engine.

The fused tail stores no dz1.  dW1 / db1 are then evaluated from dz1_ref = bf16(gate W2_b^T dz2), and their bound grows by
scale * sum (hi - lo) |x| over the terms whose interval (a) is not a single value: what legitimate flips inside the
kernel can move, and nothing more.

The head.  From the exported h, the fp32 Wh / bh and the minibatch's planes, in float64 (head_train_body.inc's formulas;
m = mask / N_mask, N_mask the minibatch's unmasked count):
    z = Wh h + bh;  lp = z - logsumexp(z);  p = exp(lp);  ent = -sum p lp;  rho = exp(lp[act] - old_lp[act])
    gs = -rho adv where the clip is inactive (adv >= 0: rho <= 1 + clip; adv < 0: rho >= 1 - clip), else 0
    g_a = m (gs ((a == act) - p_a) + c_e p_a (lp_a + ent))       g_v = m c_v (v - ret)
    dh = Wh^T g   (bf16: interval (a), K = A + 1)      dWh = sum_rows g h^T,  dbh = sum_rows g   (both (c))
The engine forms g in fp32 from ITS logits, so each check is widened by the linear image of an allowance delta on g:
|Wh|^T delta for dh, sum_rows |h| delta for dWh, sum_rows delta for dbh.  delta, per row (derived like adam_ref's bounds:
twice the plain count of roundings, on the term magnitudes, plus the input's own bound pushed through):
    E      the heads' forward bound of layer_ref (c) on that row's logits (E_l, the largest over the actions) and value
           (E_v): min(FLOOR_FACTOR R u Sa + 2 u |z|, 2 K u Sa + 4 u |z|)
    e_lp   = 2 (A + 5) u (max|z| + |lse| + 1): z - mx, exp, the A-term sum, log, mx + log, z - lse - A + 5 operations on
           magnitudes max|z| and |lse|; the 1 turns the relative error of the sum (1 <= se <= A) into an absolute one of
           its logarithm
    dl     = 2 E_l + e_lp                       |lp' - lp|: a logit moves by <= E_l, the logsumexp by <= E_l
    rp     = expm1(dl) + 2u                     relative error of p = exp(lp) (the exp itself: one operation)
    de     = rp ent + (1 + rp) dl + 2 (A + 1) u ent       |ent' - ent|, ent = sum p |lp|
    rr     = expm1(dl + 2u |log rho|) + 4u      relative error of rho (the subtraction, the exp), and of gs (the product)
    dgs    = |adv| rho rr, plus |adv| rho where rho is within rr rho of its clip boundary (the select may go either way)
    delta_a = m (dgs |(a == act) - p_a| + |gs| p_a rp + c_e p_a (rp |lp_a + ent| + (1 + rp) (dl + de)))
              + 18u m (|gs| |(a == act) - p_a| + c_e p_a |lp_a + ent|)
              nine operations from p, lp, ent and rho to g: (a == act) - p, -rho adv, the product, lp + ent, c_e p, the
              product, the sum, 1 / N_mask, the product with m
    delta_v = m c_v (E_v + 8u |v - ret|)        v - ret, c_v, 1 / N_mask, m: four operations
A masked row has m = 0: delta = 0, g = 0, and every stored gradient of that sample must be exactly 0.
restate_f32() is a float32 numpy restatement of the same formulas from float32 logits; tests/test_backward_ref_cpu.py
asserts that it stays within delta / FLOOR_FACTOR on every row's inputs.
head() and restate_f32() also take the kernel's options - value clipping, the KL penalty, per-minibatch advantage
normalisation - and an absolute term for probabilities below the smallest fp32 normal; tests/head_ref.py derives what each
adds to delta, and the per-sample planes and means with their bounds.  With every option off nothing above changes."""
import hashlib

import numpy as np

import layer_ref as lr
from layer_ref import FLOOR_FACTOR, U, fp32_check, im2col, interval, mismatches  # noqa: F401

SCALE1 = lr.SCALE1
BLOCK = 16  # samples per im2col block
# X: (the layer whose weights it uses, the stored gradient it reads, the one it produces, the activation that gates)
DGRAD = dict(fc=("fc", "dfc", "dconv3", "conv3"), conv3=("conv3", "dconv3", "dconv2", "conv2"),
             conv2=("conv2", "dconv2", "dconv1", "conv1"))
# layer: (its stored gradient, its stored input)
WGRAD = dict(fc=("dfc", "conv3"), conv3=("dconv3", "conv2"), conv2=("dconv2", "conv1"), conv1=("dconv1", "obs"))


class GateLayer(lr.Layer):
    """a data gradient: lr.Layer with act(z) = gate * z, K per element, and `extra` added to eps (the head's delta)"""

    def __init__(self, name, K, gate, z, Sa, z32, extra=0.0):
        super().__init__(name, K, False, z, Sa, z32)
        self.gate, self.extra = gate, extra

    def act(self, z):
        return np.where(self.gate, z, 0.0)

    def eps(self):
        return super().eps() + self.extra


def _f32_pair(cols32, wt32):
    """the two float32 evaluations of cols @ wt: one matmul, and CHUNK consecutive k at a time added in float32"""
    blas = cols32 @ wt32
    acc = np.zeros_like(blas)
    for k0 in range(0, cols32.shape[1], lr.CHUNK):
        acc += cols32[:, k0:k0 + lr.CHUNK] @ wt32[k0:k0 + lr.CHUNK]
    return blas, acc


def _dilate(dz, k, stride):
    """[n, OC, OH, OW] -> the image a stride-1 k x k convolution with the flipped kernels turns into the input gradient"""
    n, OC, OH, OW = dz.shape
    out = np.zeros((n, OC, (OH - 1) * stride + 1 + 2 * (k - 1), (OW - 1) * stride + 1 + 2 * (k - 1)), dz.dtype)
    out[:, :, k - 1:k - 1 + (OH - 1) * stride + 1:stride, k - 1:k - 1 + (OW - 1) * stride + 1:stride] = dz
    return out


def dgrad(X, dz, w, act):
    """the data gradient in front of layer X ("fc", "conv3", "conv2"): dz its stored gradient ([n, H] or [n, OC, OH, OW]),
    w its weights [rows, K] as layer_ref.split_params gives them, act the stored activation that gates ([n, C, IH, IW])"""
    dz, w = np.asarray(dz), np.asarray(w, np.float32)
    gate = np.asarray(act) > 0
    n = dz.shape[0]
    if X == "fc":
        wd = np.ascontiguousarray(w.T)  # [3136, H]
        cols_of = lambda s: np.ascontiguousarray(dz[s], dtype=np.float64)
        shape = lambda m: m.reshape((m.shape[0],) + gate.shape[1:])
        K = w.shape[0]
    else:
        cin, k, stride, oc = lr.CONV[X]
        wd = np.ascontiguousarray(w.reshape(oc, cin, k, k)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)).reshape(cin, oc * k * k)
        cols_of = lambda s: im2col(_dilate(dz[s], k, stride), k, 1, np.float64)[0]
        IH, IW = gate.shape[2:]
        shape = lambda m: np.ascontiguousarray(m.reshape(-1, IH, IW, cin).transpose(0, 3, 1, 2))
        ones = np.ones((1, 1) + dz.shape[2:])
        K = oc * im2col(_dilate(ones, k, stride), k, 1, np.float64)[0].sum(axis=1).reshape(1, 1, IH, IW)
    wt64 = np.ascontiguousarray(wd.T.astype(np.float64))
    wt32 = np.ascontiguousarray(wd.T)
    z, Sa, b32, c32 = [], [], [], []
    for n0 in range(0, n, BLOCK):
        cols = cols_of(slice(n0, n0 + BLOCK))
        cols32 = cols.astype(np.float32)
        assert np.array_equal(cols32.astype(np.float64), cols)  # (bf16 or fp32 values: exact)
        z.append(shape(cols @ wt64))
        Sa.append(shape(np.abs(cols) @ np.abs(wt64)))
        blas, chunks = _f32_pair(cols32, wt32)
        b32.append(shape(blas))
        c32.append(shape(chunks))
    cat = np.concatenate
    return GateLayer("d" + DGRAD[X][3], K, gate, cat(z), cat(Sa), dict(blas=cat(b32), chunks=cat(c32)))


def _rows_of(layer, x, s):
    """the im2col rows of samples s of the stored input x of `layer`, float32 (exact)"""
    if layer == "fc":
        return np.ascontiguousarray(x[s], dtype=np.float32).reshape(len(x[s]), -1)
    _, k, stride, _ = lr.CONV[layer]
    return im2col(x[s], k, stride, np.float32)[0]


def _dz_rows(layer, dz, s):
    """[samples * positions, OC] of the stored gradient, rows in im2col's order"""
    d = np.asarray(dz[s])
    return d if layer == "fc" else np.ascontiguousarray(d.reshape(d.shape[0], d.shape[1], -1).transpose(0, 2, 1)).reshape(-1, d.shape[1])


def wgrad(layer, dz, x, spread=None):
    """(dW, db) as lr.Layer: the weight and bias gradient of `layer` from its stored gradient dz and its stored input x (the
    bytes for conv1).  spread ([like dz], >= 0): also extra = scale * spread^T |x| and sum spread, kept as .extra"""
    dz, x = np.asarray(dz), np.asarray(x)
    n = dz.shape[0]
    scale = SCALE1 if layer == "conv1" else 1.0
    s32 = np.float32(scale)
    acc = None
    for n0 in range(0, n, BLOCK):
        s = slice(n0, n0 + BLOCK)
        cols32, d32 = _rows_of(layer, x, s), np.ascontiguousarray(_dz_rows(layer, dz, s), dtype=np.float32)
        cols, d = cols32.astype(np.float64), d32.astype(np.float64)
        assert np.array_equal(d, _dz_rows(layer, dz, s))
        part = dict(z=d.T @ cols, Sa=np.abs(d).T @ np.abs(cols), bz=d.sum(axis=0), bSa=np.abs(d).sum(axis=0),
                    blas=d32.T @ cols32, bblas=d32.sum(axis=0, dtype=np.float32), rows=d.shape[0])
        ch, bch = np.zeros_like(part["blas"]), np.zeros_like(part["bblas"])
        for r0 in range(0, d32.shape[0], lr.CHUNK):
            ch += d32[r0:r0 + lr.CHUNK].T @ cols32[r0:r0 + lr.CHUNK]
            bch += d32[r0:r0 + lr.CHUNK].sum(axis=0, dtype=np.float32)
        part.update(chunks=ch, bchunks=bch)
        if spread is not None:
            sp = _dz_rows(layer, np.asarray(spread, np.float64), s)
            part.update(extra=sp.T @ np.abs(cols), bextra=sp.sum(axis=0))
        if acc is None:
            acc = part
        else:  # (float64 keys add in float64; the float32 evaluations add their blocks in float32, one after the other)
            for key in part:
                acc[key] = acc[key] + part[key]
    W = lr.Layer(layer + ".w", acc["rows"], False, acc["z"] * scale, acc["Sa"] * scale,
                 dict(blas=acc["blas"] * s32, chunks=acc["chunks"] * s32))
    b = lr.Layer(layer + ".b", acc["rows"], False, acc["bz"], acc["bSa"], dict(blas=acc["bblas"], chunks=acc["bchunks"]))
    W.extra = acc["extra"] * scale if spread is not None else 0.0
    b.extra = acc["bextra"] if spread is not None else 0.0
    return W, b


def measured_R(ref):
    """the larger max |z32 - z| / (u Sa) of the two float32 evaluations; kept as fp32_check's R"""
    return ref.memo("R", lambda: max(lr.measured_ratio(ref, ref.z32[o]) for o in ref.z32))


def bound_check(ref, got, extra=0.0):
    """check (c) with R of both float32 evaluations and `extra` more room per element"""
    measured_R(ref)
    return fp32_check(ref, np.asarray(got, np.float64).reshape(ref.z.shape), extra)


# ------------------------------------------------------------------ the head
class Head:
    """what head() returns: the float64 quantities per row, g [B, A + 1] (the value last), delta [B, A + 1], and the Layers
    dh (GateLayer, gate all open, extra = |Wh|^T delta), dW [A + 1, H], db [A + 1] with their .extra"""


def _logits_bound(h, wh, bh):
    """the heads' forward bound of layer_ref (c) per element [B, A + 1], and the exact logits"""
    ref = lr.evaluate("heads", h, wh, bh)
    return lr.fp32_bound(ref)[0], ref


def head(h, wh, bh, batch, hyper, n_mask, *, vold=None, beta=None, advs=None, exact_logits=False):
    """h [B, H] as exported; wh [A + 1, H], bh [A + 1] fp32 (layer_ref.split_params "heads"); batch: dict(actions [B],
    old_lp [B, A], adv [B], ret [B], masks [B]) of the minibatch's samples; hyper: dict(clip, c_v, c_e[, vclip]); n_mask:
    the minibatch's unmasked count.  The options of tests/head_ref.py, whose docstring derives what they add to delta
    (every default leaves each number as it was, bit for bit): vold [B]: the value-clip select against these old values
    at hyper["vclip"] (default: clip); beta: the exact KL and, where beta != 0, its gradient (None: the option off);
    advs = (mean_f, inv_f): the advantage is fp32((a - mean_f) * inv_f); exact_logits: E = 0 (the identity head of the
    stateless operator)"""
    h = np.asarray(h, np.float32)
    wh, bh = np.asarray(wh, np.float32), np.asarray(bh, np.float32)
    B, A = h.shape[0], wh.shape[0] - 1
    clip, c_v, c_e = (float(np.float32(hyper[k])) for k in ("clip", "c_v", "c_e"))
    E, fwd = _logits_bound(h, wh, bh)  # (R of the "blas" evaluation alone, as the forward check of the heads has it)
    if exact_logits:
        E = np.zeros_like(E)
    z, v = fwd.z[:, :A], fwd.z[:, A]
    act = np.asarray(batch["actions"], np.int64)
    olp = np.asarray(batch["old_lp"], np.float32).astype(np.float64)
    adv, ret = (np.asarray(batch[k], np.float32).astype(np.float64) for k in ("adv", "ret"))
    e_adv = None
    if advs is not None:  # head_ref: "Advantage normalisation"
        mean_f, inv_f = np.float32(advs[0]), np.float32(advs[1])
        a32 = np.asarray(batch["adv"], np.float32)
        adv = ((a32 - mean_f) * inv_f).astype(np.float64)
        e_adv = (float(inv_f) * float(np.spacing(np.abs(mean_f))) + np.abs(a32.astype(np.float64) - float(mean_f)) * float(
            np.spacing(np.abs(inv_f)))) * (1 + 4 * U) + 4 * U * np.abs(adv)
    m = np.where(np.asarray(batch["masks"]) != 0, float(np.float32(1.0) / np.float32(n_mask)), 0.0)
    idx = np.arange(B)
    mx = z.max(axis=1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    lp = z - lse[:, None]
    p = np.exp(lp)
    ent = -(p * lp).sum(axis=1)
    logr = lp[idx, act] - olp[idx, act]
    rho = np.exp(logr)
    active = np.where(adv >= 0, rho <= 1 + clip, rho >= 1 - clip)
    gs = np.where(active, -rho * adv, 0.0)
    onehot = np.zeros((B, A))
    onehot[idx, act] = 1.0
    t2 = c_e * p * np.abs(lp + ent[:, None])
    g_a = m[:, None] * (gs[:, None] * (onehot - p) + c_e * p * (lp + ent[:, None]))
    dv = v - ret
    o = Head()
    if vold is None:
        dvg = dv
    else:  # head_ref: "Value clipping"
        c = float(np.float32(hyper.get("vclip", hyper["clip"])))
        vo = np.asarray(vold, np.float32).astype(np.float64)
        d = v - vo
        vc = np.where(np.abs(d) <= c, v, vo + np.copysign(c, d))
        dc = vc - ret
        lu, lc = dv * dv, dc * dc
        dvg = np.where(lu >= lc, dv, 0.0)
        o.vclip = dict(c=c, vo=vo, d=d, vc=vc, dc=dc, lu=lu, lc=lc, zero=lu < lc)
    # the underflow term (head_ref: "Underflow"): 2^-126 on the rows where some p (or q) is below 2^-100, else 0
    q = np.exp(olp) if beta is not None else None
    small = p.min(axis=1) < 2.0 ** -100 if A else np.zeros(B, bool)
    if q is not None and A:
        small = small | (q.min(axis=1) < 2.0 ** -100)
    T = np.where(small, 2.0 ** -126, 0.0)
    b64 = 0.0 if beta is None else float(np.float32(beta))
    if q is not None:
        S = q.sum(axis=1)
        kl = (q * (olp - lp)).sum(axis=1)
        if b64 != 0.0:
            g_a = g_a + m[:, None] * b64 * (p * S[:, None] - q)
    g = np.concatenate([g_a, (m * c_v * dvg)[:, None]], axis=1)
    # delta (the module's docstring)
    E_l, E_v = E[:, :A].max(axis=1), E[:, A]
    e_lp = 2 * (A + 5) * U * (np.abs(z).max(axis=1) + np.abs(lse) + 1)
    dl = 2 * E_l + e_lp
    if T.any():
        dl = dl + A * T
    rp = np.expm1(dl) + 2 * U
    de = rp * ent + (1 + rp) * dl + 2 * (A + 1) * U * ent
    if T.any():
        de = de + T * np.abs(lp).sum(axis=1)
    rr = np.expm1(dl + 2 * U * np.abs(logr)) + 4 * U
    edge = np.where(adv >= 0, 1 + clip, 1 - clip)
    near = np.abs(rho - edge) <= rr * rho
    dgs = np.abs(adv) * rho * (rr + near)
    # (where the select went the other way |gs| may be |adv| rho instead of 0: dgs covers the difference, and the terms
    # proportional to |gs| below use the larger of the two)
    gs_hi = np.maximum(np.abs(gs), np.where(near, np.abs(adv) * rho, 0.0))
    if e_adv is not None:
        flip = np.abs(adv) <= e_adv  # the device's advantage may have the other sign: it reads the other edge
        near = near | flip
        dgs = dgs + rho * e_adv * (1 + rr) + np.where(flip, rho * np.abs(adv), 0.0)
        gs_hi = np.maximum(gs_hi, np.where(flip, rho * np.abs(adv), 0.0)) + rho * e_adv
    t1_hi = gs_hi[:, None] * np.abs(onehot - p)
    delta_a = m[:, None] * (dgs[:, None] * np.abs(onehot - p) + gs_hi[:, None] * p * rp[:, None]
                            + c_e * p * (rp[:, None] * np.abs(lp + ent[:, None]) + (1 + rp[:, None]) * (dl + de)[:, None])) \
        + 18 * U * m[:, None] * (t1_hi + t2)
    if T.any():
        delta_a = delta_a + m[:, None] * T[:, None] * (gs_hi[:, None] + c_e * (np.abs(lp + ent[:, None]) + (dl + de)[:, None]))
    if q is not None:
        dS = 2 * (A + 1) * U * S + A * T
        o.kl = dict(q=q, S=S, kl=kl, dS=dS, beta=b64)
        if b64 != 0.0:
            delta_a = delta_a + m[:, None] * b64 * (
                p * (rp * S + (1 + rp) * dS)[:, None] + 2 * U * q + T[:, None] * (S + dS + 1)[:, None]
                + 12 * U * (p * S[:, None] + q)) + 2 * U * m[:, None] * (t1_hi + t2)
    delta_v = m * c_v * (E_v + 8 * U * np.abs(dv))
    if vold is not None:
        w = o.vclip
        e_d = E_v + 2 * U * (np.abs(v) + np.abs(w["vo"]))
        e_dv = E_v + 2 * U * np.abs(dv)
        e_dc = 2 * U * (np.abs(w["vc"]) + np.abs(dc))  # (outside the range v_c does not depend on v)
        err = (2 * np.abs(dv) * e_dv + e_dv ** 2 + 2 * U * lu) + (2 * np.abs(dc) * e_dc + e_dc ** 2 + 2 * U * lc)
        outside = np.abs(d) > c
        w["ambiguous"] = (np.abs(np.abs(d) - c) <= e_d) | (outside & (np.abs(lu - lc) <= err))
        w["e_vc"] = E_v + 2 * U * (np.abs(v) + np.abs(w["vo"]) + c)
        delta_v = delta_v + np.where(w["ambiguous"], m * c_v * (np.abs(dv) + E_v), 0.0)
    delta = np.concatenate([delta_a, delta_v[:, None]], axis=1)
    o.fwd, o.z, o.v, o.lp, o.p, o.ent, o.rho, o.g, o.delta, o.m = fwd, z, v, lp, p, ent, rho, g, delta, m
    # (what tests/head_ref.py builds the per-sample planes and their bounds from)
    o.A, o.act, o.olp, o.adv, o.ret, o.lse, o.logr = A, act, olp, adv, ret, lse, logr
    o.active, o.near, o.e_adv, o.T = active, near, e_adv, T
    o.E_l, o.E_v, o.e_lp, o.dl, o.rp, o.de, o.rr = E_l, E_v, e_lp, dl, rp, de, rr
    o.hyper = dict(clip=clip, c_v=c_v, c_e=c_e)
    # dh = Wh^T g: g is not an fp32 value, so the float32 evaluations start from its float32 rounding (their own error)
    w64 = wh.astype(np.float64)
    g32 = g.astype(np.float32)
    blas, chunks = _f32_pair(g32, wh)
    o.dh = GateLayer("dfc", A + 1, np.ones((B, wh.shape[1]), bool), g @ w64, np.abs(g) @ np.abs(w64),
                     dict(blas=blas, chunks=chunks), extra=delta @ np.abs(w64))
    h64 = h.astype(np.float64)
    ch, bch = np.zeros((A + 1, h.shape[1]), np.float32), np.zeros(A + 1, np.float32)
    for r0 in range(0, B, lr.CHUNK):
        ch += g32[r0:r0 + lr.CHUNK].T @ h[r0:r0 + lr.CHUNK]
        bch += g32[r0:r0 + lr.CHUNK].sum(axis=0, dtype=np.float32)
    o.dW = lr.Layer("heads.w", B, False, g.T @ h64, np.abs(g).T @ np.abs(h64), dict(blas=g32.T @ h, chunks=ch))
    o.db = lr.Layer("heads.b", B, False, g.sum(axis=0), np.abs(g).sum(axis=0),
                    dict(blas=g32.sum(axis=0, dtype=np.float32), chunks=bch))
    # (the float32 evaluations read float32(g): half an ulp of every term belongs to their error, not to the sum's)
    o.dW.extra = delta.T @ np.abs(h64) + U * o.dW.Sa
    o.db.extra = delta.sum(axis=0) + U * o.db.Sa
    return o


def restate_f32(h, wh, bh, batch, hyper, n_mask, *, vold=None, beta=None, advs=None, flush=False, planes=False, z32=None):
    """g [B, A + 1] as a float32 numpy restatement of head_train_body.inc forms it, from layer_ref's float32 logits ("blas").
    vold / beta / advs: head()'s options; flush: every exp result below the smallest fp32 normal becomes 0 (default:
    numpy's gradual underflow); planes: return (g, {plane: float32 [B]}) - the eight per-sample planes in the engine's
    names; z32 [B, A + 1]: these float32 logits and values instead"""
    f = np.float32
    h, wh, bh = np.asarray(h, f), np.asarray(wh, f), np.asarray(bh, f)
    B, A = h.shape[0], wh.shape[0] - 1
    clip, c_v, c_e = (f(hyper[k]) for k in ("clip", "c_v", "c_e"))
    # (the float32 evaluation E's floor is measured on)
    zz = lr.evaluate("heads", h, wh, bh).z32["blas"] if z32 is None else np.asarray(z32, f)
    z, v = zz[:, :A], zz[:, A]
    act = np.asarray(batch["actions"], np.int64)
    olp, adv, ret = (np.asarray(batch[k], f) for k in ("old_lp", "adv", "ret"))
    if advs is not None:
        adv = (adv - f(advs[0])) * f(advs[1])
    if flush:
        def exp(x):
            with np.errstate(under="ignore"):
                r = np.exp(x)
            return np.where(r < f(2.0 ** -126), f(0), r).astype(f)
    else:
        def exp(x):
            with np.errstate(under="ignore"):
                return np.exp(x)
    m = np.where(np.asarray(batch["masks"]) != 0, f(1.0) / f(n_mask), f(0.0)).astype(f)
    idx = np.arange(B)
    mx = z.max(axis=1)
    se = np.zeros(B, f)
    for a in range(A):
        se = se + exp(z[:, a] - mx)
    lse = mx + np.log(se)
    lp = z - lse[:, None]
    p = exp(lp)
    ent = np.zeros(B, f)
    for a in range(A):
        ent = ent + p[:, a] * lp[:, a]
    ent = -ent
    logr = lp[idx, act] - olp[idx, act]
    rho = exp(logr)
    active = np.where(adv >= 0, rho <= f(1) + clip, rho >= f(1) - clip)
    gs = np.where(active, -rho * adv, f(0)).astype(f)
    onehot = np.zeros((B, A), f)
    onehot[idx, act] = 1
    ga = m[:, None] * (gs[:, None] * (onehot - p) + c_e * p * (lp + ent[:, None]))
    dv = v - ret
    if vold is None:
        lv, dvg = f(0.5) * (dv * dv), dv
    else:
        c = f(hyper.get("vclip", hyper["clip"]))
        vo = np.asarray(vold, f)
        d = v - vo
        vc = np.where(np.abs(d) <= c, v, vo + np.copysign(c, d)).astype(f)
        dc = vc - ret
        lu, lc = dv * dv, dc * dc
        lv, dvg = f(0.5) * np.maximum(lu, lc), np.where(lu >= lc, dv, f(0)).astype(f)
    kl = np.zeros(B, f)
    if beta is not None:
        S = np.zeros(B, f)
        for a in range(A):
            q = exp(olp[:, a])
            S = S + q
            kl = kl + q * (olp[:, a] - lp[:, a])
        if f(beta) != 0:
            ga = ga + (m * f(beta))[:, None] * (p * S[:, None] - exp(olp))
    gv = m * c_v * dvg
    out = np.concatenate([ga, gv[:, None]], axis=1)
    assert out.dtype == f
    if not planes:
        return out
    crho = np.minimum(np.maximum(rho, f(1) - clip), f(1) + clip)
    obj = np.minimum(rho * adv, crho * adv)
    total = -obj + c_v * lv - c_e * ent
    if beta is not None and f(beta) != 0:
        total = total + f(beta) * kl
    pl = dict(total_losses=total, clipped_losses=obj, value_losses=lv, entropies=ent, ratio=rho,
              approx_kl=(rho - f(1)) - logr, clip_fraction=(np.abs(rho - f(1)) > clip).astype(f), kl=kl)
    assert all(x.dtype == f for x in pl.values())
    return out, pl


# ------------------------------------------------------------------ a whole export
def _key(*arrays):
    hsh = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        hsh.update(str((a.dtype.str, a.shape)).encode())
        hsh.update(a.view(np.uint8).reshape(-1))
    return hsh.digest()


def split_grads(grads, H, A):
    """{layer: (dW [rows, K], db [rows])} of a flat gradient in the reference's order, the heads as one layer"""
    return lr.split_params(grads, H, A, False)


def masked_rows(exp, masks):
    """the stored gradients that are not exactly zero on a masked sample: [(name, sample)]"""
    bad = []
    for name in ("dfc", "dconv3", "dconv2", "dconv1"):
        if name in exp:
            d = np.asarray(exp[name])
            for s in np.flatnonzero(np.asarray(masks) == 0):
                if d[s].any():
                    bad.append((name, int(s)))
    return bad


def check_backward(params, H, A, bf16, obs, batch, hyper, n_mask, exp, grads, cache=None, only=None, head_opts=None):
    """every stored gradient of an export `exp` (aleppo_export_backward's dict, "dconv1" absent on the fused tail) and every
    tensor of `grads` (aleppo_export_grads of the same minibatch, clip factor 1) on the export's own inputs.  obs / batch:
    the minibatch's samples in its order.  only: the check names to run (default all).  cache: a dict kept for ONE set of
    parameters, one precision and one batch - a reference whose inputs have the same bytes is not evaluated again.
    head_opts: head()'s keyword options (tests/head_ref.py; None: all off).
    Returns (failures, report, results): failures a list of strings that begin with the check's name, report {check:
    text}, results {check: dicts / Layers}.  Check names: "head", "d<activation>" for the data gradients, "<layer>.w/.b"."""
    p = lr.split_params(params, H, A, bf16)
    G = split_grads(grads, H, A) if grads is not None else None
    cache = {} if cache is None else cache
    failures, report, results = [], {}, {}
    want = lambda name: only is None or name in only

    def memo(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    def first(v):
        return tuple(int(i) for i in v[0])

    def check_c(name, ref, got, extra):
        c = bound_check(ref, got, extra)
        results[name] = dict(ref=ref, c=c)
        report[name] = "(c) max |d| / (u Sa) %.3g against R %.3g, worst |d| / bound %.3g" % (c["ratio"], c["R"], c["worst"])
        if len(c["violations"]):
            i = first(c["violations"])
            failures.append("%s (c): %d elements outside the bound, first %s: got %r, z %r, Sa %r, R %.3g" % (
                name, len(c["violations"]), i, float(np.asarray(got).reshape(ref.z.shape)[i]), float(ref.z[i]),
                float(ref.Sa[i]), c["R"]))

    def check_a(name, ref, got, count):
        got = np.asarray(got, np.float32)
        lo, hi = interval(ref)
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(~((lo <= got) & (got <= hi)))
        leak = int(((got != 0) & ~ref.gate).sum())
        res = dict(ref=ref, violations=bad, single=float((lo == hi).mean()), leak=leak)
        text = "(a) %d outside, single %.3f, %d non-zero behind a closed gate" % (len(bad), res["single"], leak)
        if len(bad):
            i = first(bad)
            failures.append("%s (a): %d elements outside their interval, first %s: got %r, z %r, eps %r" % (
                name, len(bad), i, float(got[i]), float(ref.z[i]), float(np.broadcast_to(ref.eps(), ref.z.shape)[i])))
        if count:
            b = lr.mismatch_check(ref, got)
            res["b"] = b
            text += "; (b) worst channel %d/%d (floor %d)" % (b["counts"].max(), b["cap"], b["floor"])
            if len(b["failures"]):
                failures.append("%s (b): channels %s have %s mismatches, cap %d" % (
                    name, b["failures"][:8].tolist(), b["counts"][b["failures"]][:8].tolist(), b["cap"]))
        results[name], report[name] = res, text

    # the head: dh, dWh, dbh
    if want("head"):
        hopts = dict(head_opts or {})
        okey = tuple((k, None if x is None else _key(np.asarray(x, np.float64))) for k, x in sorted(hopts.items()))
        hd = memo(("head", _key(exp["fc"])) + ((okey, repr(sorted(hyper.items()))) if hopts else ()),
                  lambda: head(exp["fc"], *p["heads"], batch, hyper, n_mask, **hopts))
        results["head"] = dict(head=hd)
        if bf16:
            check_a("dfc", hd.dh, exp["dfc"], False)
        else:
            check_c("dfc", hd.dh, exp["dfc"], hd.dh.extra)
        if G is not None:
            check_c("heads.w", hd.dW, G["heads"][0], hd.dW.extra)
            check_c("heads.b", hd.db, G["heads"][1], hd.db.extra)
    # the data gradients
    for X, (wl, src, dst, gate) in DGRAD.items():
        if dst not in exp or not want(dst):
            continue
        ref = memo((dst, _key(exp[src], exp[gate])), lambda: dgrad(X, exp[src], p[wl][0], exp[gate]))
        if bf16:
            check_a(dst, ref, exp[dst], True)
        else:
            check_c(dst, ref, exp[dst], 0.0)
    # the weight and bias gradients
    src = dict(exp, obs=np.asarray(obs))
    for layer, (dzn, xn) in WGRAD.items():
        if G is None or not (want(layer + ".w") or want(layer + ".b")):
            continue
        if dzn in exp:
            W, b = memo((layer, _key(exp[dzn], src[xn])), lambda: wgrad(layer, exp[dzn], src[xn]))
        else:  # the fused tail: dz1 never reached memory
            assert layer == "conv1" and bf16
            r1 = memo(("dconv1", _key(exp["dconv2"], exp["conv1"])),
                      lambda: dgrad("conv2", exp["dconv2"], p["conv2"][0], exp["conv1"]))
            lo, hi = interval(r1)
            W, b = memo(("conv1 fused", _key(exp["dconv2"], exp["conv1"], src["obs"])),
                        lambda: wgrad("conv1", r1.exact_bf16(), src["obs"], spread=np.abs(hi.astype(np.float64) - lo)))
            results["dconv1 (not stored)"] = dict(ref=r1, single=float((lo == hi).mean()))
        if want(layer + ".w"):
            check_c(layer + ".w", W, G[layer][0], W.extra)
        if want(layer + ".b"):
            check_c(layer + ".b", b, G[layer][1], b.extra)
    for name, s in masked_rows(exp, batch["masks"]):
        failures.append("masked: sample %d is masked and its stored %s is not exactly zero" % (s, name))
    return failures, report, results


def summary(title, report):
    return title + "".join("\n    %-8s %s" % (l, t) for l, t in report.items())


def row_summary(title, runs):
    """one line per check over the routes of a row (runs: the results dicts of check_backward): the smallest share of
    single-valued intervals and the worst mismatch count against its cap, or the worst |d| / bound"""
    lines = []
    names = [n for n in ("dfc", "heads.w", "heads.b", "dconv3", "fc.w", "fc.b", "dconv2", "conv3.w", "conv3.b", "dconv1",
                         "conv2.w", "conv2.b", "conv1.w", "conv1.b") if any(n in r for r in runs)]
    for name in names:
        rs = [r[name] for r in runs if name in r]
        if "c" in rs[0]:
            lines.append("%-8s worst |d| / bound %.3g" % (name, max(r["c"]["worst"] for r in rs)))
        else:
            text = "%-8s single >= %.3f" % (name, min(r["single"] for r in rs))
            if "b" in rs[0]:
                w = max(rs, key=lambda r: r["b"]["counts"].max() / r["b"]["cap"])["b"]
                text += ", worst channel %d/%d (floor %d), %d mismatches of %d elements" % (
                    w["counts"].max(), w["cap"], w["floor"], max(int(r["b"]["counts"].sum()) for r in rs), rs[0]["ref"].z.size)
            lines.append(text)
    return "%s, %d route(s):" % (title, len(runs)) + "".join("\n    " + l for l in lines)
