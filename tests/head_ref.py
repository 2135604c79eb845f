"""The PPO head kernel in every variant: the options of backward_ref.head, the eight per-sample planes and the four means,
each with a bound that follows from the arithmetic.

A plain helper module (no fixtures) in the style of tests/backward_ref.py, whose head() results, U and
FLOOR_FACTOR it uses; shared by tests/test_head_ref_cpu.py (room and teeth) and tests/test_gpu_head.py (the stateless
operator and the engine).  Everything is float64 from the SAME z = Wh h + bh of backward_ref.head, on the exported h, and
every bound is built from the quantities its delta already defines - E_l, E_v (the forward bound of the logits and the
value), e_lp, dl (|lp' - lp|), rp (the relative error of p), de (|ent' - ent|), rr (the relative error of rho) - by the
rule of that docstring: twice the plain count of fp32 operations, on the term magnitudes, plus the input's bound pushed
through.  u = 2^-24.  A primed quantity is the device's.

The options (head_train_body.inc; include/aleppo.h)

Value clipping (VCLIP; head(vold=...), the range c = hyper["vclip"], by default the clip range).
    d = v - v_old;  v_c = |d| <= c ? v : v_old + copysign(c, d);  l_u = (v - R)^2;  l_c = (v_c - R)^2
    lv = 0.5 max(l_u, l_c);  dL/dv = l_u >= l_c ? v - R : 0;  g_v = m c_v dL/dv
  v_c is a clamp of v: continuous and 1-Lipschitz, so |v_c' - v_c| <= e_vc = E_v + 2u (|v| + |v_old| + c) (the input's
  bound, and the two operations v - v_old, v_old + c on their magnitudes) whichever way the select |d| <= c went.  The
  gradient is two-valued.  Inside the range v_c IS v, l_c IS l_u on the device as in the reference, and the gradient is
  v - R.  The select is ambiguous (either branch is allowed, delta_v grows by m c_v (|v - R| + E_v)) where
      | |d| - c | <= e_d = E_v + 2u (|v| + |v_old|)                      the device may be on the other side of the range, or
      |d| > c and |l_u - l_c| <= err(l_u) + err(l_c)                     the two losses are within their own error:
      err(l_u) = 2 |v - R| e_dv + e_dv^2 + 2u l_u,  e_dv = E_v + 2u |v - R|
      err(l_c) = 2 |v_c - R| e_dc + e_dc^2 + 2u l_c,  e_dc = 2u (|v_c| + |v_c - R|)    (outside, v_c does not depend on v)

The KL penalty (KLPEN; head(beta=...); beta = None is the option off, beta = 0 computes the plane and adds nothing).
    q_a = exp(olp_a);  S = sum q_a;  KL = sum q_a (olp_a - lp_a);  g_a += m beta (p_a S - q_a)
  q_a has the relative error 2u of its exp, S the A - 1 additions on top: dS = 2 (A + 1) u S.  The gradient term, five
  operations (p S, the subtraction, m beta, the product, the addition to g): its allowance is
      m beta (p_a (rp S + (1 + rp) dS) + 2u q_a + 12u (p_a S + q_a)) + 2u m (|gs| |(a == act) - p_a| + c_e p_a |lp_a + ent|)

Advantage normalisation (ADVN; head(advs=(mean_f, inv_f)) with update_ref.stats' two fp32 values).
    adv = fp32(fp32(a - mean_f) * inv_f), the two roundings of the device, taken in float32
  The device forms mean_f and inv_f from its own double sums, whose last bits may differ, so each may be one fp32 ulp off:
      e_adv = (inv_f ulp(mean_f) + |a - mean_f| ulp(inv_f)) (1 + 4u) + 4u |adv|     (the two operations, on the moved value)
  gs = -rho adv moves by rho e_adv (1 + rr); where |adv| <= e_adv the device's advantage may have the other sign and read
  the other clip edge: either outcome is allowed there (the row counts as ambiguous) and dgs grows by rho |adv|.

Underflow.  expf of the device may return a subnormal (gradual underflow) or 0 (flush) below 2^-126, the smallest fp32
normal; which of the two has not been assumed.  Either way the ABSOLUTE error of p_a, q_a and exp(z_a - mx) is at most
T = 2^-126 there, where the relative bound rp no longer holds.  T is 2^-126 on the rows where some p_a (with the KL
option: or some q_a) is below 2^-100, and exactly 0 on every other row, which keeps the bounds above as they are.  Pushed
through: se >= 1 moves by A T, so dl += A T;  ent = -sum p lp: de += T sum |lp_a|;  g_a: += m T (|gs| + c_e (|lp_a + ent|
+ dl + de));  S: dS += A T;  KL: += T sum |olp_a - lp_a|;  the KL gradient: += m beta T (S + dS + 1).
A flushed p just under 2^-126 errs by nearly all of T, so on these rows a flushing implementation can come close to the
bound itself (the float32 restatement with flushed subnormals: 0.74 of delta); with gradual underflow, and on every
other row, the restatement keeps to 1 / FLOOR_FACTOR (tests/test_head_ref_cpu.py).

The per-sample planes (planes(); the engine's names).  adv is the advantage the row trains on, e_adv = 0 without ADVN.
    ratio           rho                                   rho rr
    entropies       ent                                   de
    clipped_losses  min(rho adv, clamp(rho, 1 -+ clip) adv)
                    min and the clamp are continuous and 1-Lipschitz, so there is no edge term:
                    a_hi (rho rr + 2u (1 + clip)) + 6u a_hi max(rho, crho) + max(rho, crho) e_adv,  a_hi = |adv| + e_adv
                    (1 -+ clip in fp32: one operation; the product and the min's two candidates: three)
    value_losses    0.5 (v - R)^2:   |v - R| e_dv + e_dv^2 / 2 + 2u l_u, e_dv = E_v + 4u |v - R|  (|v - R| E_v + E_v^2 / 2 and the
                    roundings of the subtraction and the square; the halving is exact).  Here the roundings take
                    FLOOR_FACTOR = 4 times the plain count, not twice: the plane has no exp and no sum whose count is
                    generous, its two roundings can go the same way, and the float32 restatement does come to 1.4 u l_u of
                    the plain 1.5 u l_u where E_v = 0 - four times the plain count is what keeps it within 1 / FLOOR_FACTOR
                    with VCLIP 0.5 max(l_u, l_c): max is continuous, so the larger of that and the same expression in
                    |v_c - R| with e_dc = e_vc + 4u |v_c - R|
    approx_kl       (rho - 1) - logr: it cancels, so the bound is absolute, from both terms:
                    rho rr + (dl + 2u |logr|) + 4u (|rho - 1| + |logr|)
    kl              sum q_a (olp_a - lp_a):  sum q_a (dl + 2 (A + 3) u |olp_a - lp_a|) + T sum |olp_a - lp_a|
                    (q's exp, the subtraction, the product and the A - 1 additions, on each term's magnitude)
    total_losses    -obj + c_v lv - c_e ent (+ beta KL): the weighted sum of the bounds above
                    + 12u (|obj| + c_v lv + c_e ent + beta |KL|)   (three products, three additions)
    clip_fraction   |rho - 1| > clip ? 1 : 0, exactly; where | |rho - 1| - clip | <= rr rho + 2u either value is allowed
                    (a value that is neither 0 nor 1 never is).
Masked rows are computed like the others (only the gradients carry the mask).

Two-valued selects.  ambiguous() gives, per row, the selects whose outcome the bound cannot decide: the clip select of gs
(rho within rr rho of the edge its advantage's sign reads, or that sign itself under ADVN), the clip fraction's, and the
value-clip select.  Their share is capped: at most one row in 16 of a test row (AMBIGUOUS_CAP), asserted on the reference
alone by tests/test_head_ref_cpu.py and against the engine's rows by tests/test_gpu_head.py.

f16 planes.  A context with ROLLOUT_FP16 stores old log-probs, advantages, returns and old values in binary16; the
reference reads them as stored, as_stored(): rounded to binary16 (to nearest even) and widened, as
tests/test_batch_stats.py treats them.  Then sum q != 1 in general, which is what S is for.

Means.  metrics_reduce_kernel sums one plane over the unmasked rows of a minibatch with 256 threads: a thread's running
sum over its ceil(B / 256) rows, the six steps of the wave butterfly, the two levels over the four waves (block_sum.hpp),
and the host divides by the count: a term passes through at most d = ceil(B / 256) + 8 additions and one division.
The depth is derived as test_optimizer_step.test_reported_norm derives sumsq_kernel's; the terms here are signed, so the
bound is on sum |x_i|, and like every bound of this module it takes twice the plain count (with the plain count the
float32 sum in the kernel's order comes to 0.31 of it on one operator row, which is more than 1 / FLOOR_FACTOR):
    |mean' - mean| <= 2 d u sum |x_i| / n + 2u |mean|
against the float64 masked mean of the engine's OWN exported plane (mean_bound())."""
import numpy as np

from backward_ref import FLOOR_FACTOR, U

PLANES = ("total_losses", "clipped_losses", "value_losses", "entropies", "ratio", "approx_kl", "clip_fraction", "kl")
AMBIGUOUS_CAP = 1.0 / 16
TINY = 2.0 ** -126


def as_stored(x, f16):
    """a per-sample plane as the context stores it: float32, through binary16 where the planes are f16"""
    x = np.asarray(x, np.float32)
    return x.astype(np.float16).astype(np.float32) if f16 else x


def planes(hd):
    """{plane: (value float64 [B], bound float64 [B])} of a backward_ref.head result; "kl" only with the KL option; for
    "clip_fraction" the bound is 1 where either value is allowed and 0 elsewhere"""
    clip, c_v, c_e = (hd.hyper[k] for k in ("clip", "c_v", "c_e"))
    A, rho, rr, adv, logr = hd.A, hd.rho, hd.rr, hd.adv, hd.logr
    e_adv = 0.0 if hd.e_adv is None else hd.e_adv
    out = {"ratio": (rho, rho * rr), "entropies": (hd.ent, hd.de)}
    crho = np.minimum(np.maximum(rho, 1 - clip), 1 + clip)
    obj = np.minimum(rho * adv, crho * adv)
    top = np.maximum(rho, crho)
    a_hi = np.abs(adv) + e_adv
    b_obj = a_hi * (rho * rr + 2 * U * (1 + clip)) + 6 * U * a_hi * top + top * e_adv
    out["clipped_losses"] = (obj, b_obj)
    dv = hd.v - hd.ret
    e_dv = hd.E_v + FLOOR_FACTOR * U * np.abs(dv)
    lu = dv * dv
    b_lv = np.abs(dv) * e_dv + e_dv ** 2 / 2 + FLOOR_FACTOR / 2 * U * lu
    lv = 0.5 * lu
    if hasattr(hd, "vclip"):
        w = hd.vclip
        e_dc = w["e_vc"] + FLOOR_FACTOR * U * np.abs(w["dc"])
        b_lv = np.maximum(b_lv, np.abs(w["dc"]) * e_dc + e_dc ** 2 / 2 + FLOOR_FACTOR / 2 * U * w["lc"])
        lv = 0.5 * np.maximum(w["lu"], w["lc"])
    out["value_losses"] = (lv, b_lv)
    out["approx_kl"] = ((rho - 1) - logr, rho * rr + (hd.dl + 2 * U * np.abs(logr)) + 4 * U * (np.abs(rho - 1) + np.abs(logr)))
    total = -obj + c_v * lv - c_e * hd.ent
    b_tot = b_obj + c_v * b_lv + c_e * hd.de
    mag = np.abs(obj) + c_v * lv + c_e * hd.ent
    if hasattr(hd, "kl"):
        k = hd.kl
        diff = np.abs(hd.olp - hd.lp)
        b_kl = (k["q"] * (hd.dl[:, None] + 2 * (A + 3) * U * diff)).sum(axis=1) + hd.T * diff.sum(axis=1)
        out["kl"] = (k["kl"], b_kl)
        if k["beta"] != 0.0:
            total = total + k["beta"] * k["kl"]
            b_tot = b_tot + k["beta"] * b_kl
            mag = mag + k["beta"] * np.abs(k["kl"])
    out["total_losses"] = (total, b_tot + 12 * U * mag)
    cf_amb = np.abs(np.abs(rho - 1) - clip) <= rr * rho + 2 * U
    out["clip_fraction"] = ((np.abs(rho - 1) > clip).astype(np.float64), cf_amb.astype(np.float64))
    return out


def ambiguous(hd):
    """{select: bool [B]}: "clip" (the select of gs, the advantage's sign included), "clip_fraction", "value" (the value-clip
    select; absent without the option) - the rows on which the reference allows either outcome"""
    out = dict(clip=hd.near & (hd.adv != 0), clip_fraction=planes(hd)["clip_fraction"][1] != 0)
    if hasattr(hd, "vclip"):
        out["value"] = hd.vclip["ambiguous"]
    return out


def ambiguous_rows(hd):
    """bool [B]: ambiguous in any select"""
    return np.logical_or.reduce(list(ambiguous(hd).values()))


def _ratio(d, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))


def plane_ratios(hd, got):
    """{plane: |got - reference| / bound per row [B]} of the engine's names (any subset of PLANES; a NaN stays a NaN); for
    clip_fraction 0 where the value is the reference's, 1 where it is the other one on an ambiguous row, inf elsewhere"""
    want = planes(hd)
    out = {}
    for name, g in got.items():
        ref, bound = want[name]
        g = np.asarray(g, np.float64).reshape(ref.shape)
        if name == "clip_fraction":
            out[name] = np.where(g == ref, 0.0, np.where((bound != 0) & ((g == 0) | (g == 1)), 1.0, np.inf))
        else:
            out[name] = _ratio(np.abs(g - ref), bound)
    return out


def check_planes(hd, got):
    """got: {plane: float32 [B]}.  Returns (failures, worst): worst {plane: the largest |d| / bound} (for clip_fraction: the
    number of rows on which the engine's value was allowed only because the row is ambiguous)"""
    want = planes(hd)
    failures, worst = [], {}
    for name, r in plane_ratios(hd, got).items():
        bad = np.flatnonzero(~(r <= 1))
        worst[name] = int((r == 1).sum()) if name == "clip_fraction" else (float(r.max()) if r.size else 0.0)
        if len(bad):
            i = int(bad[0])
            failures.append("%s: %d rows outside the bound, first %d: got %r, want %r, bound %r" % (
                name, len(bad), i, float(np.asarray(got[name]).ravel()[i]), float(want[name][0][i]), float(want[name][1][i])))
    return failures, worst


def g_ratios(hd, got):
    """|got - g| / delta per element [B, A + 1]"""
    return _ratio(np.abs(np.asarray(got, np.float64) - hd.g), hd.delta)


def check_g(hd, got):
    """g [B, A + 1] (the operator's dlogits and dvalues: the identity head's dh) against delta, element by element; a
    masked row must be exactly 0.  Returns (failures, worst |d| / delta over the unmasked rows)"""
    got = np.asarray(got, np.float64)
    ratio = g_ratios(hd, got)
    live = hd.m != 0
    failures = []
    if got[~live].any():
        failures.append("g: a masked row is not exactly zero")
    bad = np.argwhere(~(ratio <= 1))
    if len(bad):
        i = tuple(int(j) for j in bad[0])
        failures.append("g: %d elements outside delta, first %s: got %r, want %r, delta %r" % (
            len(bad), i, float(got[i]), float(hd.g[i]), float(hd.delta[i])))
    return failures, float(ratio[live].max()) if live.any() else 0.0


def mean_bound(plane, masks):
    """(the float64 masked mean of `plane` [B], its bound): the module docstring's "Means\""""
    x = np.asarray(plane, np.float64)[np.asarray(masks) != 0]
    n = x.size
    depth = -(-len(np.asarray(plane)) // 256) + 8
    mean = x.sum() / n
    return mean, 2 * depth * U * np.abs(x).sum() / n + 2 * U * abs(mean)
