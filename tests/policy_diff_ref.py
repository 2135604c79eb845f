"""aleppo_policy_diff's definitions (include/aleppo.h) in numpy, from the fp32 logits, values and fc rows of two parameter
sets; float64 by default, np.longdouble to measure what float64 itself loses.

reference(...) returns {"stats": [16], "per_sample": [rows, 8], "transitions": int64 [A, A], "lmax": max |logit| over the
rows that entered, "lmax_rows": the same per row}.  bound(...) is the issue's bound 1e-12 * (1 + max|l| + |reference|):
device and numpy differ only in double exp / log (a few ulp) and in summation order - about 4 A + H + 20 double operations
per row and one addition per row in the sums - so about 100 x 2^-53 x that count.  check(...) compares an answer with the
reference: integers exactly, every other number within the bound (a per-sample column at its own row's max |l|); it
returns the failures and the worst value / bound ratio.

plant: one deliberate error of an implementation, for the tests that show the bound rejects it -
  "kl_swap" the two KL directions exchanged, "tie_high" a tie taken to the highest index, "tv_whole" tv without the 0.5,
  "dv_sign" v_a - v_b, "drop_last" the last fc column left out of the dot products, "count_nonfinite" a non-finite row
  counted in (its numbers as they come)."""
import numpy as np

STATS = ("rows", "nonfinite_rows", "churn", "mean_kl_ab", "max_kl_ab", "mean_kl_ba", "mean_tv", "max_tv", "mean_abs_dv",
         "max_abs_dv", "rms_dv", "mean_entropy_a", "mean_entropy_b", "mean_feature_cos", "min_feature_cos",
         "feature_rel_change")
IDX = {k: i for i, k in enumerate(STATS)}
COLUMNS = ("kl_ab", "kl_ba", "tv", "dv", "cos", "dh2", "g_a", "g_b")
COL = {k: i for i, k in enumerate(COLUMNS)}
INTEGER_STATS = ("rows", "nonfinite_rows")
PLANTS = ("kl_swap", "tie_high", "tv_whole", "dv_sign", "drop_last", "count_nonfinite")


def _log_softmax(l):
    z = l - l.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def _greedy(l, high=False):
    if high:
        return l.shape[1] - 1 - np.argmax(l[:, ::-1], axis=1)
    return np.argmax(l, axis=1)  # the first (lowest) index of the maximum


def finite_rows(*arrays):
    ok = np.ones(arrays[0].shape[0], bool)
    for a in arrays:
        ok &= np.isfinite(np.asarray(a, np.float64).reshape(a.shape[0], -1)).all(axis=1)
    return ok


def reference(logits_a, values_a, h_a, logits_b, values_b, h_b, dtype=np.float64, plant=None):
    assert plant is None or plant in PLANTS
    src = [np.asarray(x, np.float32) for x in (logits_a, values_a, h_a, logits_b, values_b, h_b)]
    n, A = src[0].shape
    ok = finite_rows(*src)
    keep = np.ones(n, bool) if plant == "count_nonfinite" else ok
    with np.errstate(all="ignore"):
        la, va, ha, lb, vb, hb = (x[keep].astype(dtype) for x in src)
        rows = int(keep.sum())
        per = np.full((n, len(COLUMNS)), np.nan, dtype)
        trans = np.zeros((A, A), np.int64)
        stats = np.zeros(len(STATS), dtype)
        stats[IDX["rows"]], stats[IDX["nonfinite_rows"]] = rows, n - rows
        out = dict(stats=stats, per_sample=per, transitions=trans, lmax=0.0, lmax_rows=np.zeros(n), finite=ok)
        if rows == 0:
            return out
        pa, pb = _log_softmax(la), _log_softmax(lb)
        qa, qb = np.exp(pa), np.exp(pb)
        kl_ab, kl_ba = (qa * (pa - pb)).sum(axis=1), (qb * (pb - pa)).sum(axis=1)
        if plant == "kl_swap":
            kl_ab, kl_ba = kl_ba, kl_ab
        tv = np.abs(qa - qb).sum(axis=1) * (1 if plant == "tv_whole" else dtype(0.5))
        dv = va - vb if plant == "dv_sign" else vb - va
        if plant == "drop_last":
            ha, hb = ha[:, :-1], hb[:, :-1]
        dab, daa, dbb = (ha * hb).sum(axis=1), (ha * ha).sum(axis=1), (hb * hb).sum(axis=1)
        zero = (daa == 0) | (dbb == 0)
        cos = np.where(zero, dtype(1), dab / np.sqrt(np.where(zero, dtype(1), daa * dbb)))
        dh2 = ((hb - ha) ** 2).sum(axis=1)
        ga, gb = _greedy(la, plant == "tie_high"), _greedy(lb, plant == "tie_high")
        per[keep] = np.stack([kl_ab, kl_ba, tv, dv, cos, dh2, ga.astype(dtype), gb.astype(dtype)], axis=1)
        np.add.at(trans, (ga, gb), 1)
        ea, eb = -(qa * pa).sum(axis=1), -(qb * pb).sum(axis=1)
        s = lambda k, v: stats.__setitem__(IDX[k], v)
        s("churn", dtype((ga != gb).sum()) / rows)
        s("mean_kl_ab", kl_ab.sum() / rows)
        s("max_kl_ab", kl_ab.max())
        s("mean_kl_ba", kl_ba.sum() / rows)
        s("mean_tv", tv.sum() / rows)
        s("max_tv", tv.max())
        s("mean_abs_dv", np.abs(dv).sum() / rows)
        s("max_abs_dv", np.abs(dv).max())
        s("rms_dv", np.sqrt((dv * dv).sum() / rows))
        s("mean_entropy_a", ea.sum() / rows)
        s("mean_entropy_b", eb.sum() / rows)
        s("mean_feature_cos", cos.sum() / rows)
        s("min_feature_cos", cos.min())
        s("feature_rel_change", np.sqrt(dh2.sum() / daa.sum()) if daa.sum() > 0 else 0)
        both = np.concatenate([la, lb], axis=1)
        lrow = np.zeros(n)
        lrow[keep] = np.abs(np.where(np.isfinite(both), both, 0)).max(axis=1).astype(np.float64)
        out["lmax"], out["lmax_rows"] = float(lrow.max()), lrow
    return out


def bound(lmax, ref):
    return 1e-12 * (1.0 + lmax + np.abs(np.asarray(ref, np.float64)))


def check(stats, per_sample, transitions, ref):
    """an answer (stats [16], per_sample [rows, 8] or None, transitions [A, A] or None) against reference(...)'s result:
    (failures, worst value / bound over the non-integer numbers)"""
    bad, worst = [], 0.0
    stats = np.asarray(stats)
    rs, lmax = ref["stats"], ref["lmax"]

    def close(name, got, want, lmax=lmax):
        nonlocal worst
        got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
        if not (np.isnan(got) == np.isnan(want)).all():
            bad.append(f"{name}: NaN pattern")
            return
        m = ~np.isnan(want)
        if not m.any():
            return
        r = np.abs(got[m] - want[m]) / bound(lmax if np.isscalar(lmax) else lmax[m], want[m].astype(np.float64))
        w = float(np.nan_to_num(r, nan=np.inf).max())
        worst = max(worst, w)
        if not w <= 1.0:
            bad.append(f"{name}: {w:.3g} of the bound")

    for k in INTEGER_STATS:
        if stats[IDX[k]] != rs[IDX[k]]:
            bad.append(f"{k}: {stats[IDX[k]]} != {rs[IDX[k]]}")
    rows = int(rs[IDX["rows"]])
    churned = int(np.rint(float(rs[IDX["churn"]]) * rows)) if rows else 0
    if stats[IDX["churn"]] != (churned / rows if rows else 0.0):
        bad.append(f"churn: {stats[IDX['churn']]} != {churned} / {rows}")
    for k in STATS:
        if k not in INTEGER_STATS and k != "churn":
            close(k, stats[IDX[k]], rs[IDX[k]])
    if per_sample is not None:
        rp = ref["per_sample"]
        for k in ("g_a", "g_b"):
            a, b = per_sample[:, COL[k]], rp[:, COL[k]].astype(np.float64)
            if not np.array_equal(a, b, equal_nan=True):
                bad.append(f"{k}: differs")
        for k in COLUMNS[:6]:
            close(k, per_sample[:, COL[k]], rp[:, COL[k]], ref["lmax_rows"])  # (each row at its own max |l|)
    if transitions is not None and not np.array_equal(transitions, ref["transitions"]):
        bad.append("transitions differ")
    return bad, worst
