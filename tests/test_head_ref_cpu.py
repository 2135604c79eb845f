"""tests/head_ref.py and the options of backward_ref.head, on the CPU: room and teeth on the inputs of every row of
tests/test_gpu_head.py.

Room: backward_ref.restate_f32, the float32 numpy restatement of head_train_body.inc extended by the same options, stands
in for the kernel - once with numpy's gradual-underflow exp and once with every subnormal exp result flushed to zero - on
the CPU oracle's h (the bf16 emulation for a bf16 context).  It stays within 1 / FLOOR_FACTOR of every bound: g, dh, dWh,
dbh, each plane, each mean (the mean summed in float32 in metrics_reduce_kernel's order).  With mean_f or inv_f one fp32
ulp off it stays inside the bounds, which is what their advantage term is sized for.
With the options off the extended reference is the old one bit for bit (a copy of the old formulas is kept here).
The inputs are not trivial (asserted per row), and the reference alone keeps the ambiguous rows under the cap.
Teeth: each planted error fails its own check and none in front of it."""
import functools

import numpy as np
import pytest

import backward_ref as br
import head_ref as hr
import layer_ref as lr
import oracle_lib as orc
import update_ref as ur
from backward_ref import U
from test_gpu_backward import HYPER as OLD_HYPER, row_batch
from test_gpu_head import (BETA, ENGINE_ROWS, ENTRIES, HYPER, OPERATOR_ROWS, engine_case, engine_id, head_options,
                           operator_case, operator_reference, stored_batch, take, unit_stats_batch)

ROOM = 1.0 / br.FLOOR_FACTOR
# the order of the checks: a planted error may fail checks from its own on, never one in front of it
ORDER = ("ratio", "entropies", "clipped_losses", "value_losses", "approx_kl", "clip_fraction", "clip_fraction.own", "kl",
         "total_losses", "g.actions", "g.value")


# ------------------------------------------------------------------ the stand-ins' inputs
@functools.lru_cache(maxsize=None)
def _h(n, H, A, bf16):
    """the CPU oracle's fc activations of an engine row (the bf16 emulation for a bf16 context)"""
    params, obs, _ = engine_case(n, H, A)
    acts = orc.net_forward(params, H, A, obs, want_acts=True, emulate_bf16=bf16)[2]
    h = np.ascontiguousarray(acts[:, -H:])
    h.setflags(write=False)
    return h


def engine_standin(row, variant):
    """(h, wh, bh, batch, n_mask, options) of the last minibatch of one variant of an engine row"""
    n, M, H, A, prec, f16, _ = row
    (entry, advn, beta), vclip = variant
    params, obs, raw = engine_case(n, H, A)
    B = n // M
    idx = np.arange((M - 1) * B, M * B)
    batch = take(stored_batch(raw, f16), idx)
    wh, bh = lr.split_params(params, H, A, prec == "bf16")["heads"]
    return _h(n, H, A, prec == "bf16")[idx], wh, bh, batch, int(batch["masks"].sum()), head_options(batch, advn, beta, vclip)


def _variant_id(v):
    return v[0][0] + ("+vclip" if v[1] else "")


ENGINE_CASES = [(r, v) for r in ENGINE_ROWS for v in r[6]]
ENGINE_IDS = ["%s-%s" % (engine_id(r), _variant_id(v)) for r, v in ENGINE_CASES]


# ------------------------------------------------------------------ room
def _tree_mean(x, masks):
    """the masked mean as metrics_reduce_kernel and the host form it, in float32"""
    f = np.float32
    x = np.asarray(x, f)
    acc, cnt = np.zeros(256, f), np.zeros(256, f)
    for i in range(len(x)):
        if masks[i]:
            acc[i % 256] += x[i]
            cnt[i % 256] += f(1)
    out = []
    for v in (acc, cnt):
        v = v.reshape(4, 64).copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, np.arange(64) ^ o]
        out.append((v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0]))
    assert out[0].dtype == f
    return out[0] / out[1]


def _room(title, h, wh, bh, batch, n_mask, opts, hd):
    """Every figure of the restatement within ROOM of its bound.  The one exception is by construction: the flushed run on
    the rows that carry the underflow term T = 2^-126.  A flushed p just under 2^-126 errs by all of T (seen: 0.74 of
    delta on the A = 5 underflow row), so there the figure is held to the bound itself."""
    worst_all = {}
    kl = opts.get("beta") is not None
    f = np.float32
    for flush in (False, True):
        g32, pl = br.restate_f32(h, wh, bh, batch, HYPER, n_mask, flush=flush, planes=True, **opts)
        limit = np.where((hd.T != 0) & flush, 1.0, ROOM)
        assert not g32[hd.m == 0].any()
        ratios = hr.plane_ratios(hd, {k: v for k, v in pl.items() if k != "kl" or kl})
        cf = ratios.pop("clip_fraction")
        assert (cf <= 1).all(), (title, flush, "clip_fraction")
        ratios["g"] = hr.g_ratios(hd, g32).max(axis=1)
        worst = {}
        for k, r in ratios.items():
            assert (r <= limit).all(), (title, "flushed" if flush else "gradual", k, float((r / limit).max()) * ROOM)
            worst[k] = float(r.max())
        top = 1.0 if flush and hd.T.any() else ROOM
        for k, ref, got in (("dh", hd.dh, g32 @ np.asarray(wh, f)), ("dWh", hd.dW, g32.T @ np.asarray(h, f)),
                            ("dbh", hd.db, g32.sum(axis=0, dtype=f))):
            worst[k] = br.bound_check(ref, got, ref.extra)["worst"]
            assert worst[k] <= top, (title, flush, k, worst[k])
        for name in ("total_losses", "approx_kl", "clip_fraction") + (("kl",) if kl else ()):
            mean, bound = hr.mean_bound(pl[name], batch["masks"])
            d = abs(float(_tree_mean(pl[name], batch["masks"])) - mean)
            worst["mean " + name] = d / bound if bound > 0 else float(d > 0)
            assert worst["mean " + name] <= ROOM, (title, flush, name)
        for k, v in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
    if "advs" in opts:  # the device's statistics one fp32 ulp off, each way: inside the bounds (what e_adv is sized for)
        mean_f, inv_f = opts["advs"]
        for dm in (-1, 1):
            for di in (-1, 1):
                off = (np.nextafter(mean_f, np.float32(dm * np.inf)), np.nextafter(inv_f, np.float32(di * np.inf)))
                g32, pl = br.restate_f32(h, wh, bh, batch, HYPER, n_mask, planes=True, **dict(opts, advs=off))
                bad = hr.check_planes(hd, {k: v for k, v in pl.items() if k != "kl" or opts.get("beta") is not None})[0]
                bad += hr.check_g(hd, g32)[0]
                assert not bad, (title, "statistics one ulp off", dm, di, bad)
    amb = hr.ambiguous_rows(hd)
    assert amb.sum() <= max(len(amb) * hr.AMBIGUOUS_CAP, 0 if len(amb) >= 16 else 1), (title, int(amb.sum()))
    return worst_all


@pytest.mark.parametrize("case", ENGINE_CASES, ids=ENGINE_IDS)
def test_room_on_every_engine_row(case):
    row, variant = case
    h, wh, bh, batch, n_mask, opts = engine_standin(row, variant)
    hd = br.head(h, wh, bh, batch, HYPER, n_mask, **opts)
    assert np.abs(hd.logr).max() <= 40
    title = "%s %s" % (engine_id(row), _variant_id(variant))
    worst = _room(title, h, wh, bh, batch, n_mask, opts, hd)
    print("room %s: %s" % (title, " ".join("%s %.3g" % kv for kv in worst.items())))


@pytest.mark.parametrize("A,regime", OPERATOR_ROWS, ids=["A%d-%s" % r for r in OPERATOR_ROWS])
def test_room_on_every_operator_row(A, regime):
    logits, values, batch = operator_case(A, regime)
    hd, (h, wh) = operator_reference(A, regime)
    assert np.abs(hd.logr).max() <= 40 and not hd.E_l.any() and not hd.E_v.any()
    assert (hd.T != 0).any() == (regime == "underflow" and A > 1)
    if regime == "peaked" and A > 1:  # (no underflow term anywhere: the bounds are the plain ones)
        assert hd.p.min() >= 2.0 ** -100 and 20 * (A > 2) <= (hd.z.max(axis=1) - hd.z.min(axis=1)).min()
    worst = _room("operator A%d %s" % (A, regime), h, wh, np.zeros(A + 1, np.float32), batch, int(batch["masks"].sum()), {}, hd)
    print("room operator A%d %s: %s" % (A, regime, " ".join("%s %.3g" % kv for kv in worst.items())))


def test_without_its_underflow_term_the_bound_fails_on_the_underflow_rows():
    """what the term is for: on a row with p below the smallest normal the flushed restatement leaves the bound that has
    no absolute term by a large factor (the room test shows it inside the one that has it)"""
    A = 6
    logits, values, batch = operator_case(A, "underflow")
    hd, (h, wh) = operator_reference(A, "underflow")
    g32 = br.restate_f32(h, wh, np.zeros(A + 1, np.float32), batch, HYPER, int(batch["masks"].sum()), flush=True)
    sub = (hd.p < hr.TINY) & (hd.p > 2.0 ** -149) & (hd.m != 0)[:, None]
    assert sub.any()
    d = np.abs(g32[:, :A].astype(np.float64) - hd.g[:, :A])
    m, T = hd.m[:, None], hd.T[:, None]
    gs_hi = np.abs(hd.g[:, :A]).max(axis=1, keepdims=True) / np.maximum(m, 1e-300)  # (at least |gs| (1 - p_act))
    plain = hd.delta[:, :A] - m * T * (gs_hi + HYPER["c_e"] * np.abs(hd.lp + hd.ent[:, None]))
    assert (d[sub] > np.maximum(plain[sub], 0)).any() and (d <= hd.delta[:, :A]).all()


# ------------------------------------------------------------------ the options off
def _old_g_delta(h, wh, bh, batch, hyper, n_mask):
    """backward_ref.head's g and delta as they were before the options (the formulas of its docstring, unchanged)"""
    h = np.asarray(h, np.float32)
    wh, bh = np.asarray(wh, np.float32), np.asarray(bh, np.float32)
    B, A = h.shape[0], wh.shape[0] - 1
    clip, c_v, c_e = (float(np.float32(hyper[k])) for k in ("clip", "c_v", "c_e"))
    E, fwd = br._logits_bound(h, wh, bh)
    z, v = fwd.z[:, :A], fwd.z[:, A]
    act = np.asarray(batch["actions"], np.int64)
    olp = np.asarray(batch["old_lp"], np.float32).astype(np.float64)
    adv, ret = (np.asarray(batch[k], np.float32).astype(np.float64) for k in ("adv", "ret"))
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
    g = np.concatenate([m[:, None] * (gs[:, None] * (onehot - p) + c_e * p * (lp + ent[:, None])),
                        (m * c_v * (v - ret))[:, None]], axis=1)
    E_l, E_v = E[:, :A].max(axis=1), E[:, A]
    e_lp = 2 * (A + 5) * U * (np.abs(z).max(axis=1) + np.abs(lse) + 1)
    dl = 2 * E_l + e_lp
    rp = np.expm1(dl) + 2 * U
    de = rp * ent + (1 + rp) * dl + 2 * (A + 1) * U * ent
    rr = np.expm1(dl + 2 * U * np.abs(logr)) + 4 * U
    edge = np.where(adv >= 0, 1 + clip, 1 - clip)
    dgs = np.abs(adv) * rho * (rr + (np.abs(rho - edge) <= rr * rho))
    gs_hi = np.maximum(np.abs(gs), np.where(np.abs(rho - edge) <= rr * rho, np.abs(adv) * rho, 0.0))
    t1_hi = gs_hi[:, None] * np.abs(onehot - p)
    delta_a = m[:, None] * (dgs[:, None] * np.abs(onehot - p) + gs_hi[:, None] * p * rp[:, None]
                            + c_e * p * (rp[:, None] * np.abs(lp + ent[:, None]) + (1 + rp[:, None]) * (dl + de)[:, None])) \
        + 18 * U * m[:, None] * (t1_hi + t2)
    delta_v = m * c_v * (E_v + 8 * U * np.abs(v - ret))
    return g, np.concatenate([delta_a, delta_v[:, None]], axis=1)


def test_with_the_options_off_the_reference_is_the_old_one_bit_for_bit():
    """on an existing case of tests/test_gpu_backward.py (n = 37, H = 96, A = 6, bf16) and on a peaked engine row"""
    n, H, A = 37, 96, 6
    params, obs, batch = row_batch(n, H, A, False)
    h = orc.net_forward(params, H, A, obs, want_acts=True, emulate_bf16=True)[2][:, -H:]
    wh, bh = lr.split_params(params, H, A, True)["heads"]
    cases = [(h, wh, bh, batch, OLD_HYPER, int(batch["masks"].sum()))]
    h2, wh2, bh2, b2, nm2, _ = engine_standin(ENGINE_ROWS[4], (ENTRIES[0], False))
    cases.append((h2, wh2, bh2, b2, HYPER, nm2))
    for args in cases:
        g, delta = _old_g_delta(*args)
        for hd in (br.head(*args), br.head(*args, vold=None, beta=None, advs=None, exact_logits=False)):
            assert hd.g.tobytes() == g.tobytes() and hd.delta.tobytes() == delta.tobytes()
            assert np.array_equal(hd.dh.extra, delta @ np.abs(np.asarray(args[1], np.float64)))
        assert not hasattr(hd, "vclip") and not hasattr(hd, "kl") and not hd.T.any()
        g32, pl = br.restate_f32(*args, planes=True)
        assert g32.tobytes() == br.restate_f32(*args).tobytes()


# ------------------------------------------------------------------ the inputs are not trivial
@pytest.mark.parametrize("row", [r for r in ENGINE_ROWS if r[0] > 1], ids=[engine_id(r) for r in ENGINE_ROWS if r[0] > 1])
def test_the_inputs_are_not_in_a_trivial_regime(row):
    n, M, H, A, prec, f16, variants = row
    for advn in (False, True):
        h, wh, bh, batch, n_mask, opts = engine_standin(row, (("", advn, BETA), True))
        hd = br.head(h, wh, bh, batch, HYPER, n_mask, **opts)
        live = batch["masks"] != 0
        assert 0 < (~live).sum() < len(live)
        assert (hd.adv[live] > 0).any() and (hd.adv[live] < 0).any()
        w = hd.vclip
        inside = np.abs(w["d"]) <= w["c"]
        assert inside[live].any() and (~inside[live]).any() and (w["zero"] & live).any() and (~w["zero"] & ~inside & live).any()
        if A > 1:
            assert hd.active[live].any() and (~hd.active[live]).any()
            assert hd.p.min() < 1e-10 and (hd.ent < 1e-3).any() and np.abs(hd.lp[np.arange(len(live)), hd.act]).max() > 20
            assert hd.rho.min() < 0.9 and hd.rho.max() > 1.1
            assert np.abs(hd.kl["S"] - 1).max() > 1e-5 or not f16


# ------------------------------------------------------------------ teeth
def stand_in(hd, batch, hyper, n_mask, *, vold=None, beta=None, advs=None, bug=None):
    """(g float64 [B, A + 1], {plane: float32 [B]}) in float64 from the reference's own exact z and v, the planes rounded to
    float32 as an engine stores them and the clip fraction taken from the float32 ratio: without `bug` it passes every
    check; `bug` names one planted error"""
    z, v = hd.z, hd.v
    B, A = z.shape
    clip, c_v, c_e = (float(np.float32(hyper[k])) for k in ("clip", "c_v", "c_e"))
    act = np.asarray(batch["actions"], np.int64)
    olp = np.asarray(batch["old_lp"], np.float32).astype(np.float64)
    adv, ret = (np.asarray(batch[k], np.float32).astype(np.float64) for k in ("adv", "ret"))
    if advs is not None:
        mean_f, inv_f = advs
        if bug == "std without its 1e-8":
            inv_f = np.float32(1.0 / ur.stats(batch["adv"], batch["masks"])[2])
        adv = ((np.asarray(batch["adv"], np.float32) - np.float32(mean_f)) * np.float32(inv_f)).astype(np.float64)
    m = np.where(np.asarray(batch["masks"]) != 0, float(np.float32(1.0) / np.float32(n_mask)), 0.0)
    idx = np.arange(B)
    lse = np.log(np.exp(z - z.max(axis=1)[:, None]).sum(axis=1)) + z.max(axis=1)
    lp = z - lse[:, None]
    p = np.exp(lp)
    terms = p * lp
    if bug == "entropy without its last action":
        terms = terms[:, :A - 1]
    ent = -terms.sum(axis=1)
    logr = lp[idx, act] - olp[idx, act]
    rho = np.exp(logr)
    active = np.where(adv >= 0, rho <= 1 + clip, rho >= 1 - clip)
    gs = np.where(active, -rho * adv, 0.0)
    onehot = np.zeros((B, A))
    onehot[idx, (act + 1) % A if bug == "a == act one action over" else act] = 1.0
    g_a = m[:, None] * (gs[:, None] * (onehot - p) + c_e * p * (lp + ent[:, None]))
    dv = v - ret
    if vold is None:
        lv, dvg = 0.5 * dv * dv, dv
    else:
        c = float(np.float32(hyper.get("vclip", hyper["clip"])))
        vo = np.asarray(vold, np.float32).astype(np.float64)
        d = v - vo
        step = np.full(B, c) if bug == "vc with +c whatever the sign" else np.copysign(c, d)
        vc = np.where(np.abs(d) <= c, v, vo + step)
        lu, lc = dv * dv, (vc - ret) ** 2
        lv = 0.5 * np.maximum(lu, lc)
        unclipped = lu > lc if bug == "the tie to the clipped branch" else lu >= lc
        dvg = dv if bug == "dvg kept on the clipped branch" else np.where(unclipped, dv, 0.0)
    kl = np.zeros(B)
    if beta is not None:
        q = np.exp(lp if bug == "q from lp" else olp)
        S = np.ones(B) if bug == "S = 1" else q.sum(axis=1)
        kl = (q * (olp - lp)).sum(axis=1)
        if beta != 0:
            g_a = g_a + m[:, None] * float(np.float32(beta)) * (p * S[:, None] - q)
    crho = np.minimum(np.maximum(rho, 1 - clip), 1 + clip)
    obj = np.minimum(rho * adv, crho * adv)
    total = -obj + c_v * lv - c_e * ent + (float(np.float32(beta)) * kl if beta else 0.0)
    f = np.float32
    rho32 = rho.astype(f)
    over = np.abs(rho32 - f(1)) >= f(clip) if bug == "clip fraction with >=" else np.abs(rho32 - f(1)) > f(clip)
    akl = 0.5 * logr ** 2 if bug == "approx-KL as half the squared log-ratio" else (rho - 1) - logr
    planes = dict(total_losses=total, clipped_losses=obj, value_losses=lv, entropies=ent, ratio=rho, approx_kl=akl,
                  clip_fraction=over.astype(np.float64))
    if beta is not None:
        planes["kl"] = kl
    return np.concatenate([g_a, (m * c_v * dvg)[:, None]], axis=1), {k: x.astype(f) for k, x in planes.items()}


def failed_checks(hd, g, planes, hyper=HYPER):
    """the names of the checks that fail, in ORDER"""
    bad = {f.split(":")[0] for f in hr.check_planes(hd, planes)[0]}
    own = (np.abs(planes["ratio"] - np.float32(1)) > np.float32(hyper["clip"])).astype(np.float32)
    if not np.array_equal(own, planes["clip_fraction"]):
        bad.add("clip_fraction.own")
    with np.errstate(invalid="ignore"):
        out = ~(np.abs(np.asarray(g, np.float64) - hd.g) <= hd.delta)
    if out[:, :hd.A].any():
        bad.add("g.actions")
    if out[:, hd.A].any():
        bad.add("g.value")
    assert bad <= set(ORDER), bad
    return [n for n in ORDER if n in bad]


def _assert_tooth(hd, batch, n_mask, opts, bug, own, hyper=HYPER):
    assert failed_checks(hd, *stand_in(hd, batch, hyper, n_mask, **opts), hyper) == [], "the stand-in itself"
    failed = failed_checks(hd, *stand_in(hd, batch, hyper, n_mask, bug=bug, **opts), hyper)
    print("%s -> %s" % (bug, failed))
    assert own in failed and failed[0] == own, (bug, failed)


def _row(A, prec="bf16", f16=True):
    return (37, 1, 32, A, prec, f16, None)


ALL = (ENTRIES[3], True)  # every option on


def _reference(row, variant, change=None):
    h, wh, bh, batch, n_mask, opts = engine_standin(row, variant)
    if change:
        batch, opts = change(dict(batch), dict(opts))
    return br.head(h, wh, bh, batch, HYPER, n_mask, **opts), batch, n_mask, opts


@pytest.mark.parametrize("A", [4, 7, 11])
def test_teeth_s_replaced_by_1_in_the_kl_gradient(A):
    def change(batch, opts):  # an old policy whose q does not sum to 1: every row's log-probs moved by up to +-0.1
        shift = np.linspace(-0.1, 0.1, len(batch["old_lp"]), dtype=np.float32)[:, None]
        batch["old_lp"] = (batch["old_lp"] + shift).astype(np.float32)
        return batch, opts
    hd, batch, n_mask, opts = _reference(_row(A), ALL, change)
    assert np.abs(hd.kl["S"] - 1).max() > 0.05
    _assert_tooth(hd, batch, n_mask, opts, "S = 1", "g.actions")


@pytest.mark.parametrize("bug,own", [("q from lp", "kl"), ("the tie to the clipped branch", "g.value"),
                                     ("dvg kept on the clipped branch", "g.value"),
                                     ("vc with +c whatever the sign", "value_losses"),
                                     ("approx-KL as half the squared log-ratio", "approx_kl"),
                                     ("a == act one action over", "g.actions")])
@pytest.mark.parametrize("A,prec,f16", [(6, "fp32", False), (11, "bf16", True)])
def test_teeth_one_planted_error(bug, own, A, prec, f16):
    hd, batch, n_mask, opts = _reference(_row(A, prec, f16), ALL)
    _assert_tooth(hd, batch, n_mask, opts, bug, own)


def test_teeth_the_advantage_normalised_with_std_instead_of_std_plus_1e_8():
    """on a minibatch of near-equal advantages: +-x pairs with x ~ 1e-7 (mean exactly 0, std ~ 1e-7, so the 1e-8 is a tenth)"""
    def change(batch, opts):
        batch = unit_stats_batch(batch)
        live = np.flatnonzero(batch["masks"])
        adv = np.array(batch["adv"])
        adv[live] *= (1e-7 * (1 + (np.arange(len(live)) // 2) / 8.0)).astype(np.float32)
        batch["adv"] = adv
        n, mean, std, mean_f, inv_f = ur.stats(adv, batch["masks"])
        assert mean == 0 and 5e-8 < std < 5e-7
        return batch, dict(opts, advs=(mean_f, inv_f))
    hd, batch, n_mask, opts = _reference(_row(6, "fp32", False), ALL, change)
    _assert_tooth(hd, batch, n_mask, opts, "std without its 1e-8", "clipped_losses")


def test_teeth_the_clip_fraction_with_greater_or_equal_on_a_row_exactly_on_the_edge():
    """clip = 0.125 and a row whose fp32 ratio is exactly 1.125: against the reference the row is ambiguous (either value is
    allowed), so what catches >= is the check on the engine's own ratio plane"""
    hyper = dict(HYPER, clip=0.125)
    A, B = 2, 16
    h = np.zeros((B, 32), np.float32)
    wh, bh = np.eye(A + 1, 32, dtype=np.float32), np.zeros(A + 1, np.float32)
    lp = float(np.log(0.5))
    old_lp = np.full((B, A), lp, np.float32)
    old_lp[5, 1] = np.float32(lp - np.log(1.125))
    batch = dict(actions=np.ones(B, np.int64), old_lp=old_lp, adv=np.linspace(-1, 1, B).astype(np.float32),
                 ret=np.linspace(1, -1, B).astype(np.float32), masks=np.ones(B, np.uint8))
    hd = br.head(h, wh, bh, batch, hyper, B, exact_logits=True)
    assert np.float32(hd.rho[5]) == np.float32(1.125) and hr.ambiguous(hd)["clip_fraction"].tolist() == [i == 5 for i in range(B)]
    _assert_tooth(hd, batch, B, {}, "clip fraction with >=", "clip_fraction.own", hyper)


@pytest.mark.parametrize("A", [5, 7, 11])
def test_teeth_the_entropy_without_its_last_action(A):
    logits, values, batch = operator_case(A, "uniform")
    hd, _ = operator_reference(A, "uniform")
    _assert_tooth(hd, batch, int(batch["masks"].sum()), {}, "entropy without its last action", "entropies")


@pytest.mark.parametrize("A,prec,f16", [(6, "fp32", False), (11, "bf16", True), (18, "fp32", False)])
def test_the_largest_logit_one_fp32_ulp_off_stays_inside_every_bound(A, prec, f16):
    """the bound is not tighter than the forward's: a float32 restatement whose largest logit of every row is the next
    float32 value (either way) passes every check"""
    h, wh, bh, batch, n_mask, opts = engine_standin(_row(A, prec, f16), ALL)
    hd = br.head(h, wh, bh, batch, HYPER, n_mask, **opts)
    z32 = lr.evaluate("heads", h, wh, bh).z32["blas"]
    top = np.argmax(z32[:, :A], axis=1)
    for way in (-np.inf, np.inf):
        moved = z32.copy()
        moved[np.arange(len(top)), top] = np.nextafter(z32[np.arange(len(top)), top], np.float32(way))
        assert (moved != z32).sum() == len(top)
        g32, pl = br.restate_f32(h, wh, bh, batch, HYPER, n_mask, planes=True, z32=moved, **opts)
        assert failed_checks(hd, g32, pl) == []
