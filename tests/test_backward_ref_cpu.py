"""tests/backward_ref.py, the per-layer float64 checker of the backward pass, on the CPU oracle: room and teeth.

Room: the oracle's three modes (oracle_lib.net_forward / ppo_loss / net_backward(want_stored=True): the fp32 restatement,
the bf16 emulation with double sums and the same with sequential fp32 sums) stand in for the engine on the inputs of the
rows of tests/test_gpu_backward.py, a bf16 row in the two emulated modes and an fp32 row in the plain one; every check
passes, each layer on the SAME run's stored tensors.  The per-layer references, composed into a chain, reproduce the
emulation's gradients to the 1e-5 at which tests/test_oracle_bf16.py pins it.  A float32 numpy restatement of the head's
formulas stays within 1 / FLOOR_FACTOR of the allowance delta on every row's inputs.
Teeth: each planted error fails its own check, and no check of a layer in front of it."""
import functools

import numpy as np
import pytest

import activation_stats_ref as asr
import backward_ref as br
import bf16_check as bc
import layer_ref as lr
import oracle_lib as orc
from test_gpu_backward import HYPER, ROWS, STALE, _id, row_batch, take

MODES = dict(bf16=dict(emulate_bf16=True), floor=dict(emulate_bf16=True, sums="float32"), fp32={})
# the order of the backward pass: a planted error may fail checks from its layer on, never one in front of it
ORDER = ("dfc", "heads.w", "heads.b", "dconv3", "fc.w", "fc.b", "dconv2", "conv3.w", "conv3.b", "dconv1", "conv2.w",
         "conv2.b", "conv1.w", "conv1.b", "masked")
CASE = "n37-H96-A6-bf16"  # the teeth's
CASES = {_id(r): r for r in ROWS}
CASES["n37-H96-A6-bf16-second-of-74"] = (37, STALE[1], STALE[2], "bf16", False, None, None)


def _inputs(case):
    n, H, A, prec, modified, _, only = CASES[case]
    if case.endswith("second-of-74"):  # minibatch 1 of the N = 74, M = 2 rows
        params, obs, batch = row_batch(STALE[0], H, A, False)
        idx = np.arange(37, 74)
        return params, obs[idx], take(batch, idx), H, A, prec == "bf16", only
    params, obs, batch = row_batch(n, H, A, modified)
    return params, obs, batch, H, A, prec == "bf16", only


def oracle_run(params, H, A, obs, batch, mode, n_mask=0.0, hyper=HYPER, masks=None):
    """(export dict, grads) of one minibatch on the oracle in `mode`; n_mask / hyper / masks: what a planted error changes"""
    logits, values, acts = orc.net_forward(params, H, A, obs, want_acts=True, **MODES[mode])
    o = orc.ppo_loss(logits, batch["old_lp"], batch["actions"], batch["adv"], values, batch["ret"],
                     batch["masks"] if masks is None else masks, hyper["clip"], hyper["c_v"], hyper["c_e"], n_mask)
    grads, stored = orc.net_backward(params, H, A, acts, o["dlogits"], o["dvalues"], want_stored=True, **MODES[mode])
    exp = dict(asr.from_oracle_acts(acts, H), **stored)
    return exp, grads


@functools.lru_cache(maxsize=None)
def _oracle(case, mode):
    params, obs, batch, H, A, bf16, only = _inputs(case)
    exp, grads = oracle_run(params, H, A, obs, batch, mode)
    for a in list(exp.values()) + [grads]:
        a.setflags(write=False)
    return exp, grads


_CACHES = {}  # per case: references whose inputs have the same bytes are evaluated once (check_backward's cache)


def _check(case, exp, grads):
    params, obs, batch, H, A, bf16, only = _inputs(case)
    cache = _CACHES.setdefault((case, bf16), {}) if case == CASE else None
    return br.check_backward(params, H, A, bf16, obs, batch, HYPER, int(batch["masks"].sum()), exp, grads, cache, only)


def _failed(failures):
    """the names of the checks that failed, in the order of the backward pass"""
    names = {f.split(" ")[0].rstrip(":") for f in failures}
    assert names <= set(ORDER), names
    return [n for n in ORDER if n in names]


def test_the_margin_is_the_forward_checkers():
    assert br.FLOOR_FACTOR == bc.FLOOR_FACTOR == lr.FLOOR_FACTOR and br.U == 2.0 ** -24 and br.SCALE1 == lr.SCALE1


# ------------------------------------------------------------------ room
ROOM = [(c, m) for c, r in CASES.items() for m in (("bf16", "floor") if r[3] == "bf16" else ("fp32",))]


@pytest.mark.parametrize("case,mode", ROOM, ids=["%s-%s" % cm for cm in ROOM])
def test_room_every_oracle_mode_passes_every_check(case, mode):
    exp, grads = _oracle(case, mode)
    failures, report, results = _check(case, exp, grads)
    print(br.summary("oracle %s %s:" % (mode, case), report))
    assert not failures, failures
    if mode == "bf16" and CASES[case][6] is None:  # the double-sum emulation IS bf16(gate z): no mismatch to speak of
        assert sum(int(results[d]["b"]["counts"].sum()) for d in ("dconv3", "dconv2", "dconv1")) <= 1


def test_the_inputs_are_not_in_a_trivial_regime():
    """both branches of the clip select, both signs of the advantage, masked rows, open and closed gates, and intervals that
    are mostly a single value"""
    case = "n37-H96-A6-bf16"
    params, obs, batch, H, A, bf16, _ = _inputs(case)
    exp, grads = _oracle(case, "bf16")
    _, _, results = _check(case, exp, grads)
    hd = results["head"]["head"]
    live = batch["masks"] != 0
    active = np.where(batch["adv"] >= 0, hd.rho <= 1.1, hd.rho >= 0.9)
    assert 0.2 <= active[live].mean() <= 0.8 and 0.3 <= (batch["adv"] > 0).mean() <= 0.7 and (~live).sum() == 5
    for d in ("dconv3", "dconv2", "dconv1"):
        r = results[d]
        open_ = float(r["ref"].gate.mean())
        print("%s: gates open %.3f, single-valued intervals %.3f" % (d, open_, r["single"]))
        assert 0.25 <= open_ <= 0.75 and r["single"] >= 0.5, d


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_restatement_of_the_head_stays_within_a_quarter_of_delta(case):
    params, obs, batch, H, A, bf16, _ = _inputs(case)
    h = _oracle(case, "bf16" if bf16 else "fp32")[0]["fc"]
    wh, bh = lr.split_params(params, H, A, bf16)["heads"]
    n_mask = int(batch["masks"].sum())
    hd = br.head(h, wh, bh, batch, HYPER, n_mask)
    g32 = br.restate_f32(h, wh, bh, batch, HYPER, n_mask)
    d = np.abs(g32.astype(np.float64) - hd.g)
    live = batch["masks"] != 0
    assert not d[~live].any() and not hd.delta[~live].any()
    assert (hd.delta[live] > 0).all()
    worst = float((d[live] / hd.delta[live]).max())
    print("%s: float32 restatement of g, worst |d| / delta %.3g; delta / |g| median %.3g" % (
        case, worst, float(np.median(hd.delta[live] / np.maximum(np.abs(hd.g[live]), 1e-300)))))
    assert worst <= 1.0 / br.FLOOR_FACTOR


def test_room_the_composed_references_reproduce_the_emulated_gradients():
    case = "n37-H96-A6-bf16"
    params, obs, batch, H, A, bf16, _ = _inputs(case)
    logits, values, acts = orc.net_forward(params, H, A, obs, want_acts=True, emulate_bf16=True)
    o = orc.ppo_loss(logits, batch["old_lp"], batch["actions"], batch["adv"], values, batch["ret"], batch["masks"],
                     HYPER["clip"], HYPER["c_v"], HYPER["c_e"])
    want = orc.net_backward(params, H, A, acts, o["dlogits"], o["dvalues"], emulate_bf16=True)
    a = asr.from_oracle_acts(acts, H)
    p = lr.split_params(params, H, A, True)
    g = np.concatenate([o["dlogits"], o["dvalues"][:, None]], axis=1).astype(np.float64)
    wh = p["heads"][0].astype(np.float64)
    got = {"heads": ((g.T @ a["fc"].astype(np.float64)), g.sum(axis=0))}
    dz = orc.round_bf16((g @ wh).astype(np.float32)).reshape(len(g), H)  # dh
    x_of = dict(fc="conv3", conv3="conv2", conv2="conv1", conv1="obs")
    src = dict(a, obs=obs)
    for layer in ("fc", "conv3", "conv2", "conv1"):
        W, b = br.wgrad(layer, dz, src[x_of[layer]])
        got[layer] = (W.z, b.z)
        if layer != "conv1":
            dz = br.dgrad(layer, dz, p[layer][0], a[x_of[layer]]).exact_bf16()
    flat = np.concatenate([np.concatenate([got[l][0].ravel(), got[l][1].ravel()]) for l in ("conv1", "conv2", "conv3", "fc")]
                          + [got["heads"][0][:A].ravel(), got["heads"][1][:A], got["heads"][0][A:].ravel(), got["heads"][1][A:]])
    offs = orc.param_offsets(H, A)
    for k, nm in enumerate(bc.NAMES):
        r = bc.rel(flat[offs[k]:offs[k + 1]].astype(np.float32), want[offs[k]:offs[k + 1]])
        print("%-9s %.3g" % (nm, r))
        assert r <= 1e-5, nm


# ------------------------------------------------------------------ teeth


def _setup():
    exp, grads = _oracle(CASE, "bf16")
    failures, _, results = _check(CASE, exp, grads)
    assert not failures
    return _inputs(CASE), dict(exp), np.array(grads), results


def _assert_fails_from(failures, own, first=None):
    failed = _failed(failures)
    print("failed:", failed)
    assert own in failed, (own, failed)
    assert ORDER.index(failed[0]) >= ORDER.index(first or own), failed


def _next_bf16(x, up):
    b = np.array([x], np.float32).view(np.uint32)
    return (b + np.uint32(0x10000) if up else b - np.uint32(0x10000)).view(np.float32)[0]


@pytest.mark.parametrize("name", ["dfc", "dconv3", "dconv2", "dconv1"])
def test_teeth_one_stored_gradient_element_one_bf16_value_off(name):
    """the element is an OUTPUT of its own layer's check, which names it, and an input of the next ones"""
    (params, obs, batch, H, A, bf16, _), exp, grads, results = _setup()
    ref = results[name]["ref"]
    lo, hi = br.interval(ref)
    single = np.argwhere((lo == hi) & (lo != 0))
    i = tuple(int(j) for j in single[len(single) // 2])
    for up in (True, False):
        moved = np.array(exp[name])
        moved[i] = _next_bf16(moved[i], up)
        assert moved[i] != exp[name][i]
        failures, _, _ = _check(CASE, dict(exp, **{name: moved}), grads)
        assert any(f.startswith(name + " (a): 1 elements") and str(i) in f for f in failures), failures
        _assert_fails_from(failures, name)


def _dgrad_with(X, exp, params, H, A, change):
    wl, src, dst, gate = br.DGRAD[X]
    w = lr.split_params(params, H, A, True)[wl][0].copy()
    change(w)
    return dst, br.dgrad(X, exp[src], w, exp[gate]).exact_bf16()


def _tap(exp, params, H, A, oc):
    """the conv3 tap (of output channel oc) that carries the most in the dgrad"""
    w = lr.split_params(params, H, A, True)["conv3"][0]
    return int(np.argmax(np.abs(w[oc]))), int(np.argmax(np.abs(w[oc]))) // 9


def test_teeth_one_dgrad_tap_zeroed_fails_a_and_nothing_before():
    (params, obs, batch, H, A, bf16, _), exp, grads, _ = _setup()
    k, cin = _tap(exp, params, H, A, 11)

    def zero(w):
        w[11, k] = 0
    dst, got = _dgrad_with("conv3", exp, params, H, A, zero)
    failures, _, res = _check(CASE, dict(exp, **{dst: got}), grads)
    bad = res[dst]["violations"]
    print("one conv3 dgrad tap zeroed: %d elements outside their interval" % len(bad))
    assert len(bad) >= 20 and set(bad[:, 1].tolist()) == {cin}
    _assert_fails_from(failures, "dconv2")


def test_teeth_one_dgrad_tap_one_bf16_ulp_off_fails_b_in_its_channel_only():
    (params, obs, batch, H, A, bf16, _), exp, grads, _ = _setup()
    k, cin = _tap(exp, params, H, A, 11)

    def nudge(w):
        bits = w[11, k:k + 1].view(np.uint32)
        assert not bits[0] & 0xFFFF
        bits += np.uint32(0x10000)
    dst, got = _dgrad_with("conv3", exp, params, H, A, nudge)
    failures, _, res = _check(CASE, dict(exp, **{dst: got}), grads)
    b = res[dst]["b"]
    print("one conv3 dgrad tap one bf16 ulp off: %d mismatches in channel %d, cap %d; the other channels %d" % (
        b["counts"][cin], cin, b["cap"], np.delete(b["counts"], cin).max()))
    assert b["failures"].tolist() == [cin] and np.delete(b["counts"], cin).max() == 0
    _assert_fails_from(failures, "dconv2")


@pytest.mark.parametrize("X", ["fc", "conv3", "conv2"])
def test_teeth_the_gate_read_one_pixel_over(X):
    (params, obs, batch, H, A, bf16, _), exp, grads, results = _setup()
    wl, src, dst, gate = br.DGRAD[X]
    ref = results[dst]["ref"]
    got = orc.round_bf16(np.where(np.roll(ref.gate, 1, axis=-1), ref.z, 0.0).astype(np.float32)).reshape(ref.z.shape)
    failures, _, res = _check(CASE, dict(exp, **{dst: got}), grads)
    assert res[dst]["leak"] > 0
    _assert_fails_from(failures, dst)


@pytest.mark.parametrize("layer", ["fc", "conv3", "conv2", "conv1"])
def test_teeth_one_sample_dropped_and_one_slab_counted_twice(layer):
    (params, obs, batch, H, A, bf16, _), exp, grads, _ = _setup()
    dzn, xn = br.WGRAD[layer]
    src = dict(exp, obs=obs)
    offs = orc.param_offsets(H, A)
    k = 2 * ("conv1", "conv2", "conv3", "fc").index(layer)
    for what, rows, sign in (("one sample dropped", slice(17, 18), -1.0), ("a slab of 8 samples counted twice", slice(8, 16), 1.0)):
        W, b = br.wgrad(layer, exp[dzn][rows], src[xn][rows])
        g = np.array(grads)
        g[offs[k]:offs[k + 1]] = (g[offs[k]:offs[k + 1]].astype(np.float64) + sign * W.z.ravel()).astype(np.float32)
        g[offs[k + 1]:offs[k + 2]] = (g[offs[k + 1]:offs[k + 2]].astype(np.float64) + sign * b.z).astype(np.float32)
        failures, _, res = _check(CASE, exp, g)
        print("%s, %s: worst |d| / bound %.3g (weights), %.3g (bias)" % (
            layer, what, res[layer + ".w"]["c"]["worst"], res[layer + ".b"]["c"]["worst"]))
        assert _failed(failures) == [layer + ".w", layer + ".b"], failures


@pytest.mark.parametrize("layer", ["conv3", "conv2", "conv1"])
def test_teeth_a_bias_gradient_summed_from_the_unrounded_dz(layer):
    (params, obs, batch, H, A, bf16, _), exp, grads, results = _setup()
    dzn, _ = br.WGRAD[layer]
    ref = results[dzn]["ref"]
    unrounded = ref.act(ref.z).sum(axis=(0, 2, 3))
    offs = orc.param_offsets(H, A)
    k = 2 * ("conv1", "conv2", "conv3", "fc").index(layer) + 1
    g = np.array(grads)
    g[offs[k]:offs[k + 1]] = unrounded.astype(np.float32)
    failures, _, res = _check(CASE, exp, g)
    print("%s bias from the unrounded dz: worst |d| / bound %.3g" % (layer, res[layer + ".b"]["c"]["worst"]))
    assert _failed(failures) == [layer + ".b"], failures


def test_teeth_a_masked_sample_let_in():
    (params, obs, batch, H, A, bf16, _), _, _, _ = _setup()
    masks = np.array(batch["masks"])
    s = int(np.flatnonzero(masks == 0)[2])
    masks[s] = 1  # the stand-in trains on it, with the right N_mask; the batch says it is masked
    exp, grads = oracle_run(params, H, A, obs, batch, "bf16", n_mask=float(batch["masks"].sum()), masks=masks)
    failures, _, _ = _check(CASE, exp, grads)
    assert any("sample %d is masked" % s in f for f in failures)
    _assert_fails_from(failures, "dfc")
    assert "masked" in _failed(failures)


def test_teeth_conv1s_scale_missing():
    (params, obs, batch, H, A, bf16, _), exp, grads, _ = _setup()
    offs = orc.param_offsets(H, A)
    g = np.array(grads)
    g[offs[0]:offs[1]] *= np.float32(255.0)
    failures, _, _ = _check(CASE, exp, g)
    assert _failed(failures) == ["conv1.w"], failures


@pytest.mark.parametrize("what", ["the value coefficient dropped", "N_mask off by one"])
def test_teeth_the_head(what):
    (params, obs, batch, H, A, bf16, _), _, _, _ = _setup()
    if what == "N_mask off by one":
        exp, grads = oracle_run(params, H, A, obs, batch, "bf16", n_mask=float(batch["masks"].sum()) + 1.0)
    else:
        exp, grads = oracle_run(params, H, A, obs, batch, "bf16", hyper=dict(HYPER, c_v=1.0))
    failures, _, res = _check(CASE, exp, grads)
    failed = _failed(failures)
    print(what, "->", failed)
    # the stand-in's own layers behind the head are consistent with its (wrong) dh: only the head's checks fail
    assert failed == ["dfc", "heads.w", "heads.b"], failures
    if what != "N_mask off by one":  # ... and in the weight gradient only the value row
        assert set(res["heads.w"]["c"]["violations"][:, 0].tolist()) == {A}
