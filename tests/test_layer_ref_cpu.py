"""tests/layer_ref.py, the per-layer float64 checker, on the CPU oracle: it has room and it has teeth.

Room: the activations of oracle_lib.net_forward(want_acts=True) in all three modes, on two fixtures of
tests/test_gpu_layers.py, each layer on the SAME run's previous layer: the bf16 emulation (double sums) and the emulation
with sequential fp32 sums pass (a) and (b), the plain fp32 oracle passes (c).  Measured here: (a) no element outside and
no gate off in either mode; (b) the double-sum emulation has no mismatch at all, the fp32-sum emulation at the most 1
(n = 37) and 10 of 104 000 (n = 260, conv1) in a channel against caps of 8 and 40; (c) the fp32 oracle's sequential sums
reach 0.56 (n = 37) and 0.76 (n = 260) of the bound on fc (K = 3136), 0.17 .. 0.38 on the conv layers.  The fp32-sum
emulation's fc is NOT held to (c): its one sequential fp32 sum over 3136 terms is 2.3 u Sa off where the blocked order of
a float32 matmul is 0.38, which is 1.37 of the bound at n = 37 - (c) is that tight.
Teeth: one stored element moved to the next bf16 value, one conv3 tap zeroed, one conv3 tap one bf16 ulp off, one fc
term dropped, and the plain fp32 oracle against the bf16 model each fail the check meant for them.
The inputs: every conv layer has 25 % .. 75 % of its elements active and at least half of the intervals of (a) are a
single value, so that the fixtures cannot drift into a regime where the checks say nothing."""
import functools

import numpy as np
import pytest

import activation_stats_ref as asr
import bf16_check as bc
import layer_ref as lr
import oracle_lib as orc
from test_gpu_layers import row_inputs

# (n, H, A, modified parameters) of tests/test_gpu_layers.ROWS
FIXTURES = {"n37": (37, 96, 6, False), "n260": (260, 128, 6, False)}
MODES = dict(bf16=dict(emulate_bf16=True), floor=dict(emulate_bf16=True, sums="float32"), fp32={})
CONVS = ("conv1", "conv2", "conv3")


@functools.lru_cache(maxsize=None)
def _oracle(case, mode):
    """(export dict, (logits, values)) of the oracle in a mode; computed once, read-only"""
    n, H, A, modified = FIXTURES[case]
    params, obs = row_inputs(n, H, A, modified)
    logits, values, acts = orc.net_forward(params, H, A, obs, want_acts=True, **MODES[mode])
    out = asr.from_oracle_acts(acts, H)
    for a in out.values():
        a.setflags(write=False)
    return out, (logits, values)


@functools.lru_cache(maxsize=None)
def _checked(case, mode):
    """lr.check_export of the oracle's run against the model of its own precision"""
    n, H, A, modified = FIXTURES[case]
    params, obs = row_inputs(n, H, A, modified)
    acts, heads = _oracle(case, mode)
    if mode == "floor":  # (a) and (b) only: see the module docstring on its fc
        return lr.check_export(params, H, A, True, obs, acts, layers=CONVS)
    if mode == "fp32":  # the four exported layers; its heads are sequential sums again (0.54 and 0.99 of the bound here)
        return lr.check_export(params, H, A, False, obs, acts)
    return lr.check_export(params, H, A, True, obs, acts, heads)


def test_the_margin_is_the_bf16_checkers():
    assert lr.FLOOR_FACTOR == bc.FLOOR_FACTOR and lr.U == 2.0 ** -24
    assert lr.SCALE1 == float(np.float32(1.0) / np.float32(255.0))


# ------------------------------------------------------------------ room
@pytest.mark.parametrize("mode", ["bf16", "floor", "fp32"])
@pytest.mark.parametrize("case", list(FIXTURES))
def test_room_every_oracle_mode_passes_its_checks_layer_by_layer(case, mode):
    failures, report, results = _checked(case, mode)
    print(lr.summary("oracle %s %s:" % (mode, case), report))
    assert not failures, failures
    if mode == "fp32":
        assert all("c" in results[l] for l in lr.LAYERS)
    else:
        for l in CONVS:
            assert results[l]["a"]["gates"] == 0, l  # no gate disagreement at all
    if mode == "bf16":  # the double-sum emulation IS bf16(relu(z)), but for the float64 sums' own rounding
        assert sum(int(results[l]["b"]["counts"].sum()) for l in CONVS) <= 1


@pytest.mark.parametrize("case", list(FIXTURES))
def test_the_inputs_are_not_in_a_trivial_regime(case):
    _, _, results = _checked(case, "bf16")
    for l in CONVS:
        a = results[l]["a"]
        print("%s %s: active %.3f, single-valued intervals %.3f" % (case, l, a["active"], a["single"]))
        assert 0.25 <= a["active"] <= 0.75, (l, a["active"])
        assert a["single"] >= 0.5, (l, a["single"])


# ------------------------------------------------------------------ teeth
CASE = "n37"


def _setup():
    n, H, A, modified = FIXTURES[CASE]
    params, obs = row_inputs(n, H, A, modified)
    acts, _ = _oracle(CASE, "bf16")
    return params, obs, acts, H, A, _checked(CASE, "bf16")[2]


def test_teeth_one_element_moved_to_the_next_bf16_value_fails_a():
    params, obs, acts, H, A, results = _setup()
    for l in CONVS:
        ref = results[l]["ref"]
        lo, hi = lr.interval(ref)
        single = np.argwhere((lo == hi) & (lo > 0))  # where the interval is a single positive value: one in the middle
        i = tuple(single[len(single) // 2])
        for up in (True, False):
            moved = np.array(acts[l])
            moved[i] = lr.next_bf16(np.array([moved[i]]), up)[0]
            assert moved[i] != acts[l][i] and abs(moved[i] / acts[l][i] - 1) <= 2.0 ** -7
            a = lr.interval_check(ref, moved)
            assert a["violations"].tolist() == [list(i)], (l, up)
        assert not len(lr.interval_check(ref, acts[l])["violations"])


def _conv3_with(params, H, A, acts, change):
    """the emulation's stored conv3 (bf16(relu(z)) on the oracle's a2) with `change` applied to the bf16 weights [64, 576]"""
    w, b = lr.split_params(params, H, A, True)["conv3"]
    w = w.copy()
    change(w)
    return lr.evaluate("conv3", acts["conv2"], w, b).exact_bf16()


def _tap(params, H, A, acts, channel):
    """the tap of a conv3 output channel that carries the most: the largest |w| sum |x|"""
    w, _ = lr.split_params(params, H, A, True)["conv3"]
    cols, _ = lr.im2col(acts["conv2"], 3, 1, np.float64)
    return int(np.argmax(np.abs(w[channel]) * np.abs(cols).sum(axis=0)))


def test_teeth_one_conv3_tap_zeroed_fails_a():
    params, obs, acts, H, A, results = _setup()
    ref, ch = results["conv3"]["ref"], 11
    k = _tap(params, H, A, acts, ch)

    def zero(w):
        w[ch, k] = 0
    got = _conv3_with(params, H, A, acts, zero)
    a = lr.interval_check(ref, got)
    print("one conv3 tap zeroed: %d elements outside their interval" % len(a["violations"]))
    assert len(a["violations"]) >= 100 and set(a["violations"][:, 1].tolist()) == {ch}


def test_teeth_one_conv3_tap_one_bf16_ulp_off_fails_b_in_its_channel_only():
    params, obs, acts, H, A, results = _setup()
    ref, ch = results["conv3"]["ref"], 11
    k = _tap(params, H, A, acts, ch)

    def nudge(w):
        bits = w[ch, k:k + 1].view(np.uint32)
        assert not bits[0] & 0xFFFF
        bits += np.uint32(0x10000)  # the next bf16 value away from zero
    got = _conv3_with(params, H, A, acts, nudge)
    a, b = lr.interval_check(ref, got), lr.mismatch_check(ref, got)
    print("one conv3 tap one bf16 ulp off: %d outside their interval, %d mismatches in channel %d of %d elements, cap %d; "
          "the other channels %d" % (len(a["violations"]), b["counts"][ch], ch, ref.z.size // 64, b["cap"],
                                     np.delete(b["counts"], ch).max()))
    assert b["failures"].tolist() == [ch] and b["counts"][ch] > 4 * b["cap"]
    assert np.delete(b["counts"], ch).max() == 0


def test_teeth_one_fc_term_dropped_fails_c():
    params, obs, acts, H, A, results = _setup()
    ref, row, sample = results["fc"]["ref"], 5, 17
    w, b = lr.split_params(params, H, A, True)["fc"]
    x = acts["conv3"].reshape(acts["conv3"].shape[0], -1).astype(np.float64)
    k = int(np.argmax(np.abs(x[sample] * w[row])))
    got = np.array(acts["fc"])
    assert not len(lr.fp32_check(ref, got)["violations"])
    got[sample, row] = np.float32(ref.z[sample, row] - x[sample, k] * float(w[row, k]))  # exact, but for one term
    c = lr.fp32_check(ref, got)
    print("one fc term dropped: |d| / bound %.3g" % c["worst"])
    assert c["violations"].tolist() == [[sample, row]]


def test_teeth_the_fp32_oracle_fails_a_against_the_bf16_model():
    n, H, A, modified = FIXTURES[CASE]
    params, obs = row_inputs(n, H, A, modified)
    acts, _ = _oracle(CASE, "fp32")
    refs = lr.forward_refs(params, H, A, True, obs, acts, CONVS)
    for l in CONVS:
        a = lr.interval_check(refs[l], acts[l])
        print("fp32 oracle against the bf16 model, %s: %d of %d outside" % (l, len(a["violations"]), acts[l].size))
        assert len(a["violations"]) > 0.25 * acts[l].size, l
