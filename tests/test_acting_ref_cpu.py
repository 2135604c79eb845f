"""tests/acting_ref.py, the link-by-link references of the acting path, on the CPU: they have room and they have teeth.

The inputs are the GPU rows' own (tests/test_gpu_acting.py): the (37, 96, 6) bf16 and (37, 96, 18) fp32 rows' parameters and
protocol stacks, the sampler rows' scaled heads and hashed noise, the exact-tie rows, the built-in generator's rows.  A
"device" is emulated link by link with the float32 evaluations layer_ref keeps - the BLAS order and the k-stepped order,
14 steps of 32 for a slice - and with float32 restatements of head_dot (both with and without a contracted multiply-add), of
the softmax / divide / arg-max and of oldlp_kernel.

Room, measured here: the conv links pass (a) and (b) in both float32 orders ((c) on the fp32 row: 0.21 .. 0.39 of the bound);
the k-stepped slices reach 0.22 (bf16 row) and 0.09 (fp32 row) of their (c) bound; head_dot's order 0.18 / 0.18 (two
roundings / contracted) of the head's bound on the bf16 row and 0.10 / 0.12 on the fp32 row, and its binary16 rounding lies
inside every f16 interval; the float32 sampler agrees with the float64 restatement on every draw the gap rule keeps; the
float32 log-softmax in oldlp_kernel's order reaches 0.07 of its bound (A = 4) and less at more actions.
The restatement alone leaves out: 0 of 203 draws on every sampler row; built-in rows 1 of 6156 (seed 123, E 513, A 18) and 0
of 444, 6156 and 3084 on the others - all under 1 %.
Teeth, and the check that catches each (worst |d| / bound, or the count, in brackets):
    one conv2 channel with every weight one bf16 ulp off      (b) on conv2, in that channel only (2793 of its 2997 elements
                                                              against a cap of 8; every weight moves the same way, so at
                                                              this size (a) sees 2566 of them as well)
    one slice's last k-step dropped                           (c) on that slice only (3e5)
    the hidden sum missing one slice / one unit               the head's (c) (6e5 / 1e5; the hidden vector itself is restated
                                                              exactly, so the faulty sum shows in what is computed from it)
    the second half of head_dot dropped for one lane          the head's (c) (7e5), and the f16 interval
    a sampler that takes the last maximum                     the exact-tie rows (the gap rule alone never sees it)"""
import functools

import numpy as np
import pytest

import acting_ref as ar
import activation_stats_ref as asr
import eval_ref as er
import layer_ref as lr
import oracle_lib as orc
from test_gpu_acting import SAMPLER_E, SAMPLER_H, SAMPLER_ROWS

ROWS = {"bf16": (37, 96, 6, True), "fp32": (37, 96, 18, False)}
BUILTIN_ROWS = [(123, 513, 18), (123, 37, 6), (7, 513, 4), (0xDEADBEEF12345678, 257, 1)]


@functools.lru_cache(maxsize=None)
def _device(case):
    """an emulated acting forward of a row: (parameters split, stacks, export dict, float32 logits and values in head_dot's
    order).  The conv activations are the oracle's (float32 sums for the bf16 model), the slices the k-stepped float32
    evaluation of acting_ref's own slice inputs"""
    E, H, A, bf16 = ROWS[case]
    params = ar.row_params(E, H, A)
    stacks = ar.protocol(5000 + E, E, False, 3)[2]
    mode = dict(emulate_bf16=True, sums="float32") if bf16 else {}
    exp = asr.from_oracle_acts(orc.net_forward(params, H, A, stacks, want_acts=True, **mode)[2], H)
    p = lr.split_params(params, H, A, bf16)
    refs = ar.slice_refs(exp["conv3"], p["fc"][0])
    exp = {l: exp[l] for l in ar.CONVS}
    exp["fc_parts"] = np.stack([r.z32["chunks"] for r in refs])
    h = ar.hidden(p["fc"][1], exp["fc_parts"])
    return p, stacks, exp, ar.head_dot_f32(h, *p["heads"], contract=False), h


# ------------------------------------------------------------------ room
@pytest.mark.parametrize("case", list(ROWS))
def test_room_every_link_of_an_emulated_acting_forward(case):
    E, H, A, bf16 = ROWS[case]
    p, stacks, exp, heads, h = _device(case)
    params = ar.row_params(E, H, A)
    failures, report, numbers = ar.check_links(params, H, A, bf16, stacks, exp, heads[:, :A], heads[:, A])
    print(lr.summary("emulated acting forward %s:" % case, report))
    assert not failures, failures
    assert numbers["slices"] <= 0.5 and numbers["head"] <= 0.5
    for l in ar.CONVS:  # both float32 orders of every conv link, on the same stored input
        ref = numbers[l]["ref"]
        for order in ref.z32:
            if bf16:
                got = ref.stored32(order)
                assert not len(lr.interval_check(ref, got)["violations"]) and not len(lr.mismatch_check(ref, got)["failures"])
            else:
                assert lr.fp32_check(ref, ref.act(ref.z32[order]))["worst"] <= 0.5, (l, order)
    ref = ar.head_ref(h, *p["heads"])
    for contract in (False, True):
        got = ar.head_dot_f32(h, *p["heads"], contract=contract)
        bad, worst = ar.check_head(ref, got, False)
        print("head_dot's order, contracted %s: worst |d| / bound %.3g" % (contract, worst))
        assert not bad and worst <= 0.5
        bad, single = ar.check_head(ref, got.astype(np.float16).astype(np.float32), True)
        assert not bad and single >= 0.5, (bad, single)


def _softmax_f32(z):
    z = np.asarray(z, np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    assert e.dtype == np.float32
    return e / e.sum(axis=1, keepdims=True, dtype=np.float32)


@pytest.mark.parametrize("A,regime", SAMPLER_ROWS, ids=["A%d-%s" % r for r in SAMPLER_ROWS])
def test_room_sampler_rows_and_what_the_gap_rule_leaves_out(A, regime):
    E, H = SAMPLER_E, SAMPLER_H
    params, frames, starts, stacks = ar.sampler_case(E, H, A, regime)
    logits = orc.net_forward(params, H, A, stacks)[0]
    q = ar.exp1(6300 + A, (3, E, A))[1]
    got = ar.sample_f32(_softmax_f32(logits), q)
    wrong, left_out, want = ar.sample_check(logits, q, got)
    spread = logits.max(axis=1) - logits.min(axis=1)
    print("sampler A%d %s: spread %.3g .. %.3g, left out %d of %d, actions seen %d" % (
        A, regime, spread.min(), spread.max(), round(left_out * E), E, len(set(want.tolist()))))
    assert not len(wrong) and left_out <= ar.LEFT_OUT_CAP
    if A > 1:
        if regime == "uniform":
            assert len(set(want.tolist())) > 1 and np.median(spread) < 5
        else:
            assert abs(spread.max() - ar.REGIMES[regime]) < 0.01
        if regime == "peaked":
            assert (spread >= 20).mean() >= 0.95
        if regime == "underflow":  # a p below the smallest fp32 normal on a fifth of the rows and more
            assert (np.exp(ar.oldlp_ref(logits)[0]).min(axis=1) < ar.TINY).mean() >= 0.2 and (spread >= 90).mean() >= 0.15
    # oldlp_kernel's order in float32 on the same logits, both plane types
    z = logits.astype(np.float32)
    mx = z.max(axis=1, keepdims=True)
    s = np.zeros((E, 1), np.float32)
    for k in range(A):
        s = s + np.exp(z[:, k:k + 1] - mx)
    lp = z - (mx + np.log(s))
    assert lp.dtype == np.float32
    bad, worst = ar.check_oldlp(logits, lp, False)
    print("old log-probs in oldlp_kernel's order A%d %s: worst |d| / bound %.3g" % (A, regime, worst))
    assert not bad and worst <= 0.5, (bad, worst)
    z16 = z.astype(np.float16).astype(np.float32)  # f16 planes: from the logits as stored
    mx = z16.max(axis=1, keepdims=True)
    lp16 = (z16 - (mx + np.log(np.exp(z16 - mx).sum(axis=1, keepdims=True, dtype=np.float32)))).astype(np.float16)
    bad, _ = ar.check_oldlp(z16, lp16.astype(np.float32), True)
    assert not bad, bad


@pytest.mark.parametrize("seed,E,A", BUILTIN_ROWS, ids=["seed%x-E%d-A%d" % r for r in BUILTIN_ROWS])
def test_room_builtin_rows_at_a_uniform_policy(seed, E, A):
    z = np.zeros((E, A), np.float32)
    left = 0
    seen = set()
    for n in range(12):
        a, gap = er.sample(z, 1.0, ar.act_noise(seed, n, E, A))
        left += int((gap < er.SAMPLE_GAP).sum())
        seen |= set(a.tolist())
    print("built-in seed %x E%d A%d: %d of %d draws within 1e-5 of a tie" % (seed, E, A, left, 12 * E))
    assert left <= ar.LEFT_OUT_CAP * 12 * E and seen == set(range(A))
    assert not np.array_equal(ar.act_noise(seed, 0, E, A), ar.act_noise(seed + 1, 0, E, A))
    assert not np.array_equal(ar.act_noise(seed, 0, E, A), er.eval_noise(seed, 0, E, A, "sample"))  # the lanes' key differs


def test_the_generator_is_philox4x32_10():
    """the published known-answer vectors of Philox4x32-10 (Random123's kat_vectors)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        got = er.philox4x32_10(np.array([c], np.uint32), *k)[0]
        assert tuple(int(x) for x in got) == want


# ------------------------------------------------------------------ teeth
def test_teeth_one_conv2_channel_one_bf16_ulp_off_fails_b_on_conv2():
    p, stacks, exp, _, _ = _device("bf16")
    w, b = p["conv2"]
    ref = lr.evaluate("conv2", exp["conv1"], w, b)
    ch = 23
    off = w.copy()
    bits = off[ch].view(np.uint32)
    assert not (bits & 0xFFFF).any()
    bits += np.uint32(0x10000)  # every weight of the channel to the next bf16 value away from zero
    got = lr.evaluate("conv2", exp["conv1"], off, b).exact_bf16()
    a, m = lr.interval_check(ref, got), lr.mismatch_check(ref, got)
    print("one conv2 channel one ulp off: (a) %d outside; (b) %d mismatches in the channel, cap %d" % (
        len(a["violations"]), m["counts"][ch], m["cap"]))
    assert m["failures"].tolist() == [ch] and np.delete(m["counts"], ch).max() == 0
    assert not len(lr.mismatch_check(ref, exp["conv2"])["failures"])


def test_teeth_one_slices_last_k_step_dropped_fails_c_on_that_slice():
    p, stacks, exp, _, _ = _device("bf16")
    refs = ar.slice_refs(exp["conv3"], p["fc"][0])
    z, n, H = 4, exp["conv3"].shape[0], p["fc"][0].shape[0]
    x = exp["conv3"].transpose(0, 2, 3, 1)[:, z].reshape(n, ar.KC).astype(np.float32)
    w = p["fc"][0].reshape(H, 64, 7, 7).transpose(0, 2, 3, 1)[:, z].reshape(H, ar.KC)
    acc = np.zeros((n, H), np.float32)
    for k0 in range(0, ar.KC - 32, 32):  # 13 of the 14 steps
        acc += x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
    parts = np.array(exp["fc_parts"])
    assert np.abs(acc + x[:, -32:] @ w[:, -32:].T - parts[z]).max() < 1e-5  # (the full sum IS the slice)
    parts[z] = acc
    failures, worst, _ = ar.check_slices(refs, parts)
    print("one slice's last k-step dropped: worst |d| / bound %.3g" % worst)
    assert len(failures) == 1 and failures[0].startswith("fc slice %d " % z) and worst > 100


def test_teeth_a_hidden_sum_missing_a_slice_or_a_unit_and_a_lane_missing_its_second_half_fail_the_head():
    p, stacks, exp, heads, h = _device("bf16")
    ref = ar.head_ref(h, *p["heads"])
    assert not ar.check_head(ref, heads, False)[0]
    short = ar.hidden(p["fc"][1], exp["fc_parts"][:6])  # the last slice never added
    unit = h.copy()
    unit[:, 41] = 0  # one hidden unit never formed
    for name, got in (("slice", ar.head_dot_f32(short, *p["heads"], contract=False)),
                      ("unit", ar.head_dot_f32(unit, *p["heads"], contract=False)),
                      ("lane", ar.head_dot_f32(h, *p["heads"], contract=False, drop_second_half_of_lane=5))):
        bad, worst = ar.check_head(ref, got, False)
        bad16, _ = ar.check_head(ref, got.astype(np.float16).astype(np.float32), True)
        print("head fault %s: worst |d| / bound %.3g" % (name, worst))
        assert bad and worst > 100 and bad16, name


@pytest.mark.parametrize("A", [4, 6, 18])
def test_teeth_a_sampler_that_takes_the_last_maximum_fails_the_tie_rows_only(A):
    bias, probs, q, expected = ar.tie_cases(A)
    n = len(expected)
    uniform = _softmax_f32(np.broadcast_to(bias, (n, A)))
    assert (uniform == uniform[:, :1]).all()  # equal logits: bit-equal p
    for p in (uniform, probs):
        np.testing.assert_array_equal(ar.sample_f32(p, q), expected)
        assert (ar.sample_f32(p, q, last=True) != expected).all()
    if A == 18:
        assert {16, 17} <= set(expected.tolist()) | {17} and (16 in expected)
    # the gap rule alone never sees it: on hashed noise first and last maximum agree
    qh = ar.exp1(77 + A, (203, A))
    ph = _softmax_f32(np.zeros((203, A), np.float32))
    np.testing.assert_array_equal(ar.sample_f32(ph, qh), ar.sample_f32(ph, qh, last=True))
