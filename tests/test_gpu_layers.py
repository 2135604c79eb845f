"""Every stored activation of the forward pass, layer by layer, against an exact float64 evaluation (pytest -m gpu).

aleppo_forward_activations exports a1, a2, a3 and h.  With the engine's OWN a(l-1) as input, tests/layer_ref.py evaluates
layer l exactly, so nothing propagates and every element gets a bound that follows from the arithmetic (layer_ref's
docstring): (a) every bf16 element inside bf16(relu(z -+ eps)), (b) the per-channel count of elements that differ from
bf16(relu(z)) under four times what the float32 reference evaluations show, (c) every fp32 element within four times the
float32 reference evaluation's own error.  The logits and values of aleppo_forward on the same observations are checked
against the exported fc in the same way.  Scope: the training-side forward kernels (conv_fwd_fused.hpp, conv_patch.hpp,
gemm.hpp, gemm_pipe.hpp and the head forward).  The acting kernels (act_conv_kernel, fc_act_kernel, act_head.hpp) are checked
in the same way, link by link on aleppo_export_acting, by tests/test_gpu_acting.py; tests/test_gpu_shapes.py part B checks
their outputs end to end.

Measured on the MI355X (how much room the kernels really use).  On every bf16 row all routes - fused, three launches,
generic, each with the pipelined and the small-tile fc - gave the same numbers:
    (a) no element outside its interval and no gate off the exact one on any row, layer or route; 72 .. 88 % of the
        intervals are a single value (bit equality).
    (b) worst channel's mismatch count / cap (the float32 evaluations' own worst count in brackets)
                               conv1        conv2       conv3
        n = 1,   H = 32        0/8   (1)    0/8  (0)    0/8  (0)
        n = 37,  H = 96        1/8   (2)    1/8  (1)    1/8  (1)
        n = 260, H = 128       14/40 (10)   5/16 (4)    4/16 (4)     in all 62, 35 and 32 elements of 3 328 000,
        n = 260, H = 32, mod.  5/28  (7)    6/16 (4)    3/16 (4)     1 347 840 and 815 360
        the gap row, step 2    10/44 (11)   4/32 (8)    4/12 (3)
        - the MFMA accumulation flips as many bf16 roundings as a float32 sum on the host does.
    (c) the engine's max |d| / (u Sa) against the float32 evaluation's R, and the worst |d| / bound
                               conv1          conv2          conv3          fc              heads
        bf16 n = 1                                                          0.40/0.46 0.20  0.17/0.43 0.08
        bf16 n = 37                                                         1.56/0.41 0.84  0.56/0.54 0.25
        bf16 n = 260, H = 128                                               1.36/0.36 0.83  0.58/0.62 0.20
        bf16 n = 260, H = 32                                                1.23/0.44 0.62  1.55/1.55 0.21
        fp32 n = 1             2.0/3.1 0.16   3.3/2.0 0.40   2.3/1.8 0.31   1.12/0.37 0.74  0.10/0.55 0.04
        fp32 n = 37            2.9/4.8 0.15   3.6/2.9 0.30   3.8/2.4 0.37   3.44/1.09 0.75  1.15/1.83 0.14
        fp32 n = 260           4.7/4.2 0.27   5.8/5.4 0.27   4.2/3.1 0.32   3.50/1.03 0.82  0.76/0.86 0.22
        - fc (K = 3136) uses three quarters and more of its bound: the device adds its k-steps one after the other, which a
        float32 matmul on the host does not; one sequential fp32 sum (the oracle's) reaches 1.37 of it.
Each case takes under a second on the device's host."""
import functools

import numpy as np
import pytest

import activation_stats_ref as asr
import bf16_check as bc
import hashfill as hf
import layer_ref as lr
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401

pytestmark = pytest.mark.gpu

# route: (OPT_FUSED_FWD, OPT_GENERIC_CONV, OPT_FC_PIPE)
DEFAULT = (("default", (1, 0, 1)),)
THREE = (("fused", (1, 0, 1)), ("three launches", (0, 0, 1)), ("generic", (1, 1, 1)))
SIX = THREE + (("fused, fc small-tile", (1, 0, 0)), ("three launches, fc small-tile", (0, 0, 0)),
               ("generic, fc small-tile", (1, 1, 0)))
# (n, H, A, precision, modified parameters, routes): the smallest shapes at which each route can still go wrong
ROWS = [
    (1, 32, 1, "bf16", False, DEFAULT),    # one sample, fewer samples than any group
    (1, 32, 1, "fp32", False, DEFAULT),
    (37, 96, 6, "bf16", False, THREE),     # ragged against every group size; H % 64 == 32: small-tile fc with a K tail
    (37, 96, 18, "fp32", False, DEFAULT),  # the fp32 generic GEMMs, the widest head
    (260, 128, 6, "bf16", False, SIX),     # past 256: a second sample for four workgroups of the persistent fused loop, the
                                           # W4 conv2 / conv3 variants, the pipelined fc with a ragged last 128-row tile
    (260, 32, 4, "bf16", True, DEFAULT),   # H < 64 keeps the small-tile fc above 256 samples; dead channels
    (260, 64, 4, "fp32", False, DEFAULT),  # fp32 above 256
]


def _id(r):
    return "n%d-H%d-A%d-%s%s" % (r[0], r[1], r[2], r[3], "-modified" if r[4] else "")


def observations(seed, n):
    """hashed byte stacks; sample 0 all zeros and sample 1 all 255 (the dead and the saturated end of conv1's 1/255 scale),
    unless there is one sample only"""
    obs = hf.hf_bytes(seed, (n, 4, 84, 84)).copy()
    if n > 1:
        obs[0] = 0
        obs[1] = 255
    obs.setflags(write=False)
    return obs


@functools.lru_cache(maxsize=None)
def row_inputs(n, H, A, modified):
    """(parameters, observations) of a row, shared with tests/test_layer_ref_cpu.py"""
    seed = 9800 + n + H + A
    params = hf.fill_params(seed, H, A)
    if modified:
        params = asr.modified_params(params, H, A)
    params.setflags(write=False)
    return params, observations(seed + 50, n)


def _set_route(pkg, eng, route):
    for opt, val in zip((pkg.OPT_FUSED_FWD, pkg.OPT_GENERIC_CONV, pkg.OPT_FC_PIPE), route):
        eng.set_option(opt, val)
        assert eng.get_option(opt) == val


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bf16_values(acts):
    for l in ("conv1", "conv2", "conv3"):
        assert not (_bits(acts[l]) & 0xFFFF).any() and acts[l].min() >= 0, l  # bf16 values widened exactly, after the ReLU


@pytest.mark.parametrize("row", ROWS, ids=[_id(r) for r in ROWS])
def test_every_layer_on_the_engines_own_previous_export(pkg, row):
    n, H, A, prec, modified, routes = row
    assert lr.FLOOR_FACTOR == bc.FLOOR_FACTOR
    params, obs = row_inputs(n, H, A, modified)
    bf16 = prec == "bf16"
    eng = pkg.Engine(-(-n // 8), 8, A, H, precision=pkg.BF16 if bf16 else pkg.FP32)
    eng.load_params(params)
    exports, failures, cache = {}, [], {}
    for name, route in routes:
        _set_route(pkg, eng, route)
        acts = exports[name] = eng.forward_activations(obs)
        heads = eng.forward(obs)
        bad, report, _ = lr.check_export(params, H, A, bf16, obs, acts, heads, cache=cache)
        print(lr.summary("layers %s %s:" % (_id(row), name), report))
        failures += ["%s: %s" % (name, f) for f in bad]
        if bf16:
            _assert_bf16_values(acts)
    eng.close()
    assert not failures, failures
    if bf16:  # fused forward and three launches export identical bits, whatever the fc route
        for name, route in routes:
            twin = [m for m, r in routes if r == (0,) + route[1:]]
            if route[0] == 1 and route[1] == 0 and twin:
                for l in ("conv1", "conv2", "conv3", "fc"):
                    assert np.array_equal(_bits(exports[name][l]), _bits(exports[twin[0]][l])), (name, l)


# ------------------------------------------------------------------ the open gap of tests/test_gpu_shapes.py, settled
GAP_ROW = (256, 96, 18, 1)
GAP_SAMPLE, GAP_CHANNEL, GAP_PIXEL = 124, 47, (6, 5)
GAP_A2 = [(124, 31, 6, 7)]   # the a2 elements of that conv3 window that differ from the emulation's a2, and the a1
GAP_A1 = [(124, 10, 12, 16)]  # elements behind them that differ from the emulation's a1


def gap_chain(params, H, A, obs, acts, emu, cache=None):
    """the cause of the gap, from one export `acts` of the second batch and the emulation's activations `emu` on the same
    parameters: failures as strings (none: the cause stands) and the facts found, for printing.

    The chain.  conv1 reads the same bytes on both sides.  An a1 element whose exact z sits within eps of a bf16 rounding
    boundary is stored as the boundary's other neighbour (allowed: its interval has two values).  An a2 element that reads
    it moves with it across a rounding boundary of its own; on the ENGINE's a1 it is exactly where its interval says.  That
    a2 element times its W3 tap moves the conv3 pre-activation of (sample 124, channel 47, pixel (6, 5)), which sits 2.5e-5
    below its gate on the emulation's a2, to above the gate; on the ENGINE's a2 the engine's value is inside its interval."""
    s, c, (py, px) = GAP_SAMPLE, GAP_CHANNEL, GAP_PIXEL
    refs = lr.forward_refs(params, H, A, True, obs, acts, ("conv1", "conv2", "conv3"), cache)
    ivl = {l: lr.interval(refs[l]) for l in refs}
    bad, facts = [], {}

    def inside(l, i):
        return ivl[l][0][i] <= acts[l][i] <= ivl[l][1][i]

    def two_valued(l, i):
        return ivl[l][0][i] != ivl[l][1][i]

    at = (s, c, py, px)
    z_own = float(refs["conv3"].z[at])
    p = lr.split_params(params, H, A, True)
    # the emulation's exact pre-activation there: the same window of ITS a2
    w3 = p["conv3"][0][c].astype(np.float64)
    win_e = acts["conv2"][s, :, py:py + 3, px:px + 3].astype(np.float64)
    win_m = emu["conv2"][s, :, py:py + 3, px:px + 3].astype(np.float64)
    z_emu = float(win_m.ravel() @ w3 + np.float64(p["conv3"][1][c]))
    facts.update(conv3=(float(acts["conv3"][at]), float(emu["conv3"][at])), z_own=z_own, z_emu=z_emu,
                 eps=float(refs["conv3"].eps()[at]))
    if not (acts["conv3"][at] > 0 and emu["conv3"][at] == 0 and z_emu < 0 < z_own):
        bad.append("the gate at %s is not the one described: %r" % (at, facts))
    if not inside("conv3", at):
        bad.append("conv3 %s is outside its interval on the engine's own a2" % (at,))
    a2 = [(s, int(ci), py + int(dy), px + int(dx)) for ci, dy, dx in np.argwhere(win_e != win_m)]
    facts["a2"] = a2
    moved = float((win_e - win_m).ravel() @ w3)
    facts["moved"] = moved
    if not abs((z_own - z_emu) - moved) <= 1e-9 * abs(moved):
        bad.append("the differing a2 elements do not account for the pre-activation's move: %r against %r" % (
            z_own - z_emu, moved))
    a1 = []
    for i in a2:
        if not inside("conv2", i):
            bad.append("a2 %s is outside its interval on the engine's own a1" % (i,))
        _, ci, y, x = i
        patch = np.argwhere(acts["conv1"][s, :, 2 * y:2 * y + 4, 2 * x:2 * x + 4] != emu["conv1"][s, :, 2 * y:2 * y + 4, 2 * x:2 * x + 4])
        behind = [(s, int(cj), 2 * y + int(dy), 2 * x + int(dx)) for cj, dy, dx in patch]
        a1 += [j for j in behind if j not in a1]
        if not behind and not two_valued("conv2", i):
            bad.append("a2 %s differs from the emulation on identical inputs where its interval is a single value" % (i,))
    facts["a1"] = a1
    for j in a1:  # conv1's input is the observation itself: the same on both sides
        if not (two_valued("conv1", j) and inside("conv1", j) and ivl["conv1"][0][j] <= emu["conv1"][j] <= ivl["conv1"][1][j]):
            bad.append("a1 %s: not a rounding flip at a boundary" % (j,))
        # (how close, in units of the error an fp32 sum has: the distance of the exact z from the boundary between the two)
        mid = (float(ivl["conv1"][0][j]) + float(ivl["conv1"][1][j])) / 2
        facts.setdefault("a1_distance", []).append(abs(float(refs["conv1"].z[j]) - mid) / (lr.U * float(refs["conv1"].Sa[j])))
    if a2 != GAP_A2 or a1 != GAP_A1:
        bad.append("the elements are not the ones named: a2 %s, a1 %s" % (a2, a1))
    return bad, facts


def test_the_gap_of_the_every_hidden_size_row_is_a_rounding_flip_in_a1(pkg):
    """row (256, 96, 18, 1) of test_gpu_shapes.test_bf16_every_hidden_size_vs_emulated_oracle, its second step: the same
    parameters and batches, one train(LR, 1, 1) on the first batch, then forward_activations on the second batch's
    observations with the parameters after the step (state_dict), on the fused, three-launch and generic routes.  conv1,
    conv2 and conv3 pass (a) and (b) on the engine's own inputs, and the one conv3 gate that differs from the emulation
    (sample 124, channel 47, pixel (6, 5)) is traced to ONE a1 element, (124, 10, 12, 16), whose exact pre-activation lies
    at a bf16 rounding boundary: gap_chain asserts every link.  A legitimate rounding flip, not a kernel fault."""
    from test_gpu_bf16_emulated import sweep_batch
    from test_gpu_shapes import LR, _second_batch
    N, H, A, pipe = GAP_ROW
    params, *batch1 = sweep_batch(N, H, A)
    obs = _second_batch(N, H, A)[0]
    eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
    eng.set_option(pkg.OPT_FC_PIPE, pipe)
    eng.load_params(params)
    eng.set_batch(*batch1)
    eng.train(LR, 1, 1)
    sd = eng.state_dict()
    assert int(sd["step"]) == 1
    exports = {}
    for name, route in THREE:
        _set_route(pkg, eng, route)
        exports[name] = eng.forward_activations(obs, layers=("conv1", "conv2", "conv3"))
    eng.close()
    emu = asr.from_oracle_acts(orc.net_forward(sd["params"], H, A, obs, want_acts=True, emulate_bf16=True)[2], H)
    cache, failures = {}, []
    for name, acts in exports.items():
        _assert_bf16_values(acts)
        bad, report, _ = lr.check_export(sd["params"], H, A, True, obs, acts, layers=("conv1", "conv2", "conv3"), cache=cache)
        chain, facts = gap_chain(sd["params"], H, A, obs, acts, emu, cache)
        print(lr.summary("gap row %s:" % name, report), "\n    chain", facts)
        failures += ["%s: %s" % (name, f) for f in bad + chain]
    assert not failures, failures
    assert all(np.array_equal(_bits(exports["fused"][l]), _bits(exports["three launches"][l])) for l in exports["fused"])
