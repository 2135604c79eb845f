"""Every stored gradient of the backward pass, layer by layer, against an exact float64 evaluation (pytest -m gpu).

aleppo_export_backward gives what the last minibatch of an update left: a1, a2, a3, h, dh, dz3, dz2 and - where the route
stores it - dz1; aleppo_export_grads gives that minibatch's gradient.  With the engine's OWN stored tensors as inputs,
tests/backward_ref.py evaluates each backward layer exactly, so nothing propagates and every element gets a bound that
follows from the arithmetic (backward_ref's docstring): the head's dh / dWh / dbh from the exported h, each data gradient
(a) inside bf16(gate (z -+ eps)) and (b) with a per-channel mismatch count under four times the float32 evaluations', each
weight and bias gradient (c) within four times the float32 evaluations' own error, fp32 contexts (c) throughout.  Masked
samples must leave exact zeros.  The update is train(lr = 0): the parameters stay bit-identical (asserted), so every
minibatch sees the loaded ones; the gradient-norm limit is 1e30, so the clip factor is exactly 1 (asserted).

Routes: ALEPPO_OPT_FUSED_BWD 0 / 2 x ALEPPO_OPT_GENERIC_CONV 0 / 1 x ALEPPO_OPT_FC_PIPE 0 / 1.  Which routes must export
the same bits, settled by reading api_train.hip: ALEPPO_OPT_FUSED_BWD only chooses the tail after conv3's dgrad, so two
routes that differ in it alone run the same launches up to dz2 and the same head, fc and conv3 weight-gradient kernels -
a1, a2, a3, h, dh, dz3, dz2 and the head / fc / conv3 gradients are equal bit for bit (and, with the generic convolutions,
which have no fused tail, everything is).  ALEPPO_OPT_FC_PIPE only chooses fc kernels: a1, a2, a3 are equal bit for bit.

Measured on the MI355X (how much room the kernels really use).  Within a row every route gave the same picture:
    (a) no element outside its interval and nothing non-zero behind a closed gate on any row, layer or route.  Share of
        single-valued intervals (bit equality):       dh       dz3      dz2      dz1
        n = 1,   H = 32                               1.000    0.986    0.814    0.907
        n = 37,  H = 96, 8 routes                     0.970    0.952    0.847    0.922
        n = 260, H = 128, 8 routes                    0.980    0.936    0.886    0.922
        n = 260, H = 32, dead channels                0.994    0.991    0.875    0.920
        n = 520, H = 128                              0.973    0.943
        N = 74, M = 2, contiguous / shuffled          0.984 / 0.981   0.949 / 0.950   0.845   0.935
    (b) worst channel's mismatch count / cap (the float32 evaluations' own worst count in brackets)
                                       dz3        dz2        dz1
        n = 1                          0/8  (0)   0/8  (1)   1/8  (1)
        n = 37                         1/8  (1)   1/8  (2)   1/8  (2)
        n = 260, H = 128               2/12 (3)   3/12 (3)   5/24 (6)     in all 15, 24 elements of 815 360, 1 347 840
        n = 260, H = 32, dead channels 4/16 (4)   3/12 (3)   8/28 (7)     18, 27 and 61 of 3 328 000
        n = 520                        3/16 (4)
        N = 74, M = 2                  1/8  (2)   1/8  (1)   1/8  (2)
    (c) worst |d| / bound over a row's routes
                          dWh   dbh   fc.w  fc.b  conv3.w conv3.b conv2.w conv2.b conv1.w conv1.b
        bf16 n = 1        0.10  0.09  0     0     0.14    0       0.21    0       0.31    0.10
        bf16 n = 37       0.03  0.01  0.15  0     0.15    0.16    0.16    0.13    0.30    0.16
        bf16 n = 260      0.02  0.02  0.32  0.16  0.19    0.12    0.20    0.20    0.23    0.30
        bf16 n = 260 dead 0.03  0.01  0.27  0.13  0.16    0.09    0.20    0.12    0.27    0.48
        bf16 n = 520      0.02  0.00  0.17  0.14
        bf16 N = 74 cont. 0.06  0.01  0.21  0     0.18    0.15    0.23    0.17    0.20    0.14
        bf16 N = 74 shuf. 0.05  0.01  0.25  0     0.20    0.22    0.18    0.19    0.29    0.09
        fp32 n = 1        0.14  0.13  0.17  0     0.22    0.18    0.21    0.14    0.13    0.08   dh 0.13 dz3 0.26 dz2 0.61 dz1 0.22
        fp32 n = 37       0.01  0.01  0.25  0.24  0.18    0.14    0.21    0.19    0.15    0.11   dh 0.02 dz3 0.26 dz2 0.39 dz1 0.37
        fp32 n = 260      0.03  0.00  0.39  0.14  0.19    0.12    0.16    0.19    0.18    0.17   dh 0.11 dz3 0.24 dz2 0.37 dz1 0.29
        - the conv1 columns are the routes that store dz1.  On the fused tail, whose dz1 never reaches memory, the allowance
        of the two-valued intervals is 200 .. 1000 times the fp32 bound at n = 37 and 260 (conv1.w 0.005 and 0.0009 of the
        widened bound): there the check sees a dropped sample or a missing scale, not a rounding.  What closes that gap is
        _fused_tail_on_the_stored_dz1: the fused tail's dW1 / db1 under (c) with NO allowance on the dz1 its three-launch
        twin stored (n = 37: 1.2 u Sa against R 0.9, where the evaluation on bf16(gate z) shows 46 u Sa - one dz1 element on
        a rounding boundary).  Worst |d| / bound of that check: conv1.w 0.28 (n = 37), 0.24 (n = 260), 0.24 / 0.29
        (N = 74 contiguous / shuffled); conv1.b 0.09 .. 0.18.
    The routes agreed as asserted (the equalities above), and the captured update exported the eager update's bits.
Each case takes under 4 seconds, most under half a second."""
import functools

import numpy as np
import pytest

import backward_ref as br
import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401
from test_gpu_layers import row_inputs

pytestmark = pytest.mark.gpu

HYPER = dict(clip=0.1, c_v=0.5, c_e=0.01)  # the Engine's defaults
MAX_NORM = 1e30
# route: (OPT_FUSED_BWD, OPT_GENERIC_CONV, OPT_FC_PIPE); None: the context's defaults
DEFAULT = (("default", None),)
ALL = tuple(("%s, %s, fc %s" % ("fused tail" if f else "three launches", "generic" if g else "patch",
                                "pipelined" if p else "small-tile"), (f, g, p))
            for f in (2, 0) for g in (0, 1) for p in (1, 0))
PAIR = (("fused tail", (2, 0, 1)), ("three launches", (0, 0, 1)))
FC_HEAD = ("head", "dfc", "heads.w", "heads.b", "dconv3", "fc.w", "fc.b")
# (n, H, A, precision, modified parameters, routes, the checks to run (None: all)): the smallest shapes at which each route
# can still go wrong
ROWS = [
    (1, 32, 1, "bf16", False, DEFAULT, None),      # one sample, fewer than any group
    (1, 32, 1, "fp32", False, DEFAULT, None),
    (37, 96, 6, "bf16", False, ALL, None),         # ragged against every tile; H % 64 == 32: the K-tail fc dgrad, partial-M fc wgrad
    (37, 96, 18, "fp32", False, DEFAULT, None),    # the generic fp32 GEMMs, the widest head
    (260, 128, 6, "bf16", False, ALL, None),       # past 256: a second sample for four workgroups of the fused tail and of the
                                                   # patch wgrads; the pipelined fc with a ragged last tile
    (260, 32, 4, "bf16", True, DEFAULT, None),     # dead channels: whole planes of closed gates
    (260, 64, 4, "fp32", False, DEFAULT, None),    # fc wgrad in two split-K slices (260 / (4 * 32))
    (520, 128, 6, "bf16", False, DEFAULT, FC_HEAD),  # fc wgrad in two slices (520 / (4 * 64)); fc and head layers only
]


def _id(r):
    return "n%d-H%d-A%d-%s%s" % (r[0], r[1], r[2], r[3], "-modified" if r[4] else "")


@functools.lru_cache(maxsize=None)
def row_batch(n, H, A, modified, adv_scale=1.0):
    """(parameters, observations, batch) of a row: test_gpu_layers.row_inputs (sample 0 all zeros, sample 1 all 255) and
    hashed actions, old log-probs, advantages of both signs and returns; every seventh mask zero.  Shared with
    tests/test_backward_ref_cpu.py"""
    params, obs = row_inputs(n, H, A, modified)
    seed = 9900 + n + H + A
    batch = dict(actions=(hf.hf_u32(seed, n) % np.uint32(A)).astype(np.int64),
                 old_lp=orc.log_softmax(hf.hf_range(seed + 1, (n, A), -0.5, 0.5)),
                 adv=(hf.hf_range(seed + 2, (n,), -1, 1) * np.float32(adv_scale)).astype(np.float32),
                 ret=hf.hf_range(seed + 3, (n,), -1, 1),
                 masks=(np.arange(n) % 7 != 6).astype(np.uint8))
    for a in batch.values():
        a.setflags(write=False)
    return params, obs, batch


def take(batch, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in batch.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(pkg, N, H, A, prec):
    eng = pkg.Engine(N, 1, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
    eng.set_hyper(max_grad_norm=MAX_NORM)
    return eng


def _set_route(pkg, eng, route):
    if route is None:
        return
    for opt, val in zip((pkg.OPT_FUSED_BWD, pkg.OPT_GENERIC_CONV, pkg.OPT_FC_PIPE), route):
        eng.set_option(opt, val)
        assert eng.get_option(opt) == val


def _set_batch(eng, obs, batch):
    eng.set_batch(obs, batch["actions"], batch["old_lp"], batch["adv"], batch["ret"], batch["masks"])


def _update(eng, params, M, tensors=None):
    """train(lr = 0, 1 epoch, M minibatches) -> (export, B, stored, grads): the parameters stay bit-identical and the clip
    factor is exactly 1"""
    m = eng.train(0.0, 1, M)
    assert np.array_equal(_bits(eng.export_params()), _bits(params))
    norm = np.float32(m["grad_norm"][0, M - 1])
    assert np.isfinite(norm) and np.float32(MAX_NORM) / (norm + np.float32(1e-6)) >= 1
    exp, B, stored = eng.export_backward() if tensors is None else eng.export_backward(tensors)
    return exp, B, stored, eng.export_grads()


def _assert_stored_values(pkg, exp, stored, bf16, fused_tail):
    assert bool(stored & pkg.BWD_TENSORS["dconv1"]) == (not fused_tail) and ("dconv1" in exp) == (not fused_tail)
    assert stored | pkg.BWD_TENSORS["dconv1"] == 255
    if bf16:  # bf16 values widened exactly; the activations after the ReLU
        for name in ("conv1", "conv2", "conv3", "dfc", "dconv3", "dconv2", "dconv1"):
            if name in exp:
                assert not (_bits(exp[name]) & 0xFFFF).any(), name
    for name in ("conv1", "conv2", "conv3"):
        if name in exp:
            assert exp[name].min() >= 0, name


def _same_bits(routes, exports, grads, H, A):
    """the equalities of the module docstring"""
    for a, ra in routes:
        for b, rb in routes:
            if ra is None or rb is None or a >= b:
                continue
            if ra[1:] == rb[1:]:  # differ in OPT_FUSED_BWD alone
                for t in ("conv1", "conv2", "conv3", "fc", "dfc", "dconv3", "dconv2") + (("dconv1",) if ra[1] else ()):
                    assert np.array_equal(_bits(exports[a][t]), _bits(exports[b][t])), (a, b, t)
                ga, gb = br.split_grads(grads[a], H, A), br.split_grads(grads[b], H, A)
                for l in ("heads", "fc", "conv3") + (("conv2", "conv1") if ra[1] else ()):
                    for k in (0, 1):
                        assert np.array_equal(_bits(ga[l][k]), _bits(gb[l][k])), (a, b, l, k)
            if ra[:2] == rb[:2]:  # differ in OPT_FC_PIPE alone
                for t in ("conv1", "conv2", "conv3"):
                    assert np.array_equal(_bits(exports[a][t]), _bits(exports[b][t])), (a, b, t)


def _fused_tail_on_the_stored_dz1(title, routes, exports, grads, H, A, obs):
    """The fused tail forms dz1 from the same dz2, a1 and W2d as conv2's dgrad launch (bit-identical inputs: _same_bits), and
    conv_bwd_fused.hpp rounds it at the same point, so its dW1 / db1 must be an fp32 sum over the dz1 that the
    three-launch twin of the route STORED: check (c) with no allowance at all.  This is the exact chain behind the one
    large figure of the fused tail (n = 37: conv1.w of output channel 12 is 46 u Sa from the evaluation on
    bf16(gate W2_b^T dz2)): the twin's stored dz1 element (22, 12, 5, 7) is the other neighbour of an exact value that lies
    on a bf16 rounding boundary (inside its interval (a)), and on the stored dz1 the fused gradient is within 1.2 u Sa."""
    failures = []
    for name, route in routes:
        twin = [m for m, r in routes if route is not None and r == (0,) + route[1:]]
        if route is None or route[0] != 2 or route[1] != 0 or not twin:
            continue
        W, b = br.wgrad("conv1", exports[twin[0]]["dconv1"], obs)
        G = br.split_grads(grads[name], H, A)["conv1"]
        for ref, got, what in ((W, G[0], "conv1.w"), (b, G[1], "conv1.b")):
            c = br.bound_check(ref, got)
            print("%s %s: %s on the dz1 that '%s' stored: max |d| / (u Sa) %.3g against R %.3g, worst |d| / bound %.3g" % (
                title, name, what, twin[0], c["ratio"], c["R"], c["worst"]))
            if len(c["violations"]):
                failures.append("%s %s: %s is outside (c) on the stored dz1 of '%s' at %s" % (
                    title, name, what, twin[0], c["violations"][0].tolist()))
    return failures


def _check(title, params, H, A, bf16, obs, batch, exp, grads, cache, only=None):
    n_mask = int(np.asarray(batch["masks"]).sum())
    bad, report, results = br.check_backward(params, H, A, bf16, obs, batch, HYPER, n_mask, exp, grads, cache, only)
    print(br.summary(title, report))
    return ["%s: %s" % (title, f) for f in bad], results


@pytest.mark.parametrize("row", ROWS, ids=[_id(r) for r in ROWS])
def test_every_backward_layer_on_the_engines_own_stored_tensors(pkg, row):
    n, H, A, prec, modified, routes, only = row
    params, obs, batch = row_batch(n, H, A, modified)
    bf16 = prec == "bf16"
    eng = _engine(pkg, n, H, A, prec)
    eng.load_params(params)
    _set_batch(eng, obs, batch)
    tensors = None if only is None else ("conv3", "fc", "dfc", "dconv3")
    exports, grads, failures, cache, runs = {}, {}, [], {}, []
    for name, route in routes:
        _set_route(pkg, eng, route)
        exp, B, stored, g = _update(eng, params, 1, tensors)
        assert B == n
        if tensors is None:
            if route is None:  # (the default decides by the size; an fp32 context has no fused tail)
                fused = bf16 and not (stored & pkg.BWD_TENSORS["dconv1"])
            else:  # the fused tail is a patch-kernel route
                fused = route[0] == 2 and route[1] == 0
            _assert_stored_values(pkg, exp, stored, bf16, fused)
        exports[name], grads[name] = exp, g
        bad, results = _check("backward %s %s" % (_id(row), name), params, H, A, bf16, obs, batch, exp, g, cache, only)
        failures += bad
        runs.append(results)
    eng.close()
    print(br.row_summary("row %s" % _id(row), runs))
    assert not failures, failures
    _same_bits(routes, exports, grads, H, A)
    if bf16 and only is None:
        bad = _fused_tail_on_the_stored_dz1("row %s" % _id(row), routes, exports, grads, H, A, obs)
        assert not bad, bad


# ------------------------------------------------------------------ stale rows, the sample-map offset, the shuffle
STALE = (74, 96, 6, 520)  # N, H, A, and the size of the update that runs first


@pytest.mark.parametrize("shuffle", [0, 1], ids=["contiguous", "shuffled"])
def test_second_minibatch_after_a_larger_update_with_large_gradients(pkg, shuffle):
    """N = 74, M = 2 on a context that first ran an update on 520 samples with advantages 100 times larger: rows >= 37 of
    every buffer hold stale, large values, and the export is of minibatch 1 - samples [37, 74), or the second half of
    aleppo_read_sample_order's order (the IDX instantiations of the fused tail and of conv1's wgrad)"""
    N, H, A, big = STALE
    params, obs, batch = row_batch(N, H, A, False)
    _, obs_big, batch_big = row_batch(big, H, A, False, 100.0)
    failures, exports, grads, cache, runs = [], {}, {}, {}, []
    orders = []
    for name, route in PAIR:
        eng = _engine(pkg, big, H, A, "bf16")
        _set_route(pkg, eng, route)
        eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, shuffle)
        eng.load_params(params)
        _set_batch(eng, obs_big, batch_big)
        eng.train(0.0, 1, 1)
        _set_batch(eng, obs, batch)
        exp, B, stored, g = _update(eng, params, 2)
        order = eng.sample_order(1)[0]
        eng.close()
        assert B == N // 2 and np.array_equal(np.sort(order), np.arange(N))
        if not shuffle:
            assert np.array_equal(order, np.arange(N))
        else:
            assert not np.array_equal(order, np.arange(N))
        orders.append(order)
        idx = order[B:]
        _assert_stored_values(pkg, exp, stored, True, route[0] == 2)
        exports[name], grads[name] = exp, g
        bad, results = _check("backward stale N%d %s %s" % (N, "shuffled" if shuffle else "contiguous", name), params, H, A,
                              True, obs[idx], take(batch, idx), exp, g, cache)
        failures += bad
        runs.append(results)
    print(br.row_summary("row N%d M2 %s" % (N, "shuffled" if shuffle else "contiguous"), runs))
    assert not failures, failures
    assert np.array_equal(orders[0], orders[1])
    _same_bits(PAIR, exports, grads, H, A)
    bad = _fused_tail_on_the_stored_dz1("row N%d M2" % N, PAIR, exports, grads, H, A, obs[orders[0][N // 2:]])
    assert not bad, bad


def test_captured_update_exports_the_eager_updates_bits(pkg):
    """ALEPPO_OPT_UPDATE_GRAPH = 1: the first update of a shape runs eagerly, the second is captured, the third replays;
    after each the export and the gradient have the bits of an eager context's"""
    n, H, A = 37, 96, 6
    params, obs, batch = row_batch(n, H, A, False)
    out = {}
    for graph in (0, 1):
        eng = _engine(pkg, n, H, A, "bf16")
        eng.set_option(pkg.OPT_UPDATE_GRAPH, graph)
        eng.load_params(params)
        _set_batch(eng, obs, batch)
        out[graph] = [_update(eng, params, 1) for _ in range(3)]
        if graph:
            assert eng.get_option(pkg.OPT_UPDATE_GRAPH) >= 2  # graph launches
        eng.close()
    exp0, B0, stored0, g0 = out[0][0]
    bad, _ = _check("backward n37 captured (third call)", params, H, A, True, obs, batch, out[1][2][0], out[1][2][3], {})
    assert not bad, bad
    for graph in (0, 1):
        for exp, B, stored, g in out[graph]:
            assert (B, stored) == (B0, stored0) and set(exp) == set(exp0)
            assert np.array_equal(_bits(g), _bits(g0))
            for t in exp:
                assert np.array_equal(_bits(exp[t]), _bits(exp0[t])), (graph, t)


# ------------------------------------------------------------------ the entry point itself
def test_export_errors(pkg):
    import ctypes as C
    n, H, A = 37, 96, 6
    params, obs, batch = row_batch(n, H, A, False)
    eng = _engine(pkg, n, H, A, "bf16")
    eng.load_params(params)
    lib = pkg.lib()
    buf = np.zeros((n, H), np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def call(cap, fc):
        return lib.aleppo_export_backward(eng._ctx, C.c_int64(cap), None, None, None, fc, None, None, None, None, None, None)
    assert call(n, ptr) == pkg.ERR_RUNTIME  # before any update
    _set_batch(eng, obs, batch)
    eng.train(0.0, 1, 1)
    assert call(n, None) == pkg.ERR_INVALID_ARGUMENT  # no output
    assert call(n - 1, ptr) == pkg.ERR_INVALID_ARGUMENT  # capacity < B
    assert call(n, ptr) == pkg.OK and buf.any()
    again = buf.copy()
    assert call(n, ptr) == pkg.OK and np.array_equal(again, buf)  # reading changes nothing
    eng.forward(obs[:3])
    assert call(n, ptr) == pkg.ERR_RUNTIME  # something else has run the network
    with pytest.raises(pkg.AleppoError):
        eng.export_backward()
    eng.train(0.0, 1, 1)
    assert call(n, ptr) == pkg.OK
    eng.forward_activations(obs[:3])
    assert call(n, ptr) == pkg.ERR_RUNTIME
    eng.close()


def test_the_export_only_reads(pkg):
    """two contexts run the same two updates with a real learning rate, one calls the export between them (and after):
    state digests and exported gradients are equal bit for bit"""
    n, H, A = 74, 96, 6
    params, obs, batch = row_batch(n, H, A, False)
    out = []
    for export in (False, True):
        eng = pkg.Engine(n, 1, A, H, precision=pkg.BF16)
        eng.load_params(params)
        _set_batch(eng, obs, batch)
        eng.train(2.5e-4, 1, 2)
        if export:
            exp, B, stored = eng.export_backward()
            assert B == n // 2 and exp["dfc"].any()
        eng.train(2.5e-4, 1, 2)
        if export:
            eng.export_backward()
        out.append((eng.state_digest(), eng.export_grads(), eng.export_params()))
        eng.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and np.array_equal(_bits(out[0][2]), _bits(out[1][2]))
