"""The regularised optimizer step (ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF, reg_step_kernel), the anchor and
aleppo_shrink_perturb on the GPU.

Shapes: N = 64 samples (E = 8, T = 8).  fp32 (H, A) = (32, 4); bf16 (96, 6), whose last fc tile has 32 of 64 rows; bf16
(128, 18).  The element-by-element check needs the state around ONE optimizer step, so it runs one minibatch of 64 per
call; everything that compares whole calls runs two minibatches of 32 (a call's second step reads its own schedule slot).
Coefficients: the regime where the terms dominate, f_wd = 1e-2 and f_an = 2e-2 at lr = 1e-3, and one realistic row,
lr = 2.5e-4 with wd = 1e-2.  The bound is tests/reg_ref.py's; everything else is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_ref as ar
import hashfill as hf
import reg_ref as rg
import update_harness as uh

pytestmark = pytest.mark.gpu

E, T, N, M = 8, 8, 64, 2
SHAPES = [("fp32", 32, 4), ("bf16", 96, 6), ("bf16", 128, 18)]
LR, WD, LA = 1e-3, 10.0, 20.0
# (name, lr, wd, la, anchor: None, "hashed" or "live")
COMBOS = [("decay", LR, WD, 0.0, None), ("anchor", LR, 0.0, LA, "hashed"), ("both", LR, WD, LA, "hashed"),
          ("both, anchor = a take of the live set", LR, WD, LA, "live"), ("realistic", 2.5e-4, 1e-2, 0.0, None)]


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    p = load_package()
    p.lib()
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


@functools.lru_cache(maxsize=None)
def _batch(seed, A):
    b = uh.hashed_batch(seed, N, A, mask_p=0.1)
    for a in b:
        a.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _params(seed, H, A):
    p = hf.fill_params(seed, H, A)
    p.setflags(write=False)
    return p


def _state(eng):
    sd = eng.state_dict()
    return (sd["params"], sd["exp_avg"], sd["exp_avg_sq"]), int(sd["step"])


def _regularise(eng, wd, la, anchor, H, A):
    """the coefficients and the anchor of one COMBOS row; the anchor as the reference reads it (None: none)"""
    want = None
    if anchor == "hashed":
        eng.load_anchor(_params(7105, H, A))
        want = eng.anchor_params()
        assert _same(want, _params(7105, H, A))  # an import followed by an export returns the imported bits
    elif anchor == "live":
        eng.anchor_take("live")
        want = eng.anchor_params()
        assert _same(want, eng.export_params())
    eng.set_regularization(weight_decay=wd, anchor_coef=la)
    got = eng.regularization()
    assert got == dict(weight_decay=float(np.float32(wd)), anchor_coef=float(np.float32(la)))
    return want


# ------------------------------------------------------------------ 1: every element, at the bound
@pytest.mark.parametrize("combo", COMBOS, ids=[c[0] for c in COMBOS])
@pytest.mark.parametrize("prec,H,A", SHAPES)
def test_every_element_of_a_regularised_step(pkg, prec, H, A, combo):
    """steps t = 1, 2, 3 from load_params, each on another batch, then one step at t = 10^6 from imported hashed moments:
    around every step the engine's own exports - parameters, both moments, the scaled gradient, the anchor - go to reg_ref,
    and every element of all 12 tensors and both moments must be within its bound"""
    _, lr, wd, la, anchor = combo
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
    offs = ar.param_offsets(H, A)
    eng.load_params(_params(7100, H, A))
    a = _regularise(eng, wd, la, anchor, H, A)
    total = ar.StepCheck()
    before, step = _state(eng)
    assert step == 0
    moved = []

    def take(t, seed):
        nonlocal before
        eng.set_batch(*_batch(seed, A))
        m = eng.train(lr, 1, 1)
        assert np.isfinite(m["loss"]).all() and np.isfinite(m["grad_norm"]).all()
        after, step = _state(eng)
        assert step == t
        g = eng.export_grads()
        assert np.abs(g).max() > 0
        if a is not None:
            assert _same(eng.anchor_params(), a)  # (the update only reads the anchor)
        total.merge(rg.check_step(before, after, g, t, lr, offs, wd, la, a))
        # the terms are there: against the plain step of adam_ref the same result is far outside the bound
        moved.append(float(np.mean(ar.ratios(before, after, g, t, lr)["p"] > 1.0)))
        before = after

    for t in (1, 2, 3):
        take(t, 7100 + 10 * t)
    m0, v0 = ar.hashed_moments(7200, before[0].size)
    eng.load_state_dict(dict(params=before[0], exp_avg=m0, exp_avg_sq=v0, step=10 ** 6 - 1))
    before, step = _state(eng)
    assert step == 10 ** 6 - 1
    take(10 ** 6, 7150)
    eng.close()
    print(total.summary(f"regularised step {prec} H={H} A={A} {combo[0]}: worst ratio to bound"),
          "share outside the plain step's bound per step:", ["%.3g" % x for x in moved])
    assert not total.failures, total.failures[:8]
    first = 1 if (anchor == "live" and wd == 0.0) else 0
    assert all(x > 0.5 for x in moved[first:]), moved


# ------------------------------------------------------------------ 2, 3, 4: where nothing may change
def _run(pkg, prec, H, A, configure=None, epochs=2, lr=LR, **kw):
    """one context (update_harness.make_engine(**kw)): configure(eng) after load_params, the batch, one call of `epochs`
    epochs x two minibatches; its read_update with the state"""
    eng = uh.make_engine(pkg, E, T, A, H, prec=_prec(pkg, prec), **kw)
    eng.load_params(_params(7300, H, A))
    if configure:
        configure(eng)
    eng.set_batch(*_batch(7310, A))
    m = eng.train(lr, epochs, M)
    out = uh.read_update(eng, m, epochs, M, state=True)
    eng.close()
    return out


@pytest.mark.parametrize("prec,H,A", SHAPES)
def test_zero_coefficients_are_the_plain_update_bit_for_bit(pkg, prec, H, A):
    """both coefficients zero - never set, set to zero, or set to zero after an update ran with them - give the bits of a
    context that never touched the options: parameters, moments, metrics, per-sample planes, gradients"""
    plain = _run(pkg, prec, H, A)

    def zeros(eng):
        eng.set_regularization(weight_decay=0.0, anchor_coef=0.0)

    def after_use(eng):
        _regularise(eng, WD, LA, "hashed", H, A)
        eng.set_batch(*_batch(7320, A))
        eng.train(LR, 1, M)
        assert not _same(eng.export_params(), _params(7300, H, A))
        eng.set_regularization(weight_decay=0.0, anchor_coef=0.0)
        eng.load_params(_params(7300, H, A))  # (resets Adam; the anchor stays, unread)

    uh.assert_identical(plain, _run(pkg, prec, H, A, zeros))
    uh.assert_identical(plain, _run(pkg, prec, H, A, after_use))
    # (and the options do something: one of them set, the parameters differ while the gradient of step 1 does not)
    decayed = _run(pkg, prec, H, A, lambda eng: eng.set_regularization(weight_decay=WD), epochs=1)
    one = _run(pkg, prec, H, A, epochs=1)
    assert not _same(decayed["params"], one["params"])
    assert _same(decayed["m"]["grad_norm"][0, 0], one["m"]["grad_norm"][0, 0])


@pytest.mark.parametrize("prec,H,A", SHAPES)
def test_anchor_at_the_live_parameters_and_a_zero_rate_change_nothing(pkg, prec, H, A):
    """la > 0, wd = 0 and the anchor taken at the step: r = f_an (p0 - p0) is exactly zero, and one step is the plain step
    bit for bit.  lr = 0 with both coefficients changes no parameter bit."""
    res = {}
    for name in ("plain", "anchored"):
        eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
        eng.load_params(_params(7400, H, A))
        if name == "anchored":
            eng.anchor_take("live")
            eng.set_regularization(anchor_coef=LA)
        eng.set_batch(*_batch(7410, A))
        m = eng.train(LR, 1, 1)
        res[name] = uh.read_update(eng, m, 1, 1, state=True)
        if name == "anchored":  # the second step is pulled back: the anchor is where step 1 started
            m = eng.train(LR, 1, 1)
            second = uh.read_update(eng, m, 1, 1, state=True)
        eng.close()
    uh.assert_identical(res["plain"], res["anchored"])
    assert not _same(second["params"], res["anchored"]["params"])
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
    eng.load_params(_params(7400, H, A))
    _regularise(eng, WD, LA, "hashed", H, A)
    eng.set_batch(*_batch(7410, A))
    eng.train(0.0, 1, M)
    (p, m1, m2), step = _state(eng)
    eng.close()
    assert step == M and _same(p, _params(7400, H, A)) and np.abs(m1).max() > 0


# ------------------------------------------------------------------ 5: what the kernel writes besides P
@pytest.mark.parametrize("prec,H,A", SHAPES)
def test_copies_the_regularised_step_writes_match_load_time_copies(pkg, prec, H, A):
    """engine X takes two regularised steps, so its bf16 compute copy and its transposed data-gradient layouts are the ones
    reg_step_kernel wrote; engine Y is fresh and loads X's state, so its copies come from the load-time kernels.  A forward
    on 37 observations and one more regularised step must agree bit for bit in everything.  As in test_optimizer_step.py
    the steps run at lr = 1e-2 from an imported optimizer state in which every entry is moving."""
    lr = 1e-2
    params = _params(7500, H, A)
    x, y = (pkg.Engine(E, T, A, H, precision=_prec(pkg, prec)) for _ in range(2))
    sign = np.where(hf.hf_u32(7501, params.size) & np.uint32(1), -1.0, 1.0)
    x.load_state_dict(dict(params=params, exp_avg=(1e-4 * sign).astype(np.float32),
                           exp_avg_sq=np.full(params.size, 1e-8, np.float32), step=10))
    for eng in (x, y):
        eng.load_anchor(_params(7105, H, A))
        eng.set_regularization(weight_decay=1.0, anchor_coef=2.0)  # f_wd = 1e-2, f_an = 2e-2 at this rate
    for seed in (7510, 7520):
        x.set_batch(*_batch(seed, A))
        x.train(lr, 1, 1)
    sd = x.state_dict()
    assert int(sd["step"]) == 12
    y.load_state_dict(sd)
    out = []
    for eng in (x, y):
        logits, values = eng.forward(hf.hf_bytes(7531, (37, 4, 84, 84)))
        eng.set_batch(*_batch(7540, A))
        m = eng.train(lr, 1, 1)
        (p, m1, m2), step = _state(eng)
        assert step == 13
        out.append(dict(logits=logits, values=values, loss=m["loss"], norm=m["grad_norm"], grads=eng.export_grads(),
                        params=p, exp_avg=m1, exp_avg_sq=m2))
        eng.close()
    diff = {k: int(np.sum(_bits(out[0][k]) != _bits(out[1][k]))) for k in out[0]}
    print(f"copies written by the regularised step vs load-time copies {prec} H={H}: differing elements {diff}")
    assert not any(diff.values()), diff
    assert not _same(out[0]["params"], sd["params"])


# ------------------------------------------------------------------ 6, 7, 8: schedules
SEQUENCE = [(WD, LA), (WD, LA), (WD, LA), (3.0, 0.5), (0.0, 0.0), (0.0, 0.0), (WD, 0.0), (WD, 0.0)]


@pytest.mark.parametrize("prec,H,A", SHAPES[:2])
def test_captured_update_equals_eager_and_follows_the_coefficients(pkg, prec, H, A):
    """the same eight calls on an eager and on a capturing context (ALEPPO_OPT_UPDATE_GRAPH), the coefficients changed
    between them: bit-identical after every call.  Launch counts: the first call of a kernel choice runs eagerly, the second
    captures, later ones replay; a change of the VALUES between two replays is followed without a capture, a change of the
    choice (to zero and back) re-arms."""
    engines = []
    for graph in (0, 1):
        eng = uh.make_engine(pkg, E, T, A, H, prec=_prec(pkg, prec), options=[(pkg.OPT_UPDATE_GRAPH, graph)])
        eng.load_params(_params(7600, H, A))
        eng.load_anchor(_params(7105, H, A))
        eng.set_batch(*_batch(7610, A))
        engines.append(eng)
    launches, states = [], []
    for wd, la in SEQUENCE:
        outs = []
        for eng in engines:
            eng.set_regularization(weight_decay=wd, anchor_coef=la)
            m = eng.train(LR, 1, M)
            outs.append(uh.read_update(eng, m, 1, M, state=True))
        uh.assert_identical(outs[0], outs[1])
        states.append(outs[1]["params"])
        launches.append((engines[0].get_option(pkg.OPT_UPDATE_GRAPH), engines[1].get_option(pkg.OPT_UPDATE_GRAPH)))
    for eng in engines:
        eng.close()
    print("graph launches (eager, capturing) after each call:", launches)
    assert [l[0] for l in launches] == [0] * len(SEQUENCE)
    #        eager, capture, replay, replay with new values, eager (zero: adam_kernel), capture, eager (non-zero), capture
    assert [l[1] for l in launches] == [0, 1, 2, 3, 3, 4, 4, 5]
    assert not _same(states[2], states[3])


@pytest.mark.parametrize("prec,H,A", SHAPES[:2])
def test_one_rank_communicator_gives_the_single_gpu_bits(pkg, prec, H, A):
    conf = lambda eng: _regularise(eng, WD, LA, "hashed", H, A)
    single = _run(pkg, prec, H, A, conf)
    comm = _run(pkg, prec, H, A, conf, comm=True, options=[(pkg.OPT_FORCE_COMM, 1)])
    uh.assert_identical(single, comm)


@pytest.mark.parametrize("prec,H,A", SHAPES[:2])
@pytest.mark.parametrize("features", [False, True], ids=["plain", "shuffle + value clip + advantage norm + KL penalty"])
def test_one_call_of_three_epochs_equals_three_calls(pkg, prec, H, A, features):
    res = []
    for calls in ((3,), (1, 1, 1)):
        eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
        if features:
            for opt in (pkg.OPT_MINIBATCH_SHUFFLE, pkg.OPT_VALUE_CLIP, pkg.OPT_ADV_NORM_MINIBATCH, pkg.OPT_KL_PENALTY):
                eng.set_option(opt, 1)
            eng.set_kl_coef(0.5)
        eng.load_params(_params(7700, H, A))
        _regularise(eng, WD, LA, "hashed", H, A)
        eng.set_batch(*_batch(7710, A), values=hf.hf_range(7711, (N,), -1, 1) if features else None)
        ms = [eng.train(LR, epochs, M) for epochs in calls]
        state, step = _state(eng)
        res.append((state, step, np.concatenate([m["loss"] for m in ms]), np.concatenate([m["grad_norm"] for m in ms])))
        eng.close()
    (s1, t1, l1, n1), (s3, t3, l3, n3) = res
    assert t1 == t3 == 3 * M and l1.shape == l3.shape == (3, M)
    diff = {name: int(np.sum(_bits(a) != _bits(b)))
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "loss", "norm"), s1 + (l1, n1), s3 + (l3, n3))}
    assert not any(diff.values()), diff


# ------------------------------------------------------------------ 9: errors
def test_failed_calls_change_nothing(pkg):
    prec, H, A = SHAPES[0]
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
    lib, ctx = pkg.lib(), eng._ctx
    INV, RUN = pkg.ERR_INVALID_ARGUMENT, pkg.ERR_RUNTIME
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    n = eng.param_count
    eng.load_params(_params(7800, H, A))
    eng.set_batch(*_batch(7810, A))
    eng.train(LR, 1, M)
    held, step = _state(eng)
    grads = eng.export_grads()

    def unchanged(anchor=None, reg=None):
        now, t = _state(eng)
        ok = t == step and all(_same(a, b) for a, b in zip(now, held)) and _same(eng.export_grads(), grads)
        if anchor is not None:
            ok = ok and _same(eng.anchor_params(), anchor)
        return ok and (reg is None or eng.regularization() == reg)

    # before any anchor: the export is refused; la > 0 makes aleppo_train refuse, and nothing moves
    with pytest.raises(pkg.AleppoError):
        eng.anchor_params()
    eng.set_regularization(anchor_coef=LA)
    with pytest.raises(pkg.AleppoError, match="anchor"):
        eng.train(LR, 1, M)
    assert unchanged(reg=dict(weight_decay=0.0, anchor_coef=float(np.float32(LA))))
    eng.set_regularization(weight_decay=WD, anchor_coef=0.0)  # weight decay alone needs no anchor
    eng.train(LR, 1, M)
    with pytest.raises(pkg.AleppoError):
        eng.anchor_params()
    held, step = _state(eng)
    grads = eng.export_grads()
    # invalid bit patterns leave the old value in place
    reg = eng.regularization()
    for opt in (pkg.OPT_WEIGHT_DECAY, pkg.OPT_ANCHOR_COEF):
        for x in (-0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert lib.aleppo_set_option(ctx, C.c_int(opt), C.c_int(pkg.float_bits(x))) == INV, (opt, x)
        assert lib.aleppo_set_option(ctx, C.c_int(opt), C.c_int(-1)) == INV
    assert lib.aleppo_set_option(ctx, C.c_int(22), C.c_int(0)) == INV  # (22 stays unassigned)
    assert unchanged(reg=reg)
    # wrong counts, null pointers, unknown sets
    eng.load_anchor(_params(7105, H, A))
    anchor = eng.anchor_params()
    flat = np.full(n + 1, -7, np.float32)
    for count in (n - 1, n + 1, 0):
        assert lib.aleppo_anchor_import(ctx, ptr(flat), C.c_size_t(count)) == INV
        assert lib.aleppo_anchor_export(ctx, ptr(flat), C.c_size_t(count)) == INV
    assert lib.aleppo_anchor_import(ctx, None, C.c_size_t(n)) == INV
    assert lib.aleppo_anchor_export(ctx, None, C.c_size_t(n)) == INV
    assert (flat == -7).all()
    assert lib.aleppo_anchor_take(ctx, C.c_int(3)) == INV and lib.aleppo_anchor_take(ctx, C.c_int(-1)) == INV
    assert lib.aleppo_anchor_take(ctx, C.c_int(pkg.SET_AVERAGED)) == RUN  # (a set that does not exist yet)
    assert lib.aleppo_anchor_take(ctx, C.c_int(pkg.SET_SNAPSHOT)) == RUN
    # the anchor is not a set the policy comparison or the snapshot accept: their checks are what they were
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.snapshot_take(3)
    for shrink, sigma, flags in ((1.5, 0.0, 0), (-0.1, 0.0, 0), (float("nan"), 0.0, 0), (0.5, -1.0, 0),
                                 (0.5, float("inf"), 0), (0.5, float("nan"), 0), (0.5, 1e39, 0), (0.5, 0.1, 2)):
        assert lib.aleppo_shrink_perturb(ctx, C.c_double(shrink), C.c_double(sigma), C.c_uint64(1), C.c_int(flags)) == INV
    assert unchanged(anchor, reg)
    # while a step is armed every call is refused
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(7880, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    assert lib.aleppo_anchor_take(ctx, C.c_int(pkg.SET_LIVE)) == RUN
    assert lib.aleppo_anchor_import(ctx, ptr(flat), C.c_size_t(n)) == RUN
    assert lib.aleppo_anchor_export(ctx, ptr(flat), C.c_size_t(n)) == RUN
    assert lib.aleppo_shrink_perturb(ctx, C.c_double(0.5), C.c_double(0.1), C.c_uint64(1), C.c_int(0)) == RUN
    assert lib.aleppo_set_option(ctx, C.c_int(pkg.OPT_WEIGHT_DECAY), C.c_int(0)) == RUN
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    eng.synchronize()
    assert (flat == -7).all() and unchanged(anchor, reg)
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()


def test_what_never_touches_the_anchor(pkg):
    """load_params, a recycle, shrink and perturb, the averaged set and the snapshot leave the anchor alone; a take copies
    the averaged set and the snapshot as they stand"""
    prec, H, A = SHAPES[1]
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec))
    eng.load_params(_params(7900, H, A))
    eng.load_anchor(_params(7105, H, A))
    anchor = eng.anchor_params()
    digest = eng.state_digest()
    eng.load_anchor(_params(7106, H, A))
    assert eng.state_digest() == digest  # the digest does not cover the anchor
    eng.load_anchor(anchor)
    eng.load_params(_params(7901, H, A))
    eng.recycle_units(np.ones(160 + H, np.uint8), key=3)
    eng.shrink_perturb(0.5, 0.5, key=4)
    eng.ema_open()
    eng.ema_update(0.5)
    eng.snapshot_take("live")
    eng.load_snapshot(_params(7902, H, A))
    assert _same(eng.anchor_params(), anchor)
    eng.anchor_take("snapshot")
    assert _same(eng.anchor_params(), _params(7902, H, A))
    eng.anchor_take("averaged")
    assert _same(eng.anchor_params(), eng.ema_params()[0])
    eng.close()


# ------------------------------------------------------------------ 10: shrink and perturb
@pytest.mark.parametrize("prec,H,A", SHAPES)
def test_shrink_perturb(pkg, prec, H, A):
    key, shrink, sigma = 0xC0FFEE123456789, 0.8, 0.1
    params = _params(8000, H, A)
    m0, v0 = ar.hashed_moments(8001, params.size)
    sd0 = dict(params=params, exp_avg=m0, exp_avg_sq=v0, step=17)
    want = rg.shrink_perturb(params, shrink, sigma, key, H, A)
    assert np.mean(_bits(want) != _bits(params)) > 0.99
    engines = [pkg.Engine(E, T, A, H, precision=_prec(pkg, prec)) for _ in range(3)]
    x, y, z = engines
    for eng in (x, y):
        eng.load_state_dict(sd0)
    # shrink = 1, sigma = 0 runs the pass and changes no bit
    x.shrink_perturb(1.0, 0.0, key=key)
    (p, m1, m2), step = _state(x)
    assert _same(p, params) and _same(m1, m0) and _same(m2, v0) and step == 17
    # the restatement, bit for bit on every element; the moments kept, or zeroed with the flag; the step count stays
    x.shrink_perturb(shrink, sigma, key=key)
    y.shrink_perturb(shrink, sigma, key=key, reset_moments=True)
    (px, m1x, m2x), sx = _state(x)
    (py, m1y, m2y), sy = _state(y)
    bad = np.flatnonzero(_bits(px) != _bits(want))
    assert bad.size == 0, (bad.size, bad[:8], int(np.searchsorted(ar.param_offsets(H, A), bad[0], side="right")) - 1)
    assert _same(py, want)  # two contexts given the same key agree
    assert _same(m1x, m0) and _same(m2x, v0) and sx == 17
    assert not _bits(m1y).any() and not _bits(m2y).any() and sy == 17
    # the pads are still zero: the averaged set's statistics add P^2 over the PADDED vector in double
    x.ema_open()
    norm = x.ema_stats()["param_norm"]
    assert abs(norm ** 2 / float(np.sum(want.astype(np.float64) ** 2)) - 1) < 1e-10
    # the derived copies: a fresh engine that loads the state answers and steps identically
    z.load_state_dict(x.state_dict())
    out = []
    for eng in (x, z):
        logits, values = eng.forward(hf.hf_bytes(8031, (37, 4, 84, 84)))
        eng.set_batch(*_batch(8040, A))
        m = eng.train(LR, 1, M)
        (p, m1, m2), step = _state(eng)
        out.append(dict(logits=logits, values=values, loss=m["loss"], norm=m["grad_norm"], grads=eng.export_grads(),
                        params=p, exp_avg=m1, exp_avg_sq=m2))
    diff = {k: int(np.sum(_bits(out[0][k]) != _bits(out[1][k]))) for k in out[0]}
    assert not any(diff.values()), diff
    # another key draws another perturbation; sigma = 0 only shrinks
    y.load_state_dict(sd0)
    y.shrink_perturb(shrink, sigma, key=key + 1)
    assert not _same(y.export_params(), want)
    y.load_state_dict(sd0)
    y.shrink_perturb(0.5, 0.0, key=key)
    assert _same(y.export_params(), np.float32(0.5) * params)
    for eng in engines:
        eng.close()
