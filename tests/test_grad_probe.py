"""Gradient probes on the GPU (-m gpu, everything through the C ABI).

The Gram kernel alone, on hashed vectors put into the slots with load_grad: every entry within the derived bound of
grad_probe_ref.gram ((n_r - 1) * 2^-53 * sum |x_i x_j|), exact symmetry, a repeated slot, two calls, planted NaN / Inf,
zeros, pads - at (H, A) = (32, 1), (32, 5) (the head split inside a 16-byte group), (96, 18) (the H % 64 == 32 pads) and
(512, 18) (fc.w has more chunks than one reduce tile).

The probe, on caller batches from update_harness.hashed_batch with a share of the samples masked: bit for bit
aleppo_train's gradient; it changes nothing, eager and under a captured update; the loss terms separate exactly; the
composed reference (update_ref.composed_train) at fp32 atol 1e-4 and bf16 1e-5 + 2e-3 max|g|; grad_take; the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import grad_probe_ref as gp
import hashfill as hf
import update_harness as uh
import update_ref as ur
from shared_fixtures import pkg  # noqa: F401

_hashed = functools.partial(uh.hashed_batch, mask_p=0.15)
LISTS = ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3], [1, 1], [2, 0], [3, 0, 3])


def _prec(pkg, prec):
    return pkg.BF16 if prec == "bf16" else pkg.FP32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def _case(H, A):
    """four hashed vectors of different scales and their reference Gram and bound, computed once per (H, A)"""
    n = sum(gp.sizes(H, A))
    x = [hf.hf_range(8100 + 7 * H + A + i, (n,), -1.0 - i, 0.5 + 0.25 * i) for i in range(4)]
    return x, gp.gram(x, H, A)[0], gp.bound(x, H, A)


# ------------------------------------------------------------------ the Gram kernel alone
@pytest.mark.gpu
@pytest.mark.parametrize("H,A", [(32, 1), (32, 5), (96, 18), (512, 18)])
def test_gram_against_the_reference(pkg, H, A):
    x, want, lim = _case(H, A)
    eng = pkg.Engine(8, 8, A, H, precision=pkg.FP32)
    for s in range(4):
        eng.load_grad(s, x[s])
        np.testing.assert_array_equal(eng.grad_vector(s), x[s])
    full = None
    for slots in LISTS:
        g, nf = eng.grad_gram(slots, raw=True)
        ix = np.ix_(range(13), slots, slots)
        err = np.abs(g - want[ix])
        worst = float(np.max(np.where(lim[ix] > 0, err / np.where(lim[ix] > 0, lim[ix], 1.0), 0.0)))
        print(f"H={H} A={A} slots={slots}: largest |error| / bound = {worst:.3g}")
        assert (err <= lim[ix]).all(), (slots, np.argwhere(err > lim[ix])[:5])
        assert not nf.any()
        np.testing.assert_array_equal(_bits(g), _bits(g.transpose(0, 2, 1)))  # [i][j] and [j][i]: the same bits
        g2, nf2 = eng.grad_gram(slots, raw=True)
        np.testing.assert_array_equal(_bits(g), _bits(g2))  # two calls
        if slots == [0, 1, 2, 3]:
            full = g
        for i, a in enumerate(slots):  # a repeated slot's entries are the diagonal's bits
            for j, b in enumerate(slots):
                if a == b:
                    assert _bits(g[:, i, j]).tolist() == _bits(g[:, i, i]).tolist()
                if full is not None:
                    assert _bits(g[:, i, j]).tolist() == _bits(full[:, a, b]).tolist(), (slots, i, j)
    named = eng.grad_gram([2, 0])
    assert set(named) == set(pkg.GRAM_NAMES) | {"nonfinite"} and named["all"].shape == (2, 2)
    np.testing.assert_array_equal(named["fc.w"], full[6][np.ix_([2, 0], [2, 0])])
    # zeros: an all-zero slot gives exact zeros, and a vector that was there before does not leak through the pads
    eng.load_grad(3, np.zeros_like(x[3]))
    g, nf = eng.grad_gram([0, 3], raw=True)
    assert (g[:, 1, :] == 0).all() and (g[:, :, 1] == 0).all() and not nf.any()
    np.testing.assert_array_equal(_bits(g[:, 0, 0]), _bits(full[:, 0, 0]))
    g, _ = eng.grad_gram([3], raw=True)
    assert (g == 0).all()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,A", [(32, 1), (32, 5), (96, 18), (512, 18)])
def test_gram_leaves_out_nonfinite_indices(pkg, H, A):
    x = [v.copy() for v in _case(H, A)[0][:3]]
    spans = gp.bounds(H, A)
    x[0][spans[2][0] + 4097] = np.nan   # conv2.w of one slot
    x[1][spans[11][0]] = np.inf         # value.b of another
    x[1][spans[9][1] - 1] = -np.inf     # and the last action bias: the group the head split runs through
    fc = 0
    if H == 512:  # fc.w is 392 chunks of 4096, the reduce adds them in tiles of 128: counts in the first, third and last tile
        for chunk, who in ((5, 2), (300, 0), (300, 1), (391, 2)):
            x[who][spans[6][0] + chunk * 4096 + 37 * chunk % 4096] = np.nan  # (chunk 300: the same index in two slots counts once)
        fc = 3
    eng = pkg.Engine(8, 8, A, H, precision=pkg.FP32)
    for s in range(3):
        eng.load_grad(s, x[s])
    g, nf = eng.grad_gram([0, 1, 2], raw=True)
    worst = gp.check(g, nf, x, H, A)
    print(f"H={H} A={A} with NaN / Inf planted: largest |error| / bound = {worst:.3g}")
    assert nf[2] == 1 and nf[11] == 1 and nf[9] == 1 and nf[6] == fc and nf[12] == 3 + fc and nf.sum() == 6 + 2 * fc
    assert np.isfinite(g).all() and (g[11] == 0).all()  # value.b's only element is left out of every entry
    # a list without the first two slots counts only the third's own and is that vector's Gram
    g2, nf2 = eng.grad_gram([2], raw=True)
    assert nf2[6] == (2 if fc else 0) and nf2.sum() == 2 * nf2[6]
    gp.check(g2, nf2, x[2:], H, A)
    eng.close()


# ------------------------------------------------------------------ the probe
def _engine(pkg, N, A, H, prec, M=1, options=(), T=1, **kw):
    eng = uh.make_engine(pkg, N // T, T, A, H, _prec(pkg, prec), options, max_minibatch=N // M, **kw)
    return eng


def _probe_vs_train(pkg, prec, N, M, A, H, options=(), configure=None, vold=None, T=1, seed=8200):
    eng = _engine(pkg, N, A, H, prec, M, options, T)
    eng.set_hyper(max_grad_norm=1e30)  # (aleppo_export_grads applies the clip factor: 1 under this limit)
    if configure:
        configure(eng)
    eng.load_params(hf.fill_params(seed, H, A))
    batch = _hashed(seed + 20, N, A)
    eng.set_batch(*batch, values=vold)
    B = N // M
    count = eng.grad_probe(0, first=(M - 1) * B, n=B)
    m = eng.train(0.0, 1, M)
    got, want = eng.grad_vector(0), eng.export_grads()
    eng.close()
    assert count == int(m["mask_count"][0, M - 1]) == int(batch[5][(M - 1) * B:].sum())
    assert np.abs(want).max() > 0
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("N,M", [(37, 1), (74, 2), (520, 1)])
def test_probe_is_the_gradient_of_train(pkg, prec, N, M):
    """(520, 1): the two-slice fc weight gradient"""
    _probe_vs_train(pkg, prec, N, M, 4, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("fused_bwd", [0, 2])
@pytest.mark.parametrize("fc_pipe", [0, 1])
def test_probe_takes_the_routes_of_train(pkg, fused_bwd, fc_pipe):
    _probe_vs_train(pkg, "bf16", 260, 1, 4, 128, T=4,
                    options=[(pkg.OPT_FUSED_BWD, fused_bwd), (pkg.OPT_FC_PIPE, fc_pipe)])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["value_clip", "adv_norm", "kl_penalty"])
def test_probe_follows_the_update_options(pkg, which):
    N, A = 74, 4
    vold = hf.hf_range(8290, (N,), -1, 1) if which == "value_clip" else None
    opt = dict(value_clip=pkg.OPT_VALUE_CLIP, adv_norm=pkg.OPT_ADV_NORM_MINIBATCH, kl_penalty=pkg.OPT_KL_PENALTY)[which]
    configure = (lambda eng: eng.set_kl_coef(0.2)) if which == "kl_penalty" else None
    for prec in ("fp32", "bf16"):
        _probe_vs_train(pkg, prec, N, 2, A, 32, options=[(opt, 1)], configure=configure, vold=vold, seed=8300)


def _everything(pkg, eng, m, epochs, M, **read):
    out = uh.read_update(eng, m, epochs, M, state=True, **read)
    out["digest"] = np.array(list(eng.state_digest().values()), np.uint64)
    out["tensor_stats"] = eng.tensor_stats("all", raw=True)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("batch", ["caller", "caller_options", "rollout_options"])
def test_probe_changes_nothing(pkg, graph, batch):
    """_options: value clipping, per-minibatch advantage normalisation and the KL penalty on - the probe then reads the old
    values (a rollout batch: it transposes them into the plane aleppo_train transposes them into), forms its own advantage
    record and reads its own beta"""
    from test_gpu_at_size import DeviceBytes, _flags
    E, T, A, H, epochs, M = 8, 16, 6, 64, 2, 2
    N, B = E * T, E * T // M
    on = batch != "caller"
    params = hf.fill_params(8400, H, A)
    caller = _hashed(8401, N, A)
    vold = hf.hf_range(8402, (N,), -1, 1)
    frames = hf.hf_bytes(8403, (T, E, 84, 84))
    te, tr, st = _flags(8404, T, E)
    rew = hf.hf_range(8405, (T, E), -2, 2)
    options = [(pkg.OPT_UPDATE_GRAPH, graph)]
    if on:
        options += [(pkg.OPT_VALUE_CLIP, 1), (pkg.OPT_ADV_NORM_MINIBATCH, 1), (pkg.OPT_KL_PENALTY, 1)]
    read = dict(kl=on, adv_stats=on)
    outs = {}
    for probing in (False, True):
        eng = uh.make_engine(pkg, E, T, A, H, pkg.BF16, options, max_minibatch=B, seed=3)
        if on:
            eng.set_kl_coef(0.2)
        eng.load_params(params)
        if batch == "rollout_options":
            dev = DeviceBytes(frames)
            eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
            eng.finish_rollout()
            dev.free()
        else:
            eng.set_batch(*caller, values=vold if on else None)
        for _ in range(2):  # (captured: the first call of a shape runs eagerly, the second records)
            m = eng.train(2.5e-4, epochs, M)
        replays = eng.get_option(pkg.OPT_UPDATE_GRAPH)
        assert replays == graph
        if probing:
            before = _everything(pkg, eng, m, epochs, M, **read)
            assert eng.grad_probe(1, first=5, n=37, policy=False, value_loss_coef=1.0, entropy_coef=0.0) > 0
            assert eng.grad_probe(0, n=B) > 0 and np.abs(eng.grad_vector(0)).max() > 0
            eng.gradient_interference(first=0, n=37)
            uh.assert_identical(before, _everything(pkg, eng, m, epochs, M, **read))
        m = eng.train(2.5e-4, epochs, M)
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) == (replays + 1 if graph else 0)  # a replay, not a re-capture
        outs[probing] = _everything(pkg, eng, m, epochs, M, **read)
        eng.close()
    uh.assert_identical(outs[False], outs[True])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_terms_separate_exactly(pkg, prec):
    N, A, H = 37, 5, 32
    eng = _engine(pkg, N, A, H, prec)
    eng.load_params(hf.fill_params(8500, H, A))
    eng.set_batch(*_hashed(8501, N, A))
    eng.grad_probe(0, policy=False, value_loss_coef=1.0, entropy_coef=0.0)
    eng.grad_probe(1, policy=True, value_loss_coef=1.0, entropy_coef=0.0)
    eng.grad_probe(2, policy=True, value_loss_coef=0.0, entropy_coef=0.0)
    v, pv, p = (eng.grad_vector(s) for s in range(3))
    eng.close()
    spans = gp.bounds(H, A)
    for r in (8, 9):  # action.w, action.b: exactly 0 (either sign) without the policy and entropy terms
        b, e = spans[r]
        assert (v[b:e] == 0).all() and np.abs(pv[b:e]).max() > 0
    for r in (10, 11):  # value.w, value.b: the bits of the probe with the policy term, and exactly 0 without a value term
        b, e = spans[r]
        np.testing.assert_array_equal(_bits(v[b:e]), _bits(pv[b:e]))
        assert np.abs(v[b:e]).max() > 0 and (p[b:e] == 0).all()
    assert np.abs(v[:spans[8][0]]).max() > 0 and np.abs(p[:spans[8][0]]).max() > 0  # both reach the trunk


CASES = dict(policy=(1, 0.0, 0.0), value=(0, 1.0, 0.0), entropy=(0, 0.0, 1.0), mixed=(1, 0.25, 0.03))


@functools.lru_cache(maxsize=None)
def _composed(prec, case):
    """the composed reference's gradient of samples [5, 42) of the 74-sample batch, once per (precision, case)"""
    H, A = 32, 4
    policy, c_v, c_e = CASES[case]
    obs, actions, old_lp, adv, ret, masks = (a[5:42] for a in _hashed(8601, 74, A))
    if not policy:
        adv = np.zeros_like(adv)
    ref = ur.composed_train(hf.fill_params(8600, H, A), H, A, obs, actions, old_lp, adv, ret, masks, 1, 1, lr=0.0,
                            max_norm=1e30, c_v=c_v, c_e=c_e, emulate_bf16=prec == "bf16")
    return ref["last_grads"]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_probe_against_the_composed_reference(pkg, prec):
    """a slice that is no minibatch of any M: first = 5, n = 37 of N = 74"""
    N, A, H = 74, 4, 32
    eng = _engine(pkg, N, A, H, prec, 2, T=2)
    eng.load_params(hf.fill_params(8600, H, A))
    eng.set_batch(*_hashed(8601, N, A))
    got = {}
    for case, (policy, c_v, c_e) in CASES.items():
        eng.grad_probe(0, first=5, n=37, policy=bool(policy), value_loss_coef=c_v, entropy_coef=c_e)
        got[case] = eng.grad_vector(0)
        want = _composed(prec, case)
        atol = 1e-4 if prec == "fp32" else 1e-5 + 2e-3 * float(np.abs(want).max())
        err = float(np.abs(got[case] - want).max())
        print(f"{prec} {case}: max |g - ref| = {err:.3g} (atol {atol:.3g}, max |ref| = {np.abs(want).max():.3g})")
        np.testing.assert_allclose(got[case], want, atol=atol, rtol=0, err_msg=case)
    eng.close()
    if prec == "fp32":  # g(1, c_v, c_e) = g_pi + c_v g_v + c_e g_e to rounding, formed from the three pure probes
        comb = got["policy"].astype(np.float64) + 0.25 * got["value"] + 0.03 * got["entropy"]
        np.testing.assert_allclose(got["mixed"], comb, atol=1e-4, rtol=0)


@pytest.mark.gpu
def test_grad_take_and_the_helpers(pkg):
    N, A, H = 74, 4, 32
    eng = _engine(pkg, N, A, H, "bf16", 2, T=2)
    eng.load_params(hf.fill_params(8700, H, A))
    eng.set_batch(*_hashed(8701, N, A))
    eng.snapshot_take("live")
    eng.train(2.5e-4, 1, 2)
    sd = eng.state_dict()
    eng.grad_take(0, "exp_avg")
    np.testing.assert_array_equal(_bits(eng.grad_vector(0)), _bits(sd["exp_avg"]))
    eng.grad_take(1, "delta", "snapshot")
    want = (sd["params"] - eng.snapshot_params()).astype(np.float32)  # one fp32 subtraction per element
    assert np.abs(want).max() > 0
    np.testing.assert_array_equal(_bits(eng.grad_vector(1)), _bits(want))
    # the momentum against a fresh gradient, from one Gram
    eng.grad_probe(2, n=37)
    cos = pkg.Engine.grad_cosines(eng.grad_gram([0, 2]))
    assert -1.0 <= cos["all"][0, 1] <= 1.0
    # the two composite helpers return the host arithmetic on grad_gram of the slots they filled
    ns = eng.gradient_noise_scale(20, 74 // 2)
    b_small, b_big = ns.pop("counts")
    assert 0 < b_small < b_big <= 37
    np.testing.assert_equal(ns, pkg.Engine.noise_scale_from_gram(eng.grad_gram([0, 1]), b_small, b_big))
    assert np.isfinite(ns["b_simple"]["all"])
    gi = eng.gradient_interference(first=3, n=30)
    np.testing.assert_equal(gi, pkg.Engine.interference_from_gram(eng.grad_gram([0, 1, 2])))  # (NaN == NaN here)
    assert gi["norms"]["value"]["action.w"] == 0.0 and np.isnan(gi["cosines"]["policy_value"]["action.w"])
    assert -1.0 <= gi["cosines"]["policy_value"]["fc.w"] <= 1.0
    eng.close()


def _raw_probe(pkg, eng, slot, first, n, cfg=None):
    count = C.c_int64(-7)
    c = None if cfg is None else C.byref(pkg.GradProbeConfig(*cfg))
    rc = pkg.lib().aleppo_grad_probe(eng._ctx, C.c_int(slot), C.c_int64(first), C.c_int64(n), c, C.byref(count))
    assert rc == pkg.OK or count.value == -7
    return rc


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    E, T, A, H = 8, 8, 4, 32
    N = E * T
    INV, RUN = pkg.ERR_INVALID_ARGUMENT, pkg.ERR_RUNTIME
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, max_minibatch=40)
    lib, ctx = pkg.lib(), eng._ctx
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    eng.load_params(hf.fill_params(8800, H, A))
    flat = np.full(eng.param_count, -7.0, np.float32)
    gram, nfc = np.full(13 * 16, -7.0), np.full(13, -7, np.int64)
    slots = np.array([0, 1, 2, 3], np.int32)

    def raw_gram(sl, k, gcount, ncount, nf=True):
        rc = lib.aleppo_grad_gram(ctx, None if sl is None else p(sl), C.c_int(k), p(gram), C.c_size_t(gcount),
                                  p(nfc) if nf else None, C.c_size_t(ncount))
        assert rc == pkg.OK or ((gram == -7).all() and (nfc == -7).all())
        return rc

    # nothing written yet, no batch yet
    assert lib.aleppo_grad_export(ctx, C.c_int(0), p(flat), C.c_size_t(flat.size)) == RUN and (flat == -7).all()
    assert raw_gram(slots, 1, 13, 13) == RUN
    assert _raw_probe(pkg, eng, 0, 0, 8) == RUN
    assert lib.aleppo_grad_take(ctx, C.c_int(0), C.c_int(pkg.GRAD_SRC_PARAM_DELTA), C.c_int(pkg.SET_SNAPSHOT)) == RUN
    assert lib.aleppo_grad_take(ctx, C.c_int(0), C.c_int(pkg.GRAD_SRC_PARAM_DELTA), C.c_int(pkg.SET_AVERAGED)) == RUN
    assert lib.aleppo_grad_export(ctx, C.c_int(0), p(flat), C.c_size_t(flat.size)) == RUN  # the failed takes wrote none
    batch = _hashed(8801, N, A)
    eng.set_batch(*batch)
    x = hf.hf_range(8802, (eng.param_count,), -1, 1)
    eng.load_grad(0, x)
    eng.train(2.5e-4, 1, 2)
    state = lambda: (eng.grad_vector(0), eng.export_grads(), eng.export_params(), eng.state_dict()["exp_avg"],
                     np.array(list(eng.state_digest().values()), np.uint64))
    before = state()
    # slots
    for s in (-1, 4):
        assert _raw_probe(pkg, eng, s, 0, 8) == INV
        assert lib.aleppo_grad_take(ctx, C.c_int(s), C.c_int(0), C.c_int(0)) == INV
        assert lib.aleppo_grad_export(ctx, C.c_int(s), p(flat), C.c_size_t(flat.size)) == INV
        assert lib.aleppo_grad_import(ctx, C.c_int(s), p(x), C.c_size_t(x.size)) == INV
        assert raw_gram(np.array([0, s], np.int32), 2, 52, 13) == INV
    # the slice: maxB = 40, N = 64
    for first, n in ((0, 0), (0, -1), (0, 41), (-1, 8), (60, 8), (64, 1), (2 ** 40, 1), (0, 2 ** 40)):
        assert _raw_probe(pkg, eng, 0, first, n) == INV, (first, n)
    # cfg
    for cfg in ((2, 0.5, 0.01, 0), (-1, 0.5, 0.01, 0), (1, -0.5, 0.01, 0), (1, 0.5, -1e-9, 0), (1, float("nan"), 0.0, 0),
                (1, 0.5, float("inf"), 0), (1, 0.5, 0.01, 1)):
        assert _raw_probe(pkg, eng, 0, 0, 8, cfg) == INV, cfg
    # take
    for src, which in ((2, 0), (-1, 0), (pkg.GRAD_SRC_EXP_AVG, 1), (pkg.GRAD_SRC_PARAM_DELTA, pkg.SET_LIVE),
                       (pkg.GRAD_SRC_PARAM_DELTA, 3)):
        assert lib.aleppo_grad_take(ctx, C.c_int(0), C.c_int(src), C.c_int(which)) == INV, (src, which)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.grad_take(0, "gradient")
    # export / import / gram: counts and pointers, slots that nothing has written
    for ptr, cnt in ((None, flat.size), (p(flat), flat.size - 1), (p(flat), 0)):
        assert lib.aleppo_grad_export(ctx, C.c_int(0), ptr, C.c_size_t(cnt)) == INV and (flat == -7).all()
        assert lib.aleppo_grad_import(ctx, C.c_int(0), ptr, C.c_size_t(cnt)) == INV
    assert lib.aleppo_grad_export(ctx, C.c_int(1), p(flat), C.c_size_t(flat.size)) == RUN and (flat == -7).all()
    for sl, k, gc, nc, nf in ((None, 1, 13, 13, True), (slots, 0, 0, 13, True), (slots, 5, 13 * 25, 13, True),
                              (slots, 1, 12, 13, True), (slots, 1, 13, 12, True), (slots, 1, 13, 13, False),
                              (slots, 1, 13 * 4, 13, True)):
        assert raw_gram(sl, k, gc, nc, nf) == INV, (k, gc, nc, nf)
    assert raw_gram(slots, 2, 52, 13) == RUN  # slot 1 is not written
    assert raw_gram(slots, 1, 13, 0, nf=False) == pkg.OK and gram[0] >= 0 and (gram[13:] == -7).all()
    gram[:] = -7
    # value clipping on a caller batch without values
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    assert _raw_probe(pkg, eng, 0, 0, 8) == RUN
    eng.set_option(pkg.OPT_VALUE_CLIP, 0)
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(a, b)
    # while a step is armed: every call is refused
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(8803, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    assert _raw_probe(pkg, eng, 0, 0, 8) == RUN
    assert lib.aleppo_grad_take(ctx, C.c_int(0), C.c_int(0), C.c_int(0)) == RUN
    assert lib.aleppo_grad_export(ctx, C.c_int(0), p(flat), C.c_size_t(flat.size)) == RUN and (flat == -7).all()
    assert lib.aleppo_grad_import(ctx, C.c_int(0), p(x), C.c_size_t(x.size)) == RUN
    assert raw_gram(slots, 1, 13, 13) == RUN
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    np.testing.assert_array_equal(eng.grad_vector(0), x)
    eng.close()
