"""The tail of every update - sumsq_kernel, adam_kernel, aleppo_export_grads - element by element at fp32 rounding
bounds (tests/adam_ref.py), and what adam_kernel writes besides the parameters, bit for bit.

CPU (not marked gpu): the bounds hold with room for plain fp32 arithmetic and reject the classic Adam mistakes.
GPU: every element of both moments and of the parameters after a step against the float64 restatement of that step on
the engine's own exported inputs; the clip regimes; the reported norm; the bf16 / transposed weight copies of
adam_kernel against the copies a fresh engine builds at load time; the schedule slots of a multi-step call."""
import functools

import numpy as np
import pytest

import adam_ref as ar
import hashfill as hf

LR = 2.5e-4
N = 64  # E = 8, T = 8
T_STEPS = (1, 2, 10, 1000, 10 ** 6)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ CPU: the bounds themselves
def test_fp32_restatement_within_half_of_every_bound():
    """adam_element in plain numpy float32 (no fused multiply-add, correctly rounded division and root) must sit within
    0.5 of every bound: the bounds are twice the plain operation count.  Fails if a bound of adam_ref is tightened below
    what plain fp32 needs.  |g| in 1e-12 .. 10, |m0| in 1e-12 .. 1, v0 in 1e-24 .. 1, every third g zero, zero moments,
    m0 = -0.11 g on half of the elements (cancellation in m), t = 1, 2, 10, 1000, 10^6."""
    n = 1 << 18
    worst = {q: 0.0 for q in ar.QUANTITIES}
    for k, t in enumerate(T_STEPS):
        p0, m0, v0, g = ar.hashed_step_inputs(7000 + 100 * k, n)
        assert (g == 0).sum() >= n // 3 and ((m0 == 0) & (v0 == 0)).sum() > n // 8
        assert ((m0 != 0) & (np.sign(m0) == -np.sign(g))).sum() > n // 4
        r = ar.ratios((p0, m0, v0), ar.adam_element_f32(p0, m0, v0, g, t, LR), g, t, LR)
        for q in ar.QUANTITIES:
            worst[q] = max(worst[q], float(r[q].max()))
    print("fp32 restatement, worst ratio to bound:", {q: "%.3g" % x for q, x in worst.items()})
    for q in ar.QUANTITIES:
        assert worst[q] <= 0.5, (q, worst[q])
        assert worst[q] > 0.1, (q, worst[q])  # (the inputs do exercise the bound)


def _mutations():
    """name -> function(p0, m0, v0, g, t) -> (p, m, v) in float64: the step with one classic mistake"""
    def scalars(t):
        return ar.step_scalars(t, LR)

    def eps_inside(p0, m0, v0, g, t):
        s, c = scalars(t)
        p, m, v, _ = ar.adam_f64(p0, m0, v0, g, s, c)
        d = np.sqrt(v / float(c) ** 2 + float(ar.EPS))
        return np.asarray(p0, np.float64) - float(s) * m / d, m, v

    def unclamped(p0, m0, v0, g, t):  # max_norm / norm = 1 / 0.5 applied although it exceeds 1; the export says g
        return ar.adam_f64(p0, m0, v0, np.asarray(g, np.float64) / 0.5, *scalars(t))[:3]

    return {
        "eps = 1e-8": lambda p0, m0, v0, g, t: ar.adam_f64(p0, m0, v0, g, *scalars(t), eps=1e-8)[:3],
        "eps inside the square root": eps_inside,
        "t + 1 in both corrections": lambda p0, m0, v0, g, t: ar.adam_f64(p0, m0, v0, g, *scalars(t + 1))[:3],
        "t - 1 in both corrections": lambda p0, m0, v0, g, t: ar.adam_f64(p0, m0, v0, g, *scalars(t - 1))[:3],
        "no sqrt(1 - beta2^t)": lambda p0, m0, v0, g, t: ar.adam_f64(p0, m0, v0, g, scalars(t)[0], 1.0)[:3],
        "coef not clamped to 1": unclamped,
    }


def test_checker_rejects_each_mutation():
    """every listed mistake, applied to the float64 step and rounded to fp32 like a device result, is rejected on at least
    20 % of the elements at t = 2 (elements with g = m0 = 0 do not move under any of them, and a large denominator hides a
    changed eps), and the unmutated step on none"""
    n, t = 1 << 18, 2
    p0, m0, v0, g = ar.hashed_step_inputs(7700, n)
    offs = np.linspace(0, n, 13).astype(np.int64)

    def rejected(after):
        r = ar.ratios((p0, m0, v0), tuple(a.astype(np.float32) for a in after), g, t, LR)
        return np.mean(np.maximum(np.maximum(r["m"], r["v"]), r["p"]) > 1.0)

    assert rejected(ar.adam_f64(p0, m0, v0, g, *ar.step_scalars(t, LR))[:3]) == 0.0
    shares = {}
    for name, step in _mutations().items():
        after = tuple(a.astype(np.float32) for a in step(p0, m0, v0, g, t))
        shares[name] = rejected(after)
        assert ar.check_step((p0, m0, v0), after, g, t, LR, offs).failures, name
    print("share of elements rejected:", {k: "%.3g" % v for k, v in shares.items()})
    for name, share in shares.items():
        assert share >= 0.2, (name, share)


def test_checker_reports_tensor_and_index_and_exact_zeros():
    """one wrong element is named by tensor and index; where a bound is exactly 0 any difference fails"""
    H, A = 32, 4
    offs = ar.param_offsets(H, A)
    n = int(offs[-1])
    assert n == hf.fill_params(1, H, A).size
    p0, m0, v0, g = ar.hashed_step_inputs(7800, n)
    p, m, v = ar.adam_element_f32(p0, m0, v0, g, 3, LR)
    assert not ar.check_step((p0, m0, v0), (p, m, v), g, 3, LR, offs).failures
    i = int(offs[6]) + 1234  # fc.w
    bad = p.copy()
    bad[i] += np.float32(1e-3)
    res = ar.check_step((p0, m0, v0), (bad, m, v), g, 3, LR, offs)
    assert [(f[0], f[1], f[3]) for f in res.failures] == [("fc.w", "p", 1234)]
    assert res.worst["p"][1:] == ("fc.w", 1234) and "fc.w[1234]" in res.summary("x")
    z = np.flatnonzero((m0 == 0) & (v0 == 0) & (g == 0))
    assert z.size
    for q, arr in (("m", m), ("v", v)):
        bad = arr.copy()
        bad[z[0]] = np.float32(1e-45)  # the smallest subnormal
        after = (p, bad, v) if q == "m" else (p, m, bad)
        res = ar.check_step((p0, m0, v0), after, g, 3, LR, offs)
        assert len(res.failures) == 1 and res.failures[0][1] == q and res.failures[0][2] == np.inf


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    p = load_package()
    p.lib()
    return p


@functools.lru_cache(maxsize=None)
def _obs(seed, n):
    a = hf.hf_bytes(seed, (n, 4, 84, 84))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _batch(seed, n, A):
    """a hashed batch as in test_train_vs_oracle: (obs, actions, old log-probs, advantages, returns, masks)"""
    import oracle_lib as orc
    return (_obs(seed + 1, n), (hf.hf_u32(seed + 2, n) % np.uint32(A)).astype(np.int64),
            orc.log_softmax(hf.hf_range(seed + 3, (n, A), -1, 1)), hf.hf_range(seed + 4, (n,), -1, 1),
            hf.hf_range(seed + 5, (n,), -1, 1), (hf.hf_unit(seed + 6, n) >= np.float32(0.1)).astype(np.uint8))


def _state(eng):
    sd = eng.state_dict()
    return (sd["params"], sd["exp_avg"], sd["exp_avg_sq"]), int(sd["step"])


def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


# H = 32, 96, 480: a 32-row last tile in adam_kernel's walk of Wfc; A = 1 / 6 / 18 move the start of every flat range
MATRIX = [("fp32", 32, 4), ("fp32", 96, 18), ("bf16", 32, 1), ("bf16", 96, 6), ("bf16", 480, 18), ("bf16", 512, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,H,A", MATRIX)
def test_every_element_of_a_step(pkg, prec, H, A):
    """steps t = 1, 2, 3 from load_params, each on another batch, then one step at t = 10^6 from imported hashed moments
    (|m0| in 1e-12 .. 1, v0 in 1e-24 .. 1, a fifth of them zero; not a reachable state - the check is per element): around
    every step the parameters, both moments and the scaled gradient are exported, and every element of all 12 tensors
    must be within adam_ref's bounds of the float64 step on those inputs"""
    eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec))
    offs = ar.param_offsets(H, A)
    eng.load_params(hf.fill_params(6100, H, A))
    total = ar.StepCheck()
    before, step = _state(eng)
    assert step == 0 and not before[1].any() and not before[2].any()

    def take(t, seed):
        nonlocal before
        eng.set_batch(*_batch(seed, N, A))
        m = eng.train(LR, 1, 1)
        assert np.isfinite(m["loss"]).all() and np.isfinite(m["grad_norm"]).all()
        after, step = _state(eng)
        assert step == t
        g = eng.export_grads()
        assert np.abs(g).max() > 0
        res = ar.check_step(before, after, g, t, LR, offs)
        total.merge(res)
        before = after
        return res

    for t in (1, 2, 3):
        take(t, 6100 + 10 * t)
    m0, v0 = ar.hashed_moments(6200, before[0].size)
    eng.load_state_dict(dict(params=before[0], exp_avg=m0, exp_avg_sq=v0, step=10 ** 6 - 1))
    params = before[0]
    before, step = _state(eng)
    assert step == 10 ** 6 - 1
    for got, want in zip(before, (params, m0, v0)):  # an import followed by an export returns the imported bits
        assert np.array_equal(_bits(got), _bits(want))
    take(10 ** 6, 6150)
    eng.close()
    print(total.summary(f"adam step {prec} H={H} A={A}, t = 1, 2, 3, 1e6: worst ratio to bound"))
    assert not total.failures, total.failures[:8]


@pytest.mark.gpu
def test_clip_regimes(pkg):
    """the same first step (H = 96, bf16, zero moments) under four gradient-norm limits: 1e6 (coef exactly 1: the export
    is the raw gradient), the default 0.5, the pre-clip norm itself (coef = norm / (norm + 1e-6), just below 1) and 1e-3.
    The third regime exists only while norm < 32: from there on norm + 1e-6 rounds back to norm in fp32 and coef is
    exactly 1.  With fill_params as it is the norm at H = 96 is 30 - 34 (measured on the MI355X, whatever the scale of the
    advantages), so the parameters are fill_params x 0.7, where it is 2.2; the test asserts 0.5 < norm < 16.
    In the last regime the scaled gradient's norm is <= 1e-3, so at most 1e-6 / 1e-10 = 10^4 of the 3 x 10^5 elements
    can exceed eps = 1e-5, and at t = 1 with zero moments sqrt(v) / c = |g|: eps dominates the denominator on more than
    90 % of the elements."""
    H, A = 96, 6
    params = hf.fill_params(6300, H, A) * np.float32(0.7)
    offs = ar.param_offsets(H, A)
    eng = pkg.Engine(8, 8, A, H, precision=pkg.BF16)
    total = ar.StepCheck()

    def run(max_norm):
        eng.load_params(params)
        eng.set_hyper(max_grad_norm=max_norm)
        before, _ = _state(eng)
        eng.set_batch(*_batch(6310, N, A))
        m = eng.train(LR, 1, 1)
        after, step = _state(eng)
        assert step == 1
        g = eng.export_grads()
        res = ar.check_step(before, after, g, 1, LR, offs)
        total.merge(res)
        assert not res.failures, (max_norm, res.failures[:8])
        return m["grad_norm"][0, 0], g

    norm, raw = run(1e6)
    assert ar.clip_coef(1e6, norm) == 1.0 and 0.5 < norm < 16
    np.testing.assert_allclose(norm, np.linalg.norm(raw.astype(np.float64)), rtol=1e-5)  # (raw it is; tightly below)
    coefs = {}
    for name, max_norm in (("default", 0.5), ("norm", float(norm)), ("tiny", 1e-3)):
        n2, g = run(max_norm)
        assert _bits(n2) == _bits(norm)
        coef = coefs[name] = ar.clip_coef(max_norm, norm)
        assert np.array_equal(_bits(g), _bits(raw * coef)), name
    eng.close()
    print(total.summary(f"clip regimes norm={norm:.6g} coef={ {k: float(v) for k, v in coefs.items()} }: worst ratio"))
    assert coefs["default"] < 1.0 and coefs["default"] == np.float32(0.5) / (norm + np.float32(1e-6))
    assert 1.0 - 1e-5 < coefs["norm"] < 1.0
    assert coefs["tiny"] < 2e-3
    assert np.mean(np.abs(g) < float(ar.EPS)) > 0.9


# the summation depth of the reported norm (see test_reported_norm)
NORM_DEPTH = 1 + 16 + 6 + 2 + 4 + 6 + 2


@pytest.mark.gpu
@pytest.mark.parametrize("prec,H,A", MATRIX)
def test_reported_norm(pkg, prec, H, A):
    """with coef = 1 (limit 1e6) the export is the raw gradient, and the reported pre-clip norm is its norm.  Depth of
    the sum, in fp32 roundings that one term can pass through: the square (1); a sumsq_kernel thread's running sum over
    its <= 16 terms (a block owns <= 4096 elements: nblk = ceil(n / 4096) <= 800 for every H <= 512) (16); the block
    tree - six wave shuffles and the two levels over the four waves (6 + 2); adam_kernel's re-reduction - <= 4 of the
    <= 1024 partials per thread (4) and the same block tree (6 + 2): d = 37.  The tail blocks (conv1) are shallower.
    All terms are >= 0, so the sum is within d u relative, the root halves that and rounds once more:
    rtol = (d / 2 + 1) 2^-24 = 1.2e-6."""
    rtol = (NORM_DEPTH / 2 + 1) * ar.U
    assert NORM_DEPTH == 37 and rtol < 4e-6
    eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec))
    assert (eng.param_count + 4095) // 4096 <= 800
    eng.load_params(hf.fill_params(6400, H, A))
    eng.set_hyper(max_grad_norm=1e6)
    eng.set_batch(*_batch(6410, N, A))
    norm = eng.train(LR, 1, 1)["grad_norm"][0, 0]
    want = np.linalg.norm(eng.export_grads().astype(np.float64))
    eng.close()
    err = abs(float(norm) / want - 1)
    print(f"reported norm {prec} H={H} A={A}: {norm:.8g} vs {want:.10g}, rel {err:.3g}/{rtol:.3g}")
    assert norm < 1e6 and err <= rtol


def _bf16_bits(x):
    b = _bits(x).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)


# (prec, H, N, OPT_FUSED_BWD or None): N = 520 takes the pipelined fc dgrad (reads WfcT), the fused tail reads W2d
COPIES = [(prec, H, 64, None) for prec in ("bf16", "fp32") for H in (32, 96, 480, 512)]
COPIES += [("bf16", 480, 520, None), ("bf16", 96, 64, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,H,n,fused", COPIES)
def test_copies_adam_writes_match_load_time_copies(pkg, prec, H, n, fused):
    """engine X takes two steps, so its bf16 compute copy and its transposed dgrad-side layouts (WfcT, W3d, W2d) are the
    ones adam_kernel wrote; engine Y is fresh and loads X's state, so its copies come from launch_cast_params /
    launch_pack_dgrad on the same fp32 parameters.  A forward on 37 observations and one more step must then agree bit for
    bit in everything.  The steps run at lr = 1e-2 so that a stale or misplaced tile differs from the right one in bf16
    too: bf16(p) must have changed on more than 90 % of the entries of fc.w, conv3.w and conv2.w.
    From zero moments that share is not reachable at any rate: 10 - 18 % of fc.w and conv3.w and 2 - 4 % of conv2.w have a
    gradient of exactly 0 on 64 hashed samples (inputs and channels the ReLUs keep off), and Adam does not move them -
    measured on the MI355X at lr = 1e-2 / 4e-2 / 0.2: fc.w 81 - 88 / 82 - 89 / 84 - 90 % changed, conv3.w 87 - 90 % at
    all three, the unchanged entries being the ones whose exp_avg is still 0.  So X starts from an imported optimizer
    state in which every entry is moving: exp_avg = +-1e-4 (hashed sign), exp_avg_sq = 1e-8, step 10.  Steps 11 and 12
    then move an entry without gradient by 0.14 lr each (s = lr / (1 - 0.9^11), c = sqrt(1 - 0.999^11) = 0.105:
    s 0.9e-4 / (1e-4 / c)), together 2.7e-3 = 5 bf16 ulps of a weight below 0.1: measured 98.8 - 99.9 % changed."""
    A, lr = 6, 1e-2
    offs = ar.param_offsets(H, A)
    params = hf.fill_params(6500, H, A)
    engines = [pkg.Engine(n // 8, 8, A, H, precision=_prec(pkg, prec)) for _ in range(2)]
    for eng in engines:
        if fused is not None:
            eng.set_option(pkg.OPT_FUSED_BWD, fused)
    x, y = engines
    sign = np.where(hf.hf_u32(6501, params.size) & np.uint32(1), -1.0, 1.0)
    x.load_state_dict(dict(params=params, exp_avg=(1e-4 * sign).astype(np.float32),
                           exp_avg_sq=np.full(params.size, 1e-8, np.float32), step=10))
    for seed in (6510, 6520):
        x.set_batch(*_batch(seed, n, A))
        x.train(lr, 1, 1)
    sd = x.state_dict()
    assert int(sd["step"]) == 12
    changed = {}
    for k in (6, 4, 2):
        sl = slice(offs[k], offs[k + 1])
        changed[ar.NAMES[k]] = float(np.mean(_bf16_bits(sd["params"][sl]) != _bf16_bits(params[sl])))
    y.load_state_dict(sd)
    out = []
    for eng in engines:
        logits, values = eng.forward(_obs(6531, 37))
        eng.set_batch(*_batch(6540, n, A))
        m = eng.train(lr, 1, 1)
        (p, m1, m2), step = _state(eng)
        assert step == 13
        out.append(dict(logits=logits, values=values, loss=m["loss"], norm=m["grad_norm"], grads=eng.export_grads(),
                        params=p, exp_avg=m1, exp_avg_sq=m2))
        eng.close()
    diff = {k: int(np.sum(_bits(out[0][k]) != _bits(out[1][k]))) for k in out[0]}
    print(f"adam-written copies vs load-time copies {prec} H={H} N={n} fused_bwd={fused}: differing elements {diff}, "
          f"bf16(p) changed {changed}")
    assert all(share > 0.9 for share in changed.values()), changed
    for k, d in diff.items():
        if d:
            i = int(np.flatnonzero(_bits(out[0][k]).ravel() != _bits(out[1][k]).ravel())[0])
            tensor = ""
            if out[0][k].size == offs[-1]:
                t = int(np.searchsorted(offs, i, side="right")) - 1
                tensor = f" ({ar.NAMES[t]}[{i - offs[t]}])"
            pytest.fail(f"{k}: {d} elements differ, first at {i}{tensor}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_schedule_slots_match_single_step_calls(pkg, prec):
    """adam_sched + 2 mi gives each step of one aleppo_train call its own slot of device scalars, separate calls always
    use slot 0: train(lr, 3, 1) and three train(lr, 1, 1) on the same batch leave the same bits"""
    H, A = 96, 6
    res = []
    for calls in ((3,), (1, 1, 1)):
        eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec))
        eng.load_params(hf.fill_params(6600, H, A))
        eng.set_batch(*_batch(6610, N, A))
        ms = [eng.train(LR, epochs, 1) for epochs in calls]
        state, step = _state(eng)
        res.append((state, step, np.concatenate([m["loss"] for m in ms]), np.concatenate([m["grad_norm"] for m in ms])))
        eng.close()
    (s1, t1, l1, n1), (s3, t3, l3, n3) = res
    assert t1 == t3 == 3 and l1.shape == l3.shape == (3, 1)
    diff = {name: int(np.sum(_bits(a) != _bits(b)))
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "loss", "norm"), s1 + (l1, n1), s3 + (l3, n3))}
    print(f"one 3-step call vs three 1-step calls {prec}: differing elements {diff}")
    assert not any(diff.values()), diff
    assert not np.array_equal(_bits(l1[0]), _bits(l1[2]))  # (the steps do differ from each other)
