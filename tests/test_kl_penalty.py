"""ALEPPO_OPT_KL_PENALTY / ALEPPO_OPT_KL_COEF (the PPO paper's KL penalty beta KL(pi_old || pi) with the exact categorical
KL) and the read-back fields ALEPPO_M_KL / ALEPPO_M_MEAN_KL.

CPU: the header constants against the Python mirror, the composed reference (update_ref.py) against orc.train with
beta = 0, the gradient formula against torch autograd, and the trainer's kl_coef / kl_target keys against the host-only
library stand-in.
GPU (-m gpu, everything through the C ABI): the penalised update against the composed reference in fp32, in bf16 at
BASELINE configs[1]'s update, on rollout batches with fp32 and fp16 planes (sum q != 1), and together with value clipping,
per-minibatch advantage normalisation and shuffling; eager, graph-replayed, 1-rank-communicator and split-epoch schedules
bit-identical; beta changed between graph replays; beta = 0 bit-identical to the option off; the error cases; the trainer
on the device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
import update_harness as uh
import update_ref as ur
from shared_fixtures import pkg, stub_trainer, trainer  # noqa: F401
from trainer_helpers import debug_cfg as _debug_cfg, event_scalars, events as _events, header_const as const, run_stub
from update_harness import PER_SAMPLE, assert_identical
from __graft_entry__ import load_package

LR = 2e-5  # (small, like test_value_clip.py: the policy stays near the batch's, and the KL term stays comparable)
BETA = 0.2
KL = ("kl", "mean_kl")  # what only the option writes: absent from a run with it off
read_kl = functools.partial(uh.read_update, kl=True)


# ------------------------------------------------------------------ CPU
def test_header_constants_and_python_mirror():
    pkg = load_package()
    assert const("ALEPPO_OPT_KL_PENALTY") == pkg.OPT_KL_PENALTY == 15
    assert const("ALEPPO_OPT_KL_COEF") == pkg.OPT_KL_COEF == 16
    assert const("ALEPPO_M_KL") == pkg.METRIC_FIELDS["kl"] == 11
    assert const("ALEPPO_M_MEAN_KL") == pkg.METRIC_MEAN_FIELDS["kl"] == 12
    assert hasattr(pkg.Engine, "set_kl_coef") and hasattr(pkg.Engine, "kl_coef")
    assert hasattr(pkg.Engine, "kl_divergence")


def _hashed(seed, N, A, distinct=None):
    return uh.hashed_batch(seed, N, A, mask_p=0.15, distinct=distinct)


@pytest.mark.parametrize("bf16", [False, True])
def test_composed_reference_with_beta_zero_is_the_oracle(bf16):
    H, A, N, epochs, M = 32, 6, 48, 2, 3
    params = hf.fill_params(6100, H, A)
    batch = _hashed(6101, N, A)
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=0.0, emulate_bf16=bf16)
    o = orc.train(params, H, A, *batch, epochs, M, emulate_bf16=bf16)
    for k in ("params", "loss", "grad_norm", "total_losses", "ratio", "entropies", "value_losses", "clipped",
              "last_grads"):
        np.testing.assert_array_equal(ref[k], o[k], err_msg=k)
    assert (ref["kl"] > 0).all() and np.isfinite(ref["mean_kl"]).all()
    # and beta != 0 changes the update
    on = ur.composed_train(params, H, A, *batch, epochs, M, beta=BETA, emulate_bf16=bf16)
    assert not np.allclose(on["params"], o["params"], atol=1e-7, rtol=0)
    np.testing.assert_allclose(on["total_losses"][0, 0] - o["total_losses"][0, 0], BETA * on["kl"][0, 0], rtol=1e-5,
                               atol=1e-6)


@pytest.mark.parametrize("fp16", [False, True])
def test_gradient_formula_is_torch_autograd(fp16):
    """d/dz of beta sum_a q_a (olp_a - log_softmax(z)_a) is beta (p S - q), in float64; with old log-probs rounded to
    fp16 S != 1 and the formula is still exact"""
    torch = pytest.importorskip("torch")
    B, A = 64, 18
    z = hf.hf_range(6200, (B, A), -3, 3).astype(np.float64)
    olp = orc.log_softmax(hf.hf_range(6201, (B, A), -2, 2))
    if fp16:
        olp = olp.astype(np.float16).astype(np.float32)
    S = np.exp(olp.astype(np.float64)).sum(1)
    assert (np.abs(S - 1) > 1e-6).any() == fp16
    masks = (np.arange(B) % 5 != 0).astype(np.uint8)
    nm = np.float32(masks.sum())
    q = torch.tensor(np.exp(olp.astype(np.float64)))
    # (the reference works from fp32 logits: autograd differentiates at the same fp32-rounded point)
    g = ur.kl_grad(z.astype(np.float32), olp, masks, nm, BETA)
    zt32 = torch.tensor(z.astype(np.float32).astype(np.float64), requires_grad=True)
    kl32 = (q * (torch.tensor(olp.astype(np.float64)) - torch.log_softmax(zt32, 1))).sum(1)
    ((float(np.float32(BETA)) * kl32 * torch.tensor(masks, dtype=torch.float64)).sum() / float(nm)).backward()
    np.testing.assert_allclose(g, zt32.grad.numpy(), atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(ur.exact_kl(z.astype(np.float32), olp)[0], kl32.detach().numpy(), atol=1e-6, rtol=1e-5)
    assert np.abs(g).max() > 1e-4 and (g[masks == 0] == 0).all()


@pytest.mark.parametrize("on", [False, True])
def test_trainer_keys_with_the_stub_library(stub_trainer, tmp_path, on):
    """the stub's metrics read as 0, so with kl_target the logged beta halves on every rollout"""
    cfg = _debug_cfg(tmp_path, "kl_coef: 0.2\nkl_target: 0.01\n" if on else "", rollouts=4)
    r = run_stub(stub_trainer, tmp_path, cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    data = _events(tmp_path)
    assert b"_hparams_/session_start_info" in data and b"cuda_graph" in data
    for tag in (b"kl_coef", b"kl_target", b"mean_kl"):
        assert (tag in data) == on, tag
    if on:
        np.testing.assert_array_equal(event_scalars(data, b"kl_coef"), np.float32(0.2) * np.float32([1, 0.5, 0.25, 0.125]))
        assert event_scalars(data, b"mean_kl") == [0.0] * 4


def test_trainer_beta_is_not_halved_below_its_floor(stub_trainer, tmp_path):
    """(stub: the KL reads as 0, so every rollout halves beta) halving stops at 1e-6, so that beta can grow again"""
    cfg = _debug_cfg(tmp_path, "kl_coef: 4e-6\nkl_target: 0.01\n", rollouts=5)
    r = run_stub(stub_trainer, tmp_path, cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    want, b = [], np.float32(4e-6)
    for _ in range(5):
        want.append(b)
        b = max(np.float32(0.5) * b, min(b, np.float32(1e-6)))
    assert want[-1] == np.float32(1e-6) and want[-2] == np.float32(1e-6)
    np.testing.assert_array_equal(event_scalars(_events(tmp_path), b"kl_coef"), want)


@pytest.mark.parametrize("extra,msg", [("kl_coef: -0.1\n", "non-negative"), ("kl_target: 0.01\n", "kl_coef > 0"),
                                       ("kl_coef: 0\nkl_target: 0.01\n", "kl_coef > 0"),
                                       ("kl_coef: 0.2\nkl_target: -1\n", "non-negative")])
def test_trainer_refuses_kl_keys_that_would_do_nothing(stub_trainer, tmp_path, extra, msg):
    cfg = _debug_cfg(tmp_path, extra)
    r = run_stub(stub_trainer, tmp_path, cfg)
    assert r.returncode != 0 and msg in r.stdout + r.stderr, (r.returncode, r.stderr[-2000:])


# ------------------------------------------------------------------ GPU
def _penalty(pkg, beta=BETA, on=True):
    """configure(eng) of the harness: the option on at `beta` (set after the context's other options)"""
    def configure(eng):
        if on:
            eng.set_option(pkg.OPT_KL_PENALTY, 1)
            eng.set_kl_coef(beta)
    return configure


def _penalised_engine(pkg, E, T, A, H, prec=None, **kw):
    eng = uh.make_engine(pkg, E, T, A, H, prec, **kw)
    _penalty(pkg)(eng)
    return eng


def _run(pkg, E, T, A, H, params, batch, epochs, M, beta=BETA, on=True, **kw):
    """uh.run_update at LR with the penalty (unless on is False); the KL planes are read where the option wrote them"""
    return uh.run_update(pkg, E, T, A, H, params, batch, epochs, M, LR, configure=_penalty(pkg, beta, on),
                         read=dict(kl=on), **kw)


def _check(out, ref, tol=1e-4):
    uh.check_against(out, ref, tol, PER_SAMPLE + ("kl",),
                     extra=[(out["mean_kl"], "mean_kl"), (out["diag"]["approx_kl"], "mean_approx_kl")])


def _fp32_case():
    E, T, A, H, epochs, M = 8, 32, 6, 64, 2, 4
    return E, T, A, H, epochs, M, hf.fill_params(6300, H, A), _hashed(6301, E * T, A)


@pytest.mark.gpu
def test_fp32_caller_batch_vs_composed_reference(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=BETA, lr=LR)
    out = _run(pkg, E, T, A, H, params, batch, epochs, M)
    _check(out, ref)
    # the penalty is what moved the update: the reference without it is far from the engine's result
    off = ur.composed_train(params, H, A, *batch, epochs, M, beta=0.0, lr=LR)
    assert not np.allclose(out["m"]["loss"], off["loss"], atol=1e-4, rtol=1e-4)
    assert not np.allclose(out["grads"], off["last_grads"], atol=1e-4)


@pytest.mark.gpu
def test_bf16_at_the_benched_shape_vs_emulated_reference(pkg):
    """BASELINE configs[1]'s update: 128 x 128 samples, A = 4, H = 512, 4 minibatches of 4096 (both fused kernels)"""
    E, T, A, H, epochs, M = 128, 128, 4, 512, 1, 4
    params = hf.fill_params(6400, H, A)
    batch = _hashed(6401, E * T, A, distinct=8)
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=BETA, lr=LR, emulate_bf16=True, floor=True)
    out = _run(pkg, E, T, A, H, params, batch, epochs, M, prec=pkg.BF16)
    c = bc.Checker()
    planes = {ours: out[ours] for ours, _ in bc.PLANES}
    c.train(H, A, out["m"], planes, None, ref, params0=params, params=out["params"])
    # the exact KL: per sample under the plane bound, the means under the loss bound, each at least four times the floor
    # run's own distance (as test_value_clip.py bounds approx-KL)
    fl = ref["floor_run"]

    def excess(a, w):
        return np.max(np.abs(np.asarray(a, np.float64) - w) - 1e-3 * np.abs(w))

    c.floor["exact_kl_excess"] = excess(fl["kl"], ref["kl"])
    c.floor["mean_exact_kl_excess"] = np.max(np.abs(fl["mean_kl"] - ref["mean_kl"]))
    c.check("exact_kl_excess", excess(out["kl"], ref["kl"]), 2e-3)
    c.check("mean_exact_kl_excess", np.max(np.abs(out["mean_kl"] - ref["mean_kl"])), 1e-3)
    print(c.summary("bf16 KL-penalised update vs emulated composed reference"))
    assert not c.failures, c.failures


@pytest.mark.gpu
@pytest.mark.parametrize("rollout_precision", ["fp32", "fp16"])
def test_rollout_batch(pkg, rollout_precision):
    """old log-probs as stored: with fp16 planes sum q != 1, and the gradient is the exact derivative with S"""
    from test_gpu_at_size import DeviceBytes, _flags
    E, T, A, H, epochs, M = 8, 16, 6, 64, 2, 2
    N = E * T
    rp = pkg.ROLLOUT_FP16 if rollout_precision == "fp16" else pkg.ROLLOUT_FP32
    params = hf.fill_params(6500, H, A)
    dev = DeviceBytes(hf.hf_bytes(6501, (T, E, 84, 84)))
    te, tr, st = _flags(6502, T, E)
    rew = hf.hf_range(6503, (T, E), -2, 2)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=3, rollout_precision=rp)
    eng.load_params(params)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
    eng.finish_rollout()
    dev.free()
    b = {k: eng.read_batch(k) for k in ("observations", "actions", "log_probs", "advantages", "returns", "masks")}
    eng.set_option(pkg.OPT_KL_PENALTY, 1)
    eng.set_kl_coef(0.5)
    # the policy after the first minibatch steps differs from the rollout's, so the KL grows from 0
    out = read_kl(eng, eng.train(2.5e-4, epochs, M), epochs, M)
    eng.close()
    olp = b["log_probs"].reshape(N, A)
    S = np.exp(olp.astype(np.float64)).sum(1)
    assert (np.abs(S - 1).max() > 1e-5) == (rollout_precision == "fp16")
    ref = ur.composed_train(params, H, A, b["observations"].reshape(N, 4, 84, 84), b["actions"].ravel(), olp,
                            b["advantages"].ravel(), b["returns"].ravel(), b["masks"].ravel(), epochs, M, beta=0.5,
                            lr=2.5e-4)
    assert ref["mean_kl"].max() > 0
    _check(out, ref)


@pytest.mark.gpu
def test_with_value_clipping_advantage_normalisation_and_shuffling(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    obs = batch[0]
    _, v0 = orc.net_forward(params, H, A, obs)
    vold = (v0 + hf.hf_range(6600, (E * T,), -0.3, 0.3)).astype(np.float32)
    opts = [(pkg.OPT_MINIBATCH_SHUFFLE, 1), (pkg.OPT_VALUE_CLIP, 1), (pkg.OPT_ADV_NORM_MINIBATCH, 1)]
    eng = _penalised_engine(pkg, E, T, A, H, options=opts)
    eng.load_params(params)
    eng.set_batch(*batch, values=vold)
    out = read_kl(eng, eng.train(LR, epochs, M), epochs, M)
    order = eng.sample_order(epochs)
    eng.close()
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=BETA, order=order, adv_norm=True, vold=vold, lr=LR)
    _check(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shuffle", [("fp32", 0), ("fp32", 1), ("bf16", 0), ("bf16", 1)])
def test_schedules_are_bit_identical(pkg, prec, shuffle):
    E, T, A, H, epochs, M = 16, 32, 4, 256, 2, 4
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(6700, H, A)
    batch = _hashed(6701, E * T, A)
    sh = [(pkg.OPT_MINIBATCH_SHUFFLE, shuffle)]
    run = lambda **kw: _run(pkg, E, T, A, H, params, batch, epochs, M, prec=p, **kw)  # noqa: E731
    # graph replay: eager (warm-up), capture + launch, replay == three eager calls
    assert_identical(run(options=sh + [(pkg.OPT_UPDATE_GRAPH, 1)], calls=3), run(options=sh, calls=3))
    # the 1-rank communicator (the record all-reduce carries the KL sums), like for like: the fused backward kernel is
    # off under data parallelism, so off on both sides
    nofuse = sh + [(pkg.OPT_FUSED_BWD, 0)]
    assert_identical(run(options=nofuse + [(pkg.OPT_FORCE_COMM, 1)], comm=True), run(options=nofuse))
    # one 4-epoch call == four 1-epoch calls
    outs = []
    for split in (False, True):
        eng = _penalised_engine(pkg, E, T, A, H, p, options=sh)
        eng.load_params(params)
        eng.set_batch(*batch)
        if split:
            o = uh.concat_updates([read_kl(eng, eng.train(LR, 1, M), 1, M) for _ in range(4)])
        else:
            o = read_kl(eng, eng.train(LR, 4, M), 4, M)
        outs.append(o)
        eng.close()
    assert_identical(outs[0], outs[1])


@pytest.mark.gpu
def test_beta_changed_between_graph_replays_matches_a_fresh_eager_context(pkg):
    """beta is a device value: a replayed graph follows it (as a baked kernel argument it would keep the capture's)"""
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    betas = (0.2, 0.2, 0.5, 0.0)  # eager warm-up, capture + launch at 0.2, then replays at 0.5 and at 0

    def drive(graph):
        eng = _penalised_engine(pkg, E, T, A, H, options=[(pkg.OPT_UPDATE_GRAPH, int(graph))])
        eng.load_params(params)
        eng.set_batch(*batch)
        outs = []
        for b in betas:
            eng.set_kl_coef(b)
            assert eng.kl_coef() == np.float32(b)
            outs.append(read_kl(eng, eng.train(LR, epochs, M), epochs, M))
        replays = eng.get_option(pkg.OPT_UPDATE_GRAPH)
        eng.close()
        return outs, replays

    graphed, n = drive(True)
    eager, n0 = drive(False)
    assert n == 3 and n0 == 0
    for g, e in zip(graphed, eager):
        assert_identical(g, e)
    # (and the betas did differ: the 0.5 call moved the parameters differently from a 0.2 one)
    assert not np.array_equal(graphed[2]["grads"], graphed[1]["grads"])


@pytest.mark.gpu
@pytest.mark.parametrize("A", [9, 18])
def test_wide_action_sets(pkg, A):
    """AMAX = 10 (the penalty's 4-wave workgroups, which add the rows' gradients in the 8-wave option-off order) and
    AMAX = 18: the reference at beta = 0.2, and beta = 0 bit-identical to the option off in fp32 and bf16"""
    E, T, H, epochs, M = 8, 64, 64, 2, 2  # (B = 256 rows: 16 per workgroup, every wave of a workgroup has rows)
    params = hf.fill_params(6900 + A, H, A)
    batch = _hashed(6901 + A, E * T, A)
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=BETA, lr=LR)
    _check(_run(pkg, E, T, A, H, params, batch, epochs, M), ref)
    for prec in (pkg.FP32, pkg.BF16):
        zero = _run(pkg, E, T, A, H, params, batch, epochs, M, prec=prec, beta=0.0)
        never = _run(pkg, E, T, A, H, params, batch, epochs, M, prec=prec, on=False)
        assert_identical(zero, never, skip=KL)
        assert (zero["kl"] > 0).all()
    # the same on the shuffled, value-clipped, minibatch-normalised schedule
    _, v0 = orc.net_forward(params, H, A, batch[0])
    vold = (v0 + hf.hf_range(6950 + A, (E * T,), -0.3, 0.3)).astype(np.float32)
    opts = [(pkg.OPT_MINIBATCH_SHUFFLE, 1), (pkg.OPT_VALUE_CLIP, 1), (pkg.OPT_ADV_NORM_MINIBATCH, 1)]
    zero = _run(pkg, E, T, A, H, params, batch, epochs, M, vold=vold, options=opts, beta=0.0)
    never = _run(pkg, E, T, A, H, params, batch, epochs, M, vold=vold, options=opts, on=False)
    assert_identical(zero, never, skip=KL)


@pytest.mark.gpu
def test_beta_zero_is_the_option_off_and_off_restores_the_default(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    never = _run(pkg, E, T, A, H, params, batch, epochs, M, on=False)
    zero = _run(pkg, E, T, A, H, params, batch, epochs, M, beta=0.0)
    assert_identical(zero, never, skip=KL)  # (everything but the KL planes, which only the option writes)
    assert (zero["kl"] > 0).all() and np.isfinite(zero["mean_kl"]).all()
    ref = ur.composed_train(params, H, A, *batch, epochs, M, beta=0.0, lr=LR)
    np.testing.assert_allclose(zero["kl"], ref["kl"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(zero["mean_kl"], ref["mean_kl"], atol=1e-4, rtol=1e-4)
    # after an update with beta = 0.5, the option off and the option on with beta = 0 continue bit for bit alike
    outs = []
    for off in (True, False):
        eng = uh.make_engine(pkg, E, T, A, H)
        assert eng.get_option(pkg.OPT_KL_PENALTY) == 0 and eng.get_option(pkg.OPT_KL_COEF) == 0
        assert eng.kl_coef() == 0
        eng.set_option(pkg.OPT_KL_PENALTY, 1)
        eng.set_kl_coef(0.5)
        assert eng.get_option(pkg.OPT_KL_PENALTY) == 1 and eng.get_option(pkg.OPT_KL_COEF) == 0x3F000000
        eng.load_params(params)
        eng.set_batch(*batch)
        eng.train(LR, 1, M)
        if off:
            eng.set_option(pkg.OPT_KL_PENALTY, 0)
        else:
            eng.set_kl_coef(0.0)
        outs.append(read_kl(eng, eng.train(LR, epochs, M), epochs, M, kl=not off))
        eng.close()
    assert_identical(outs[0], outs[1], skip=KL)


@pytest.mark.gpu
def test_error_cases(pkg):
    E, T, A, H = 4, 8, 4, 32
    N, M = E * T, 2
    batch = _hashed(6800, N, A)
    eng = uh.make_engine(pkg, E, T, A, H)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_option(pkg.OPT_KL_PENALTY, 2)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_option(pkg.OPT_KL_PENALTY, -1)
    assert eng.get_option(pkg.OPT_KL_PENALTY) == 0
    eng.set_kl_coef(0.25)
    for bad in (-0.0, -1.0, float("inf"), float("nan"), -float("inf")):
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.set_kl_coef(bad)
    for bad in (0x7F800000, 0x7FC00000, -1, -(2 ** 31)):  # (+Inf, a NaN, and two patterns with the sign bit)
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.set_option(pkg.OPT_KL_COEF, bad)
    assert eng.kl_coef() == 0.25
    eng.set_option(pkg.OPT_KL_COEF, 0x7F7FFFFF)  # (the largest finite float is valid)
    eng.set_option(pkg.OPT_KL_COEF, 1)  # (so is the smallest subnormal)
    eng.set_kl_coef(0.25)
    eng.load_params(hf.fill_params(6801, H, A))
    eng.set_batch(*batch)
    eng.train(LR, 1, M)  # (option off)
    for name in ("kl",):
        with pytest.raises(pkg.AleppoError, match="ALEPPO_OPT_KL_PENALTY"):
            eng.read_train_metric(name, 1, M, N // M)
    with pytest.raises(pkg.AleppoError, match="ALEPPO_OPT_KL_PENALTY"):
        eng.kl_divergence(1, M)
    eng.set_option(pkg.OPT_KL_PENALTY, 1)
    eng.train(LR, 1, M)
    assert eng.kl_divergence(1, M).shape == (1, M)
    with pytest.raises(pkg.AleppoInvalidArgument):  # (count = epochs * M of the last train)
        eng.kl_divergence(2, M)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.read_train_metric("kl", 2, M, N // M)
    eng.set_option(pkg.OPT_KL_PENALTY, 0)
    eng.train(LR, 1, M)
    with pytest.raises(pkg.AleppoError, match="ALEPPO_OPT_KL_PENALTY"):
        eng.kl_divergence(1, M)
    eng.close()


@pytest.mark.gpu
def test_trainer_on_the_device(trainer, tmp_path):
    cfg = _debug_cfg(tmp_path, "kl_coef: 0.2\nkl_target: 0.01\nshuffle_minibatches: true\n", rollouts=5)
    os.makedirs(tmp_path / "tb")
    r = subprocess.run([trainer, "breakout.bin", str(tmp_path / "tb" / "run.log"), str(tmp_path), "g", str(cfg)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = _events(tmp_path / "tb")
    assert b"kl_target" in blob
    beta, d = event_scalars(blob, b"kl_coef"), event_scalars(blob, b"mean_kl")
    assert len(beta) == len(d) == 5 and np.isfinite(beta + d).all() and min(d) >= 0
    assert all(np.isfinite(event_scalars(blob, b"mean_loss")))
    assert beta[0] == np.float32(0.2)
    for i in range(4):  # the PPO paper's rule, from the logged mean KL of the last epoch
        want = beta[i] * (0.5 if d[i] < 0.01 / 1.5 else 2.0 if d[i] > 1.5 * 0.01 else 1.0)
        assert beta[i + 1] == np.float32(want), (i, beta, d)
