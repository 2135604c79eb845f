"""ALEPPO_OPT_ADV_NORM_MINIBATCH: per-minibatch advantage normalisation in aleppo_train (CleanRL norm_adv).

CPU: the header constants against the Python mirror, the host normaliser of update_ref.py against torch and its edge
cases, and the trainer's `minibatch_advantage_norm` key against the host-only library stand-in.
GPU (-m gpu, everything through the C ABI): the normalised update against the composed reference (update_ref.py) in
fp32 - contiguous and shuffled, on caller and rollout batches, with advantage_norm and with value clipping - and in bf16
at BASELINE configs[1]'s update; that it is per-minibatch and not whole-batch; graph-replayed, 1-rank communicator and
one-epoch-call schedules bit-identical to the eager one; the option off restores the default bit for bit; the errors;
the trainer on the device."""
import functools
import os
import re
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
from update_harness import assert_identical
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 2.5e-4
PER_SAMPLE = uh.PER_SAMPLE[:5]  # (these tests leave the approx-KL / clip-fraction diagnostics to test_value_clip.py)
composed_train = functools.partial(ur.composed_train, adv_norm=True)
read_stats = functools.partial(uh.read_update, diag=False, adv_stats=True)


# ------------------------------------------------------------------ CPU
def test_header_constants_and_python_mirror():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()

    assert const("ALEPPO_OPT_ADV_NORM_MINIBATCH") == pkg.OPT_ADV_NORM_MINIBATCH == 14
    assert const("ALEPPO_M_ADV_MEAN") == pkg.METRIC_ADV_FIELDS["mean"] == 9
    assert const("ALEPPO_M_ADV_STD") == pkg.METRIC_ADV_FIELDS["std"] == 10
    assert re.search(r"#define ALEPPO_ABI_VERSION 2\b", hdr)
    assert callable(pkg.Engine.advantage_stats)


def test_host_normaliser_is_torch_on_the_unmasked_samples():
    torch = pytest.importorskip("torch")
    for seed, n, off, scale in ((5000, 64, 0.0, 1.0), (5001, 257, 3.0, 0.1), (5002, 1000, -2.5, 2.0)):
        adv = (off + scale * hf.hf_range(seed, (n,), -1, 1)).astype(np.float32)
        masks = (hf.hf_unit(seed + 1, n) >= np.float32(0.25)).astype(np.uint8)
        t = torch.from_numpy(adv.astype(np.float64))[torch.from_numpy(masks != 0)]
        mean, std = t.mean().item(), t.std().item()  # (unbiased, like aleppo.h)
        want = (adv.astype(np.float64) - mean) / (std + 1e-8)
        got = ur.normalise64(adv, masks)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        _, m64, s64, mf, inv = ur.stats(adv, masks)
        assert abs(m64 - mean) <= 1e-12 and abs(s64 - std) <= 1e-12 * std
        assert mf == np.float32(mean) and inv == np.float32(1.0 / (std + 1e-8))
        # the fp32 form the device applies is within fp32 rounding of the float64 one
        f32, _, _ = ur.normalise(adv, masks, 1)
        np.testing.assert_allclose(f32, want, rtol=1e-5, atol=1e-5)


def test_host_normaliser_edge_cases():
    adv = hf.hf_range(5100, (8,), -1, 1)
    # n = 0: mean 0, inv 1 - the advantages pass through unchanged
    n, mean, std, mf, inv = ur.stats(adv, np.zeros(8, np.uint8))
    assert (n, mean, std, mf, inv) == (0, 0.0, 0.0, np.float32(0), np.float32(1))
    out, _, _ = ur.normalise(adv, np.zeros(8, np.uint8), 1)
    np.testing.assert_array_equal(out, adv)
    # n = 1: var = 0 (the max(n - 1, 1) denominator), std = 0, and the one unmasked sample becomes exactly 0
    mk = np.zeros(8, np.uint8)
    mk[3] = 1
    n, mean, std, mf, inv = ur.stats(adv, mk)
    assert n == 1 and mean == float(adv[3]) and std == 0.0 and inv == np.float32(1e8)
    out, _, _ = ur.normalise(adv, mk, 1)
    assert out[3] == 0.0
    # constant advantages: a^ = 0 on every unmasked sample
    c = np.full(16, np.float32(0.37))
    mk = (np.arange(16) % 3 != 0).astype(np.uint8)
    out, _, std = ur.normalise(c, mk, 1)
    assert (out[mk != 0] == 0).all() and std[0] < 1e-12


def test_normalise_is_per_contiguous_slice():
    N, M = 48, 3
    adv = hf.hf_range(5200, (N,), -1, 1) + np.repeat(np.float32([0, 5, -3]), N // M)
    masks = (hf.hf_unit(5201, N) >= np.float32(0.2)).astype(np.uint8)
    out, mean, std = ur.normalise(adv, masks, M)
    B = N // M
    for k in range(M):
        s = slice(k * B, (k + 1) * B)
        sel = out[s][masks[s] != 0].astype(np.float64)
        assert abs(sel.mean()) < 1e-6 and abs(sel.std(ddof=1) - 1) < 1e-5
        assert abs(mean[k] - adv[s][masks[s] != 0].astype(np.float64).mean()) < 1e-12


@pytest.mark.parametrize("on", [False, True])
def test_trainer_key_reaches_the_hparams_record(stub_trainer, tmp_path, on):
    cfg = _debug_cfg(tmp_path, "minibatch_advantage_norm: true\n" if on else "")
    r = run_stub(stub_trainer, tmp_path, cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    data = _events(tmp_path)
    assert b"_hparams_/session_start_info" in data and b"cuda_graph" in data
    assert (b"minibatch_advantage_norm" in data) == on
    assert (b"mean_advantage_std" in data) == on


# ------------------------------------------------------------------ GPU
def _batch(seed, N, A, M, distinct=None, edge=True):
    """uh.hashed_batch with advantages and masks of its own: the minibatch slices have distinct advantage offsets and
    scales, masked samples in every slice (the first sample too), and (edge, M >= 4) slice 2 all masked and slice 3 with
    a single unmasked sample"""
    obs, actions, old_lp, _, ret, masks = uh.hashed_batch(seed, N, A, mask_p=0.15, distinct=distinct)
    B = N // M
    k = np.arange(N) // B
    off = np.float32([0.5, -2.0, 3.0, 1.0, -0.7, 0.2, 4.0, -1.5])[k % 8]
    scale = np.float32([1.0, 0.1, 2.5, 0.5, 1.5, 0.3, 0.05, 3.0])[k % 8]
    adv = (off + scale * hf.hf_range(seed + 3, (N,), -1, 1)).astype(np.float32)
    masks[::7] = 0  # (masked samples in every slice)
    if edge and M >= 4:
        masks[k == 2] = 0
        masks[k == 3] = 0
        masks[3 * B + 5] = 1
    return obs, actions, old_lp, adv, ret, masks


def _run(pkg, E, T, A, H, params, batch, epochs, M, on=True, options=(), **kw):
    """uh.run_update at LR, with the option set (after `options`) unless on is False"""
    norm = [(pkg.OPT_ADV_NORM_MINIBATCH, 1)] if on else []
    return uh.run_update(pkg, E, T, A, H, params, batch, epochs, M, LR, options=list(options) + norm,
                         read=dict(diag=False, adv_stats=on), **kw)


def _check(out, ref, tol=1e-4):
    """engine outputs vs the composed reference at the fp32 bounds (losses, pre-clip norms, planes, parameters) and the
    read-back statistics vs the float64 ones at 1e-6 relative"""
    uh.check_against(out, ref, tol, PER_SAMPLE)
    np.testing.assert_allclose(out["adv_mean"], ref["adv_mean"], rtol=1e-6, atol=1e-30)
    np.testing.assert_allclose(out["adv_std"], ref["adv_std"], rtol=1e-6, atol=1e-30)


def _fp32_case():
    E, T, A, H, epochs, M = 8, 32, 6, 64, 2, 4
    params = hf.fill_params(5300, H, A)
    return E, T, A, H, epochs, M, params, _batch(5301, E * T, A, M)


@pytest.mark.gpu
def test_fp32_contiguous_caller_batch_vs_composed_reference(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    ref = composed_train(params, H, A, *batch, epochs, M, lr=LR)
    assert ref["adv_std"][0, 2] == 0 and ref["adv_std"][0, 3] == 0  # (the all-masked and the one-sample minibatch)
    out = _run(pkg, E, T, A, H, params, batch, epochs, M)
    assert np.isnan(out["m"]["loss"][:, 2]).all()  # (no unmasked sample: 0 / 0, like the reference's masked mean)
    _check(out, ref)
    assert out["adv_mean"][0, 2] == 0 and out["adv_std"][0, 2] == 0
    np.testing.assert_array_equal(out["adv_mean"][0], out["adv_mean"][1])  # (contiguous: every epoch the same)


@pytest.mark.gpu
def test_it_is_per_minibatch_not_whole_batch(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    obs, actions, old_lp, adv, ret, masks = batch
    out = _run(pkg, E, T, A, H, params, batch, epochs, M)
    for other in (orc.adv_norm(adv, masks), adv):
        r = orc.train(params, H, A, obs, actions, old_lp, other, ret, masks, epochs, M, lr=LR)
        fin = np.isfinite(r["loss"])
        assert not np.allclose(out["m"]["loss"][fin], r["loss"][fin], atol=1e-4, rtol=1e-4)
        assert not np.allclose(out["clipped_losses"], r["clipped"], atol=1e-4, rtol=1e-4)
        assert not np.allclose(out["grads"], r["last_grads"], atol=1e-4)


@pytest.mark.gpu
def test_fp32_shuffled_vs_per_epoch_composed_reference(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    masks = batch[5].copy()
    masks[::3] = 0  # (shuffled minibatches mix the slices: keep a third masked everywhere)
    batch = batch[:5] + (masks,)
    eng = uh.make_engine(pkg, E, T, A, H, options=[(pkg.OPT_MINIBATCH_SHUFFLE, 1), (pkg.OPT_ADV_NORM_MINIBATCH, 1)])
    eng.load_params(params)
    eng.set_batch(*batch)
    outs, orders = [], []
    for _ in range(2):  # (the orders are keyed by the Adam step: the second call's differ)
        outs.append(read_stats(eng, eng.train(LR, epochs, M), epochs, M))
        orders.append(eng.sample_order(epochs))
    eng.close()
    assert (orders[0] != orders[1]).any() and (orders[0][0] != orders[0][1]).any()
    ref = composed_train(params, H, A, *batch, 2 * epochs, M, order=np.concatenate(orders), lr=LR)
    assert np.ptp(ref["adv_mean"], axis=0).max() > 0  # (each epoch's minibatches see their own statistics)
    for c, out in enumerate(outs):
        sl = slice(c * epochs, (c + 1) * epochs)
        part = {k: (v[sl] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in ref.items()}
        if c == 0:  # (the parameters / gradients after the first call: the reference's after its first two epochs)
            r1 = composed_train(params, H, A, *batch, epochs, M, order=orders[0], lr=LR)
            part.update(params=r1["params"], last_grads=r1["last_grads"])
        _check(out, part)


@pytest.mark.gpu
def test_bf16_at_the_benched_shape_vs_emulated_reference(pkg):
    """BASELINE configs[1]'s update: 128 x 128 samples, A = 4, H = 512, 4 minibatches of 4096 (both fused kernels)"""
    E, T, A, H, epochs, M = 128, 128, 4, 512, 1, 4
    params = hf.fill_params(5400, H, A)
    batch = _batch(5401, E * T, A, M, distinct=8, edge=False)
    ref = composed_train(params, H, A, *batch, epochs, M, lr=LR, emulate_bf16=True, floor=True)
    out = _run(pkg, E, T, A, H, params, batch, epochs, M, prec=pkg.BF16)
    c = bc.Checker()
    planes = {ours: out[ours] for ours, _ in bc.PLANES}
    c.train(H, A, out["m"], planes, None, ref, params0=params, params=out["params"])
    print(c.summary("bf16 minibatch-normalised update vs emulated composed reference"))
    assert not c.failures, c.failures
    np.testing.assert_allclose(out["adv_mean"], ref["adv_mean"], rtol=1e-6)
    np.testing.assert_allclose(out["adv_std"], ref["adv_std"], rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("rollout_precision,whole_batch", [("fp32", 0), ("fp16", 0), ("fp32", 1)])
def test_rollout_batch(pkg, rollout_precision, whole_batch):
    from test_gpu_at_size import DeviceBytes, _flags
    E, T, A, H, epochs, M = 8, 16, 4, 64, 2, 2
    N = E * T
    rp = pkg.ROLLOUT_FP16 if rollout_precision == "fp16" else pkg.ROLLOUT_FP32
    params = hf.fill_params(5500, H, A)
    dev = DeviceBytes(hf.hf_bytes(5501, (T, E, 84, 84)))
    te, tr, st = _flags(5502, T, E)
    rew = hf.hf_range(5503, (T, E), -2, 2) + np.float32(1.5)  # (an offset, so that the advantages have a mean)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=3, rollout_precision=rp, advantage_norm=whole_batch)
    eng.load_params(params)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
    eng.finish_rollout()
    dev.free()
    b = {k: eng.read_batch(k) for k in ("observations", "actions", "log_probs", "advantages", "returns", "masks")}
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 1)
    out = read_stats(eng, eng.train(LR, epochs, M), epochs, M)
    eng.close()
    # the statistics see the advantages as stored (fp16-rounded with fp16 planes; after the whole-batch normalisation)
    adv = b["advantages"].ravel()
    ref = composed_train(params, H, A, b["observations"].reshape(N, 4, 84, 84), b["actions"].ravel(),
                            b["log_probs"].reshape(N, A), adv, b["returns"].ravel(), b["masks"].ravel(), epochs, M,
                            lr=LR)
    if whole_batch:
        whole = adv[b["masks"].ravel() != 0].astype(np.float64)
        assert abs(whole.mean()) < 1e-5 and abs(whole.std(ddof=1) - 1) < 1e-4
    assert np.abs(ref["adv_mean"]).max() > 1e-3 and np.abs(ref["adv_std"] - 1).max() > 1e-3
    _check(out, ref)


@pytest.mark.gpu
def test_with_value_clipping_vs_composed_reference(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    obs = batch[0]
    _, v0 = orc.net_forward(params, H, A, obs)
    vold = (v0 + hf.hf_range(5600, (E * T,), -0.3, 0.3)).astype(np.float32)
    ref = composed_train(params, H, A, *batch, epochs, M, vold=vold, lr=LR)
    assert ref["zero_branch"].sum() > 0  # (the clipped value branch is taken)
    out = _run(pkg, E, T, A, H, params, batch, epochs, M, vold=vold, options=[(pkg.OPT_VALUE_CLIP, 1)])
    _check(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shuffle", [("fp32", 0), ("fp32", 1), ("bf16", 0), ("bf16", 1)])
def test_schedules_are_bit_identical(pkg, prec, shuffle):
    E, T, A, H, epochs, M = 16, 32, 4, 256, 2, 4
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(5700, H, A)
    batch = _batch(5701, E * T, A, M, edge=False)
    sh = [(pkg.OPT_MINIBATCH_SHUFFLE, shuffle)]
    run = lambda **kw: _run(pkg, E, T, A, H, params, batch, epochs, M, prec=p, **kw)  # noqa: E731
    # graph replay: eager (warm-up), capture + launch, replay == three eager calls
    assert_identical(run(options=sh + [(pkg.OPT_UPDATE_GRAPH, 1)], calls=3), run(options=sh, calls=3))
    # the 1-rank communicator (the data-parallel schedule: the statistics' sums all-reduced, then finalised), like for
    # like: the fused backward kernel is off under data parallelism, so off on both sides
    nofuse = sh + [(pkg.OPT_FUSED_BWD, 0)]
    assert_identical(run(options=nofuse + [(pkg.OPT_FORCE_COMM, 1)], comm=True), run(options=nofuse))
    # one 4-epoch call == four 1-epoch calls
    outs = []
    for split in (False, True):
        eng = uh.make_engine(pkg, E, T, A, H, p, options=sh + [(pkg.OPT_ADV_NORM_MINIBATCH, 1)])
        eng.load_params(params)
        eng.set_batch(*batch)
        if split:
            o = uh.concat_updates([read_stats(eng, eng.train(LR, 1, M), 1, M) for _ in range(4)])
        else:
            o = read_stats(eng, eng.train(LR, 4, M), 4, M)
        outs.append(o)
        eng.close()
    assert_identical(outs[0], outs[1])


@pytest.mark.gpu
def test_option_off_restores_the_default(pkg):
    E, T, A, H, epochs, M, params, batch = _fp32_case()
    never = _run(pkg, E, T, A, H, params, batch, epochs, M, on=False)
    eng = uh.make_engine(pkg, E, T, A, H)
    assert eng.get_option(pkg.OPT_ADV_NORM_MINIBATCH) == 0
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 1)
    assert eng.get_option(pkg.OPT_ADV_NORM_MINIBATCH) == 1
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 2)
    assert eng.get_option(pkg.OPT_ADV_NORM_MINIBATCH) == 1
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 0)
    eng.load_params(params)
    eng.set_batch(*batch)
    toggled = read_stats(eng, eng.train(LR, epochs, M), epochs, M, adv_stats=False)
    with pytest.raises(pkg.AleppoError, match="ALEPPO_OPT_ADV_NORM_MINIBATCH"):
        eng.advantage_stats(epochs, M)
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 1)
    eng.train(LR, 1, M)
    assert eng.advantage_stats(1, M)[0].shape == (1, M)
    with pytest.raises(pkg.AleppoInvalidArgument):  # (count = epochs * M of the last train)
        eng.advantage_stats(2, M)
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, 0)
    eng.train(LR, 1, M)
    with pytest.raises(pkg.AleppoError, match="ALEPPO_OPT_ADV_NORM_MINIBATCH"):
        eng.advantage_stats(1, M)
    eng.close()
    assert_identical(toggled, never)
    # and the default is orc.train on the advantages as given
    ref = orc.train(params, H, A, *batch, epochs, M, lr=LR)
    np.testing.assert_allclose(never["params"], ref["params"], atol=1e-4)


@pytest.mark.gpu
def test_trainer_on_the_device(trainer, tmp_path):
    cfg = _debug_cfg(tmp_path, "minibatch_advantage_norm: true\nshuffle_minibatches: true\nclip_value_loss: true\n",
                     rollouts=3)
    os.makedirs(tmp_path / "tb")
    r = subprocess.run([trainer, "breakout.bin", str(tmp_path / "tb" / "run.log"), str(tmp_path), "g", str(cfg)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = _events(tmp_path / "tb")
    assert b"minibatch_advantage_norm" in blob
    vals = event_scalars(blob, "mean_advantage_std")
    assert len(vals) == 3 and all(np.isfinite(vals)) and min(vals) >= 0
