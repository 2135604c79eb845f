"""ALEPPO_OPT_VALUE_CLIP (value-function clipping) and the approx-KL / clip-fraction diagnostics of aleppo_train.

CPU: the header constants against the Python mirror, the composed reference (update_ref.py) against orc.train with
every option off, and the trainer's `clip_value_loss` / `target_kl` keys against the host-only library stand-in.
GPU (-m gpu, everything through the C ABI): the clipped update against the composed reference in fp32 and in bf16 (at
BASELINE configs[1]'s update), on a rollout batch with fp32 and fp16 planes; shuffled, graph-replayed and 1-rank
communicator schedules bit-identical to the plain one; the option off restores the default bit for bit; the error
cases; one call of E epochs equals E one-epoch calls; the trainer's target_kl on the device."""
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
from update_harness import PER_SAMPLE, assert_identical
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0.1  # Engine's default clip_param
# learning rate of the GPU tests: small enough that the values stay near where v_old was drawn over the 8 Adam steps of
# a 2 x 4 update (at 2.5e-4 they drift by ~0.8, far past the clip range, and the clipped branch stops winning)
LR = 2e-5


# ------------------------------------------------------------------ CPU
def test_header_constants_and_export():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    assert const("ALEPPO_OPT_VALUE_CLIP") == pkg.OPT_VALUE_CLIP == 13
    assert const("ALEPPO_M_APPROX_KL") == pkg.METRIC_FIELDS["approx_kl"] == 5
    assert const("ALEPPO_M_CLIP_FRACTION") == pkg.METRIC_FIELDS["clip_fraction"] == 6
    assert const("ALEPPO_M_MEAN_APPROX_KL") == pkg.METRIC_MEAN_FIELDS["approx_kl"] == 7
    assert const("ALEPPO_M_MEAN_CLIP_FRACTION") == pkg.METRIC_MEAN_FIELDS["clip_fraction"] == 8
    assert "aleppo_set_batch_values" in pkg.EXPORTS
    assert re.search(r"int aleppo_set_batch_values\(aleppo_ctx \*ctx, const float \*values, int64_t n\);", hdr)
    assert hasattr(pkg.lib(), "aleppo_set_batch_values")


def _planes(seed, N, A, distinct=None):
    """(obs, actions, old_lp, adv, masks): the returns come from _values_and_returns"""
    return uh.hashed_batch(seed, N, A, mask_p=0.1, with_ret=False, distinct=distinct)


def _values_and_returns(seed, values):
    """v_old around the current values (spread 3 x clip on each side) and returns around them, so that a real share of
    the samples takes the clipped value branch"""
    n = values.shape[0]
    vold = (values + hf.hf_range(seed, (n,), -3 * CLIP, 3 * CLIP)).astype(np.float32)
    ret = (values + hf.hf_range(seed + 1, (n,), -2 * CLIP, 2 * CLIP)).astype(np.float32)
    return vold, ret


@pytest.mark.parametrize("bf16", [False, True])
def test_composed_reference_without_clipping_is_the_oracle(bf16):
    """update_ref.composed_train with every option off is orc.train, bit for bit (same oracle calls in the same order)"""
    H, A, N, epochs, M = 32, 6, 48, 2, 3
    params = hf.fill_params(4100, H, A)
    obs, actions, old_lp, adv, masks = _planes(4101, N, A)
    ret = hf.hf_range(4106, (N,), -1, 1)
    ref = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, emulate_bf16=bf16)
    got = ur.composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, emulate_bf16=bf16)
    for k in ("params", "loss", "grad_norm", "last_grads", "total_losses", "ratio", "entropies", "value_losses",
              "clipped"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("m", "v"):
        np.testing.assert_array_equal(got["adam"][k], ref["adam"][k])
    assert got["adam"]["step"] == ref["adam"]["step"] == epochs * M
    assert (got["params"] != params).any()
    # and the value branch reduces to the reference's where v_old = v (|d| = 0 <= c: the select keeps v)
    _, values = orc.net_forward(params, H, A, obs[:N // M])
    lv, dv, zero = ur.value_branch(values, ret[:N // M], values, CLIP)
    np.testing.assert_array_equal(lv, 0.5 * (values.astype(np.float64) - ret[:N // M]) ** 2)
    assert not zero.any()


def test_trainer_keys_with_the_stub_library(stub_trainer, tmp_path):
    cfg = _debug_cfg(tmp_path, "clip_value_loss: true\ntarget_kl: 0.01\n")
    r = run_stub(stub_trainer, tmp_path, cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    data = _events(tmp_path)
    assert b"_hparams_/session_start_info" in data and b"clip_value_loss" in data
    for tag in ("mean_approx_kl", "mean_clip_fraction", "update_epochs"):
        assert len(event_scalars(data, tag)) == 2, tag
    assert event_scalars(data, "update_epochs") == [2.0, 2.0]  # (the stand-in reports zero approx-KL: every epoch runs)


# ------------------------------------------------------------------ GPU
def _run(pkg, E, T, A, H, prec, params, batch, ret, vold, epochs, M, clip_on=True, options=(), **kw):
    """uh.run_update at LR, with the option set (after `options`) unless clip_on is False"""
    clip = [(pkg.OPT_VALUE_CLIP, 1)] if clip_on else []
    return uh.run_update(pkg, E, T, A, H, params, batch[:4] + (ret, batch[4]), epochs, M, LR, vold=vold, prec=prec,
                         options=list(options) + clip, **kw)


def _check_fp32(out, ref, masks_ep, clip=CLIP, tol=1e-4, params0=None):
    """engine outputs vs the composed reference at the fp32 bounds"""
    uh.check_against(out, ref, tol, [k for k in PER_SAMPLE if k != "clip_fraction"],
                     extra=[(out["diag"]["approx_kl"], "mean_approx_kl")])
    # clip fraction: exact except where |rho - 1| is within 1e-6 of the clip
    near = np.abs(np.abs(ref["ratio"].astype(np.float64) - 1) - clip) <= 1e-6
    assert ((out["clip_fraction"] != ref["clip_fraction"]) & ~near).sum() == 0
    assert set(np.unique(out["clip_fraction"])) <= {0.0, 1.0}
    np.testing.assert_allclose(out["diag"]["clip_fraction"], ref["mean_clip_fraction"], atol=tol)
    # the means are the masked means of the planes the engine returned
    for k in ("approx_kl", "clip_fraction"):
        mine = (out[k].astype(np.float64) * masks_ep).sum(-1) / masks_ep.sum(-1)
        np.testing.assert_allclose(out["diag"][k], mine, rtol=1e-5, atol=1e-7)
    if params0 is not None:  # (the update itself, relative: at LR the parameters move by ~1e-4)
        du, dr = out["params"].astype(np.float64) - params0, ref["params"].astype(np.float64) - params0
        assert np.linalg.norm(du - dr) <= 1e-3 * np.linalg.norm(dr) and np.linalg.norm(dr) > 0


def _fp32_case(pkg):
    E, T, A, H, epochs, M = 8, 32, 6, 64, 2, 4
    N = E * T
    params = hf.fill_params(4200, H, A)
    obs, actions, old_lp, adv, masks = _planes(4201, N, A)
    _, v0 = orc.net_forward(params, H, A, obs)
    vold, ret = _values_and_returns(4210, v0)
    return E, T, A, H, epochs, M, params, (obs, actions, old_lp, adv, masks), ret, vold


@pytest.mark.gpu
def test_fp32_clipped_update_vs_composed_reference(pkg):
    E, T, A, H, epochs, M, params, batch, ret, vold = _fp32_case(pkg)
    obs, actions, old_lp, adv, masks = batch
    B = E * T // M
    ref = ur.composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold=vold, lr=LR)
    share = ref["zero_branch"].sum() / (epochs * masks.sum())
    assert 0.2 <= share <= 0.8, share  # the test has teeth: the clipped branch wins for a real share of the samples
    out = _run(pkg, E, T, A, H, pkg.FP32, params, batch, ret, vold, epochs, M)
    masks_ep = np.broadcast_to(masks.reshape(M, B), (epochs, M, B)).astype(np.float64)
    _check_fp32(out, ref, masks_ep, params0=params)
    assert out["clip_fraction"].sum() > 0 and (out["approx_kl"] >= -1e-6).all()
    # on the first minibatch (same parameters on both sides) the clipped value loss is never below the unclipped one,
    # and differs from it where the clipped branch won
    unclipped = ur.composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, M, lr=LR)
    # (up to one ulp: the reference's clipped branch is float64, the oracle's unclipped one fp32)
    assert (ref["value_losses"][0, 0] >= unclipped["value_losses"][0, 0] * (1 - 1e-6)).all()
    assert np.abs(out["value_losses"][0, 0] - unclipped["value_losses"][0, 0]).max() > 1e-3


@pytest.mark.gpu
def test_bf16_clipped_update_at_the_benched_shape_vs_emulated_reference(pkg):
    """BASELINE configs[1]'s update: 128 x 128 samples, A = 4, H = 512, minibatches of 4096 (both fused kernels)"""
    E, T, A, H, epochs, M = 128, 128, 4, 512, 1, 4
    N = E * T
    params = hf.fill_params(4300, H, A)
    obs, actions, old_lp, adv, masks = _planes(4301, N, A, distinct=8)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
    eng.load_params(params)
    _, v0 = eng.forward(obs)  # (where the values are: the inputs only need to straddle them)
    eng.close()
    vold, ret = _values_and_returns(4310, v0)
    ref = ur.composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, vold=vold, lr=LR,
                            emulate_bf16=True, floor=True)
    assert 0.2 <= ref["zero_branch"].sum() / (epochs * masks.sum()) <= 0.8
    out = _run(pkg, E, T, A, H, pkg.BF16, params, (obs, actions, old_lp, adv, masks), ret, vold, epochs, M)
    c = bc.Checker()
    planes = {ours: out[ours] for ours, _ in bc.PLANES}
    c.train(H, A, out["m"], planes, None, ref, params0=params, params=out["params"])
    # the diagnostics: per-sample approx-KL under the plane bound, the means under the loss bound, each at least four
    # times the floor run's own distance (approx-KL amplifies a logit's bf16 noise by rho - 1, up to ~6 here: the
    # batch's old log-probabilities are not the network's)
    fl = ref["floor_run"]

    def kl_excess(a, w):
        return np.max(np.abs(np.asarray(a, np.float64) - w) - 1e-3 * np.abs(w))

    c.floor["approx_kl_excess"] = kl_excess(fl["approx_kl"], ref["approx_kl"])
    c.floor["mean_kl_excess"] = np.max(np.abs(fl["mean_approx_kl"] - ref["mean_approx_kl"]))
    c.check("approx_kl_excess", kl_excess(out["approx_kl"], ref["approx_kl"]), 2e-3)
    c.check("mean_kl_excess", np.max(np.abs(out["diag"]["approx_kl"] - ref["mean_approx_kl"])), 1e-3)
    flips = (out["clip_fraction"] != ref["clip_fraction"]).mean()
    c.check("clip_fraction_flips", flips, 0.01)  # (a ratio within bf16 noise of the clip may land either side)
    print(c.summary("bf16 value-clipped update vs emulated composed reference"))
    assert not c.failures, c.failures


@pytest.mark.gpu
@pytest.mark.parametrize("rollout_precision", ["fp32", "fp16"])
def test_rollout_batch_takes_v_old_from_the_values_plane(pkg, rollout_precision):
    from test_gpu_at_size import DeviceBytes, _flags
    E, T, A, H, epochs, M = 8, 16, 4, 64, 2, 2
    N = E * T
    clip = 0.002  # (small: a v_old taken from another sample, or another layout, lands outside the clip range)
    rp = pkg.ROLLOUT_FP16 if rollout_precision == "fp16" else pkg.ROLLOUT_FP32
    params = hf.fill_params(4400, H, A)
    dev = DeviceBytes(hf.hf_bytes(4401, (T, E, 84, 84)))
    te, tr, st = _flags(4402, T, E)
    rew = hf.hf_range(4403, (T, E), -2, 2)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=3, rollout_precision=rp, clip_param=clip)
    eng.load_params(params)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
    eng.finish_rollout()
    dev.free()
    b = {k: eng.read_batch(k) for k in ("observations", "actions", "log_probs", "advantages", "returns", "masks",
                                         "values")}
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    m = eng.train(LR, epochs, M)
    out = uh.read_update(eng, m, epochs, M)
    eng.close()
    obs = b["observations"].reshape(N, 4, 84, 84)
    vold = b["values"].ravel()  # env-major [E, T], fp16-rounded with fp16 planes
    ref = ur.composed_train(params, H, A, obs, b["actions"].ravel(), b["log_probs"].reshape(N, A),
                            b["advantages"].ravel(), b["returns"].ravel(), b["masks"].ravel(), epochs, M, vold=vold,
                            lr=LR, clip=clip)
    # (the values were stored by this network, so the first minibatch sees v_old = v up to the fp16 rounding; the
    # later ones see values that the Adam steps moved)
    print("zero-gradient branch per minibatch:", ref["zero_branch"].tolist())
    masks_ep = np.broadcast_to(b["masks"].reshape(M, N // M), (epochs, M, N // M)).astype(np.float64)
    _check_fp32(out, ref, masks_ep, clip=clip, params0=params)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fp32", "bf16"])
def test_schedules_are_bit_identical_with_clipping(pkg, case):
    if case == "fp32":
        E, T, A, H, epochs, M, params, batch, ret, vold = _fp32_case(pkg)
        prec, distinct = pkg.FP32, None
    else:
        E, T, A, H, epochs, M, prec = 32, 64, 4, 512, 2, 1, pkg.BF16  # (minibatches of 2048: fused backward on)
        params = hf.fill_params(4500, H, A)
        batch = _planes(4501, E * T, A, distinct=8)
        vold, ret = _values_and_returns(4510, np.zeros(E * T, np.float32))
    N = E * T
    run = lambda **kw: _run(pkg, E, T, A, H, prec, params, batch, ret, vold, epochs, M, **kw)  # noqa: E731
    base = run()
    # the 1-rank communicator (data-parallel schedule).  (bf16: data parallelism never runs the fused backward kernel,
    # whose summation order differs from the three launches it replaces, so both sides run those)
    if prec == pkg.BF16:
        nofuse = [(pkg.OPT_FUSED_BWD, 0)]
        assert_identical(run(options=nofuse + [(pkg.OPT_FORCE_COMM, 1)], comm=True), run(options=nofuse))
    else:
        assert_identical(run(options=[(pkg.OPT_FORCE_COMM, 1)], comm=True), base)
    # graph replay: eager (warm-up), capture + launch, replay == three eager calls
    assert_identical(run(options=[(pkg.OPT_UPDATE_GRAPH, 1)], calls=3), run(calls=3))
    # shuffled == contiguous on the host-permuted batch, values permuted with it
    eng = pkg.Engine(E, T, A, H, precision=prec)
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
    eng.load_params(params)
    obs, actions, old_lp, adv, masks = batch
    eng.set_batch(obs, actions, old_lp, adv, ret, masks, values=vold)
    m = eng.train(LR, epochs, M)
    order = eng.sample_order(epochs)
    shuf = uh.read_update(eng, m, epochs, M)
    eng.close()
    assert (order != np.arange(N)[None]).any()
    eng = pkg.Engine(E, T, A, H, precision=prec)
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    eng.load_params(params)
    for e in range(epochs):
        o = order[e]
        eng.set_batch(obs[o], actions[o], old_lp[o], adv[o], ret[o], masks[o], values=vold[o])
        me = eng.train(LR, 1, M)
        ce = uh.read_update(eng, me, 1, M)
        for k in me:
            np.testing.assert_array_equal(me[k][0], shuf["m"][k][e], err_msg=k)
        for k in PER_SAMPLE:
            np.testing.assert_array_equal(ce[k][0], shuf[k][e], err_msg=k)
        for k in ("approx_kl", "clip_fraction"):
            np.testing.assert_array_equal(ce["diag"][k][0], shuf["diag"][k][e], err_msg=k)
    np.testing.assert_array_equal(eng.export_params(), shuf["params"])
    np.testing.assert_array_equal(eng.export_grads(), shuf["grads"])
    eng.close()


@pytest.mark.gpu
def test_toggling_between_graph_replays_matches_a_fresh_eager_context(pkg):
    E, T, A, H, epochs, M, params, batch, ret, vold = _fp32_case(pkg)
    seq = [1, 1, 1, 0, 0, 0, 1, 1]  # the option before each call: captures with it on, off and on again

    def drive(graph):
        eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
        if graph:
            eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
        eng.load_params(params)
        eng.set_batch(*batch[:4], ret, batch[4], values=vold)
        outs = []
        for v in seq:
            if eng.get_option(pkg.OPT_VALUE_CLIP) != v:
                eng.set_option(pkg.OPT_VALUE_CLIP, v)
            outs.append(uh.read_update(eng, eng.train(LR, epochs, M), epochs, M))
        replays = eng.get_option(pkg.OPT_UPDATE_GRAPH)
        eng.close()
        return outs, replays

    g, replays = drive(True)
    e, _ = drive(False)
    assert replays >= 4  # (per run of equal settings: eager, capture + launch, replay)
    for a, b in zip(g, e):
        assert_identical(a, b)
    assert (g[2]["value_losses"] != g[3]["value_losses"]).any()


@pytest.mark.gpu
def test_option_off_restores_the_default(pkg):
    E, T, A, H, epochs, M, params, batch, ret, vold = _fp32_case(pkg)
    never = _run(pkg, E, T, A, H, pkg.FP32, params, batch, ret, None, epochs, M, clip_on=False)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    assert eng.get_option(pkg.OPT_VALUE_CLIP) == 0
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    assert eng.get_option(pkg.OPT_VALUE_CLIP) == 1
    eng.set_option(pkg.OPT_VALUE_CLIP, 0)
    assert eng.get_option(pkg.OPT_VALUE_CLIP) == 0
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_option(pkg.OPT_VALUE_CLIP, 2)
    eng.load_params(params)
    obs, actions, old_lp, adv, masks = batch
    eng.set_batch(obs, actions, old_lp, adv, ret, masks, values=vold)  # (values given, clipping off: unused)
    toggled = uh.read_update(eng, eng.train(LR, epochs, M), epochs, M)
    eng.close()
    assert_identical(toggled, never)
    # the diagnostics with clipping off against the reference (= orc.train for everything else)
    ref = ur.composed_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, lr=LR)
    B = E * T // M
    _check_fp32(never, ref, np.broadcast_to(masks.reshape(M, B), (epochs, M, B)).astype(np.float64), params0=params)


@pytest.mark.gpu
def test_error_cases(pkg):
    E, T, A, H = 4, 8, 4, 32
    N = E * T
    obs, actions, old_lp, adv, masks = _planes(4600, N, A)
    ret = hf.hf_range(4606, (N,), -1, 1)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    eng.load_params(hf.fill_params(4601, H, A))
    with pytest.raises(pkg.AleppoError, match="aleppo_set_batch"):
        eng.set_batch_values(np.zeros(N, np.float32))  # no caller batch yet
    eng.set_option(pkg.OPT_VALUE_CLIP, 1)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    with pytest.raises(pkg.AleppoError, match="aleppo_set_batch_values"):
        eng.train(LR, 1, 2)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_batch_values(np.zeros(N, np.float32), n=N - 1)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.set_batch_values(np.zeros(N - 4, np.float32))
    eng.set_batch_values(np.zeros(N, np.float32))
    eng.train(LR, 1, 2)
    with pytest.raises(pkg.AleppoInvalidArgument):  # the means are [epochs, M]
        eng.read_train_metric("approx_kl", 1, 2, 1)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)  # a new batch forgets the values
    with pytest.raises(pkg.AleppoError, match="aleppo_set_batch_values"):
        eng.train(LR, 1, 2)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shuffle", [("fp32", 0), ("fp32", 1), ("bf16", 0), ("bf16", 1)])
def test_one_call_equals_one_epoch_calls(pkg, prec, shuffle):
    E, T, A, H, M = 16, 32, 4, 256, 2
    N = E * T
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(4700, H, A)
    obs, actions, old_lp, adv, masks = _planes(4701, N, A)
    _, v0 = orc.net_forward(params, H, A, obs)
    vold, ret = _values_and_returns(4710, v0)
    outs = []
    for split in (False, True):
        eng = pkg.Engine(E, T, A, H, precision=p)
        eng.set_option(pkg.OPT_VALUE_CLIP, 1)
        eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, shuffle)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks, values=vold)
        if split:
            o = uh.concat_updates([uh.read_update(eng, eng.train(LR, 1, M), 1, M) for _ in range(4)])
        else:
            o = uh.read_update(eng, eng.train(LR, 4, M), 4, M)
        outs.append(o)
        eng.close()
    assert_identical(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("target_kl,epochs", [("1e-12", 1), ("1e9", 2)])
def test_trainer_target_kl_on_the_device(trainer, tmp_path, target_kl, epochs):
    cfg = _debug_cfg(tmp_path, f"clip_value_loss: true\ntarget_kl: {target_kl}\n", rollouts=3)
    assert "num_epochs: 2" in cfg.read_text()
    os.makedirs(tmp_path / "tb")
    r = subprocess.run([trainer, "breakout.bin", str(tmp_path / "tb" / "run.log"), str(tmp_path), "g", str(cfg)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = _events(tmp_path / "tb")
    assert b"clip_value_loss" in blob
    assert event_scalars(blob, "update_epochs") == [float(epochs)] * 3
    kl = event_scalars(blob, "mean_approx_kl")
    assert len(kl) == 3 and all(np.isfinite(kl)) and min(kl) > 0
    assert len(event_scalars(blob, "mean_clip_fraction")) == 3
