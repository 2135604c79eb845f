"""ALEPPO_OPT_CLIP_PARAM / ALEPPO_OPT_VALUE_CLIP_RANGE / ALEPPO_OPT_VALUE_LOSS_COEF / ALEPPO_OPT_ENTROPY_COEF /
ALEPPO_OPT_MAX_GRAD_NORM: the clip range, the loss coefficients and the gradient-norm limit per update, as device values.

The yardstick needs no tolerance: a context created with values X in its config and a context created with other
values and then set to X through the options give bit-identical parameters, Adam moments, minibatch metrics,
per-sample planes and exported gradients from the same parameters and batch.

CPU: the header constants against the Python mirror, the wrapper's float <-> bits conversions, and the trainer's
*_final / value_clip_range keys against the host-only library stand-in (the scheduled values are read from the scalars
the trainer logs per rollout).
GPU (-m gpu, everything through the C ABI): the bit equality above in fp32 and bf16, H = 512 and H = 96, A = 4 and 18,
caller and rollout batches (fp32 and fp16 planes), alone and with shuffling + value clipping + per-minibatch advantage
normalisation + the KL penalty; a value-clip range of its own against update_ref.py; fp32 against the oracle and
bf16 against the emulation, called with the option values; a schedule under ALEPPO_OPT_UPDATE_GRAPH against the same
schedule run eagerly; each number's own effect; validation; the 1-rank communicator."""
import functools
import os
import re
import struct

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
import update_harness as uh
import update_ref as ur
from shared_fixtures import pkg, stub_trainer  # noqa: F401
from trainer_helpers import debug_cfg as _debug_cfg, event_scalars, events as _events, header_const as const, run_stub
from update_harness import assert_identical
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 2e-5
# X: the values under test, all different from the defaults; OTHER: what the second context is created with
X = dict(clip_param=0.17, value_loss_coef=0.8, entropy_coef=0.03, max_gradient_norm=0.3)
OTHER = dict(clip_param=0.05, value_loss_coef=0.25, entropy_coef=0.002, max_gradient_norm=7.0)
read_state = functools.partial(uh.read_update, state=True)  # (with the Adam moments and the step)
OPTS = ("OPT_CLIP_PARAM", "OPT_VALUE_CLIP_RANGE", "OPT_VALUE_LOSS_COEF", "OPT_ENTROPY_COEF", "OPT_MAX_GRAD_NORM")


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------ CPU
def test_header_constants_and_python_mirror():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()

    assert const("ALEPPO_OPT_KL_COEF") == 16  # (the five are the next free numbers after it)
    for k, name in enumerate(OPTS):
        assert const("ALEPPO_" + name) == getattr(pkg, name) == 17 + k
    abi = re.search(r"(?m)^#define ALEPPO_ABI_VERSION\s+(\d+)", hdr)
    assert abi and int(abi.group(1)) == pkg.ABI_VERSION  # (not bumped)
    assert set(pkg.HYPER_OPTIONS) == {"clip_param", "value_clip_range", "value_loss_coef", "entropy_coef",
                                      "max_grad_norm"}
    assert hasattr(pkg.Engine, "set_hyper") and hasattr(pkg.Engine, "hyper")


def test_float_bits_conversions():
    """pure Python: what Engine.set_hyper hands to aleppo_set_option and what Engine.hyper makes of aleppo_get_option"""
    pkg = load_package()
    assert pkg.float_bits(1.0) == 0x3F800000 and pkg.float_bits(0.0) == 0 and pkg.float_bits(0.5) == 0x3F000000
    assert pkg.float_bits(0.1) == 0x3DCCCCCD  # rounded to float32 (nearest even)
    assert pkg.float_bits(-0.0) == -2 ** 31 and pkg.float_bits(-1.0) < 0  # sign bit set: negative as an int
    assert pkg.float_bits(float("inf")) == 0x7F800000 and pkg.float_bits(float("nan")) >= 0x7F800001
    assert pkg.bits_float(0x3F800000) == 1.0 and pkg.bits_float(0) == 0.0
    assert pkg.bits_float(-2 ** 31) == 0.0 and str(pkg.bits_float(-2 ** 31)) == "-0.0"  # (int64 from get_option)
    for x in (0.1, 0.17, 2.5e-4, 1e-30, 3e38, 1.0 / 3.0):
        assert pkg.bits_float(pkg.float_bits(x)) == _f32(x)
        assert pkg.float_bits(x) == _bits(x)
    # a fake context: set_hyper sends only what was given, as bits, under the right option; hyper reads all five back
    sent = {}

    class Fake(pkg.Engine):
        def __init__(self):
            pass

        def __del__(self):
            pass

        def set_option(self, option, value):
            sent[option] = value

        def get_option(self, option):
            return sent.get(option, pkg.float_bits(0.25))

    e = Fake()
    e.set_hyper(clip_param=0.2, max_grad_norm=2.0)
    assert sent == {pkg.OPT_CLIP_PARAM: pkg.float_bits(0.2), pkg.OPT_MAX_GRAD_NORM: 0x40000000}
    e.set_hyper(value_clip_range=0.3, value_loss_coef=0.0, entropy_coef=0.01)
    assert sent[pkg.OPT_VALUE_LOSS_COEF] == 0 and sent[pkg.OPT_VALUE_CLIP_RANGE] == pkg.float_bits(0.3)
    assert e.hyper() == dict(clip_param=_f32(0.2), value_clip_range=_f32(0.3), value_loss_coef=0.0,
                             entropy_coef=_f32(0.01), max_grad_norm=2.0)


def _yaml_value(key):
    m = re.search(rf"(?m)^{key}: (\S+)", open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read())
    return float(m.group(1))


def test_trainer_anneals_the_scheduled_values(stub_trainer, tmp_path):
    """rollout i of n uses float(v0 + (v_final - v0) * i / n), in double: rollouts 0, 1 and the last"""
    n = 5
    final = dict(clip_param=0.01, entropy_coef=0.0, value_loss_coef=1.0, max_gradient_norm=0.1)
    extra = "".join(f"{k}_final: {v}\n" for k, v in final.items())
    r = run_stub(stub_trainer, tmp_path, _debug_cfg(tmp_path, extra, rollouts=n))
    assert r.returncode == 0, r.stderr[-2000:]
    data = _events(tmp_path)
    for k, v1 in final.items():
        v0 = float(np.float32(_yaml_value(k)))  # (the config's values are floats)
        got = event_scalars(data, k)
        want = [_f32(v0 + (v1 - v0) * (i / n)) for i in range(n)]
        assert len(got) == n, (k, got)
        for i in (0, 1, n - 1):
            assert got[i] == want[i], (k, i, got, want)
        assert got == want and got[0] == _f32(v0) and got[-1] != _f32(v1)  # like the learning rate: the end is not reached
        assert (k + "_final").encode() in data  # hparams
    assert len(event_scalars(data, "learning_rate")) == n


def test_trainer_without_the_keys_sets_and_logs_nothing(stub_trainer, tmp_path):
    r = run_stub(stub_trainer, tmp_path, _debug_cfg(tmp_path, "", rollouts=2))
    assert r.returncode == 0, r.stderr[-2000:]
    data = _events(tmp_path)
    for k in ("clip_param", "entropy_coef", "value_loss_coef", "max_gradient_norm"):
        assert event_scalars(data, k) == [] and (k + "_final").encode() not in data
    assert b"value_clip_range" not in data and len(event_scalars(data, "learning_rate")) == 2


def test_trainer_value_clip_range_is_a_constant_hparam(stub_trainer, tmp_path):
    r = run_stub(stub_trainer, tmp_path, _debug_cfg(tmp_path, "clip_value_loss: true\nvalue_clip_range: 0.3\n", 2))
    assert r.returncode == 0, r.stderr[-2000:]
    assert b"value_clip_range" in _events(tmp_path)


@pytest.mark.parametrize("extra,msg", [
    ("clip_param_final: 0\n", "clip_param_final and the value it starts from must be finite and positive"),
    ("clip_param_final: -0.1\n", "clip_param_final and the value it starts from must be finite and positive"),
    ("max_gradient_norm_final: 0\n", "max_gradient_norm_final and the value it starts from must be finite and positive"),
    ("entropy_coef_final: -1e-3\n", "entropy_coef_final and the value it starts from must be finite and non-negative"),
    ("value_loss_coef_final: 1e39\n", "value_loss_coef_final and the value it starts from must be finite and non-negative"),
    ("clip_value_loss: true\nvalue_clip_range: 0\n", "value_clip_range must be finite and positive"),
    ("value_clip_range: 0.2\n", "value_clip_range needs clip_value_loss: true"),
])
def test_trainer_refuses_invalid_values_at_load_time(stub_trainer, tmp_path, extra, msg):
    r = run_stub(stub_trainer, tmp_path, _debug_cfg(tmp_path, extra, rollouts=4))
    assert r.returncode != 0 and msg in r.stdout + r.stderr, (r.returncode, r.stderr[-2000:])
    assert "Rollout 1" not in r.stdout


# ------------------------------------------------------------------ GPU
_hashed = functools.partial(uh.hashed_batch, mask_p=0.15)


def _set_x(eng, x, value_clip_range=None):
    eng.set_hyper(clip_param=x["clip_param"], value_loss_coef=x["value_loss_coef"], entropy_coef=x["entropy_coef"],
                  max_grad_norm=x["max_gradient_norm"], value_clip_range=value_clip_range)


def _pair(pkg, E, T, A, H, prec, prepare, epochs=2, M=2, options=(), kl=False, lr=LR, **kw):
    """(a context created with X, a context created with OTHER and set to X): the outputs of one aleppo_train each.
    prepare(eng) loads the parameters and the batch."""
    outs = []
    for via_options in (False, True):
        eng = uh.make_engine(pkg, E, T, A, H, prec, options, **(OTHER if via_options else X), **kw)
        if kl:
            eng.set_kl_coef(0.2)
        prepare(eng)
        if via_options:
            _set_x(eng, X)
            assert eng.hyper() == dict(clip_param=_f32(X["clip_param"]), value_clip_range=_f32(X["clip_param"]),
                                       value_loss_coef=_f32(X["value_loss_coef"]),
                                       entropy_coef=_f32(X["entropy_coef"]),
                                       max_grad_norm=_f32(X["max_gradient_norm"]))
        outs.append(read_state(eng, eng.train(lr, epochs, M), epochs, M, kl=kl))
        eng.close()
    return outs


def _all_on(pkg):
    return [(pkg.OPT_MINIBATCH_SHUFFLE, 1), (pkg.OPT_VALUE_CLIP, 1), (pkg.OPT_ADV_NORM_MINIBATCH, 1),
            (pkg.OPT_KL_PENALTY, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H,A", [(512, 4), (96, 18), (512, 18), (96, 4)])
def test_options_equal_config_bit_for_bit_on_a_caller_batch(pkg, prec, H, A):
    E, T = 8, 16
    params = hf.fill_params(7100 + H + A, H, A)
    batch = _hashed(7101, E * T, A)
    _, v0 = orc.net_forward(params, H, A, batch[0])
    vold = (v0 + hf.hf_range(7102, (E * T,), -0.3, 0.3)).astype(np.float32)

    def prepare(eng):
        eng.load_params(params)
        eng.set_batch(*batch, values=vold)

    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    a, b = _pair(pkg, E, T, A, H, p, prepare)
    assert_identical(a, b)
    assert np.isfinite(a["params"]).all() and (a["exp_avg_sq"] > 0).any() and a["step"] == 4
    # ... and with shuffling + value clipping + per-minibatch advantage normalisation + the KL penalty (beta = 0.2)
    a, b = _pair(pkg, E, T, A, H, p, prepare, options=_all_on(pkg), kl=True)
    assert_identical(a, b)
    assert (a["kl"] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("rollout_precision", ["fp32", "fp16"])
def test_options_equal_config_bit_for_bit_on_a_rollout_batch(pkg, prec, rollout_precision):
    from test_gpu_at_size import DeviceBytes, _flags
    E, T, A, H = 8, 16, 18, 512
    rp = pkg.ROLLOUT_FP16 if rollout_precision == "fp16" else pkg.ROLLOUT_FP32
    params = hf.fill_params(7200, H, A)
    frames = hf.hf_bytes(7201, (T, E, 84, 84))
    te, tr, st = _flags(7202, T, E)
    rew = hf.hf_range(7203, (T, E), -2, 2)

    def prepare(eng):
        dev = DeviceBytes(frames)
        eng.load_params(params)
        eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
        eng.finish_rollout()
        dev.free()

    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    for options, kl in (((), False), (_all_on(pkg), True)):
        # (a larger rate than LR: the policy has to leave the rollout's for the clip range to matter)
        a, b = _pair(pkg, E, T, A, H, p, prepare, options=options, kl=kl, lr=2.5e-4, seed=3, rollout_precision=rp)
        assert_identical(a, b)


@pytest.mark.gpu
def test_value_clip_range_of_its_own(pkg):
    """the value-loss plane and dL/dv follow ALEPPO_OPT_VALUE_CLIP's formulas with c = the range (update_ref.py at
    test_value_clip.py's fp32 bounds, 1e-4); the clipped-surrogate plane and the clip fraction are those of a run with
    the range unset, bit for bit"""
    E, T, A, H, epochs, M = 8, 32, 6, 64, 1, 1
    N = E * T
    clip, rng_v = 0.1, 0.03
    params = hf.fill_params(7300, H, A)
    batch = _hashed(7301, N, A)
    _, v0 = orc.net_forward(params, H, A, batch[0])
    vold = (v0 + hf.hf_range(7302, (N,), -0.12, 0.12)).astype(np.float32)
    outs = {}
    for name in ("unset", "set"):
        eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, clip_param=clip)
        eng.set_option(pkg.OPT_VALUE_CLIP, 1)
        eng.load_params(params)
        eng.set_batch(*batch, values=vold)
        if name == "set":
            eng.set_hyper(value_clip_range=rng_v)
            assert eng.hyper()["value_clip_range"] == _f32(rng_v) and eng.hyper()["clip_param"] == _f32(clip)
        else:
            eng.set_hyper(clip_param=clip)  # (the same setter traffic on both sides; the range follows the clip)
            assert eng.hyper()["value_clip_range"] == _f32(clip)
        outs[name] = read_state(eng, eng.train(LR, epochs, M), epochs, M)
        eng.close()
    s, u = outs["set"], outs["unset"]
    for k in ("clipped_losses", "clip_fraction", "ratio", "entropies", "approx_kl"):
        np.testing.assert_array_equal(s[k], u[k], err_msg=k)
    assert not np.array_equal(s["value_losses"], u["value_losses"])
    # update_ref's value branch with clip = the range gives the value term (its surrogate would clip at the range too, so only the
    # value plane and the value gradient are taken from it) ...
    logits, values = orc.net_forward(params, H, A, batch[0])
    lv, dv, zero = ur.value_branch(values, batch[4], vold, rng_v)
    lv_c, _, zero_c = ur.value_branch(values, batch[4], vold, clip)
    mk = batch[5] != 0
    assert (zero & mk).sum() > 10 and ((zero != zero_c) & mk).sum() > 10  # both branches, and the range matters
    np.testing.assert_allclose(s["value_losses"][0, 0], lv, atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(u["value_losses"][0, 0], lv_c, atol=1e-4, rtol=1e-4)
    # ... and the whole update against the reference composed with both ranges: update_ref at clip = range for the
    # value term, the oracle's surrogate at clip_param (composed below from the same pieces)
    o = orc.ppo_loss(logits, batch[2], batch[1], batch[3], values, batch[4], batch[5], clip, 0.5, 0.01)
    nm = np.float32(mk.sum())
    dvalues = np.where(mk, 0.5 * dv / float(nm), 0.0).astype(np.float32)
    _, _, acts = orc.net_forward(params, H, A, batch[0], want_acts=True)
    g = orc.net_backward(params, H, A, acts, o["dlogits"], dvalues)
    norm, g = orc.clip_grad_norm(g, H, A, 0.5)
    np.testing.assert_allclose(s["m"]["grad_norm"][0, 0], norm, rtol=1e-4)
    np.testing.assert_allclose(s["grads"], g, atol=1e-4)
    total = -o["clipped"] + np.float32(0.5) * lv.astype(np.float32) - np.float32(0.01) * o["entropies"]
    np.testing.assert_allclose(s["total_losses"][0, 0], total, atol=1e-4, rtol=1e-4)


def _x_kw(x):
    return dict(clip=x["clip_param"], c_v=x["value_loss_coef"], c_e=x["entropy_coef"], max_norm=x["max_gradient_norm"])


@pytest.mark.gpu
@pytest.mark.parametrize("H,A,N,M", [(512, 6, 96, 2), (64, 18, 40, 1)])
def test_fp32_against_the_oracle_called_with_the_option_values(pkg, H, A, N, M):
    """test_gpu_parity.py's test_train_vs_oracle with the oracle's clip, c_v, c_e, max_norm = the options' values"""
    params = hf.fill_params(510, H, A)
    obs, actions, old_lp, adv, ret, masks = _hashed(7400, N, A)
    eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.FP32, **OTHER)
    eng.load_params(params)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    _set_x(eng, X)
    m = eng.train(2.5e-4, 2, M)
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M, **_x_kw(X))
    np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=1e-3)
    np.testing.assert_allclose(eng.export_params(), w["params"], atol=1e-4)
    g, wg = eng.export_grads(), w["last_grads"]
    np.testing.assert_allclose(g, wg, atol=1e-5 + 2e-3 * np.abs(wg).max())
    # the config's own values would not pass: the options are what the update used
    wo = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M, **_x_kw(OTHER))
    assert not np.allclose(m["loss"], wo["loss"], atol=1e-4, rtol=0)
    eng.close()


@pytest.mark.gpu
def test_bf16_against_the_emulation_called_with_the_option_values(pkg):
    E, T, A, H, epochs, M = 12, 8, 4, 512, 2, 2
    params = hf.fill_params(7500, H, A)
    batch = _hashed(7501, E * T, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, **OTHER)
    eng.load_params(params)
    eng.set_batch(*batch)
    _set_x(eng, X)
    out = read_state(eng, eng.train(2.5e-4, epochs, M), epochs, M)
    eng.close()
    ref = bc.emulated_train(params, H, A, *batch, epochs, M, **_x_kw(X))
    c = bc.Checker()
    planes = {ours: out[ours] for ours, _ in bc.PLANES if ours in out}
    c.train(H, A, out["m"], planes, None, ref, params0=params, params=out["params"])
    print(c.summary("bf16 update with the hyper-parameter options vs the emulated oracle"))
    assert not c.failures, c.failures


SCHEDULE = [dict(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.0, max_gradient_norm=0.05),
            dict(clip_param=0.1, value_loss_coef=0.5, entropy_coef=0.01, max_gradient_norm=0.5),
            dict(clip_param=0.03, value_loss_coef=0.1, entropy_coef=0.05, max_gradient_norm=40.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_schedule_under_the_captured_update(pkg, prec):
    """Three updates with three settings of all four numbers, replayed from ONE captured graph, equal the same three
    updates run eagerly bit for bit, and the launch counter advances by three.  That the graph is not captured anew
    between them is not observable through the ABI: it is the option setter's re-arm list in aleppo_set_option
    (api_core.hip) that leaves graph_key alone for the five options, as for ALEPPO_OPT_KL_COEF; a re-armed capture would
    run the next update eagerly and the counter would not advance on it."""
    E, T, A, H, epochs, M = 16, 16, 6, 256, 2, 2
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(7600, H, A)
    batch = _hashed(7601, E * T, A)
    _, v0 = orc.net_forward(params, H, A, batch[0])
    vold = (v0 + hf.hf_range(7602, (E * T,), -0.3, 0.3)).astype(np.float32)
    outs = {}
    for graph in (0, 1):
        eng = pkg.Engine(E, T, A, H, precision=p)
        eng.set_option(pkg.OPT_VALUE_CLIP, 1)
        eng.set_option(pkg.OPT_UPDATE_GRAPH, graph)
        eng.load_params(params)
        eng.set_batch(*batch, values=vold)
        _set_x(eng, X)
        eng.train(LR, epochs, M)  # eager (warm-up: the first call of a shape is never captured)
        eng.train(LR, epochs, M)  # graph: capture + first launch
        n0 = eng.get_option(pkg.OPT_UPDATE_GRAPH)
        assert n0 == (1 if graph else 0)
        res = []
        for k, x in enumerate(SCHEDULE):
            _set_x(eng, x, value_clip_range=0.5 * x["clip_param"])
            res.append(read_state(eng, eng.train(LR, epochs, M), epochs, M))
            assert eng.get_option(pkg.OPT_UPDATE_GRAPH) == (n0 + k + 1 if graph else 0)
        outs[graph] = res
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        assert_identical(a, b)
    # the settings were followed: the three updates differ from one another in what the numbers govern
    assert not np.array_equal(outs[1][0]["clip_fraction"], outs[1][2]["clip_fraction"]) or \
        not np.array_equal(outs[1][0]["total_losses"], outs[1][2]["total_losses"])
    assert not np.array_equal(outs[1][0]["total_losses"], outs[1][1]["total_losses"])


@pytest.mark.gpu
def test_each_number_bites(pkg):
    E, T, A, H, M = 8, 32, 6, 64, 1
    N = E * T
    params = hf.fill_params(7700, H, A)
    batch = _hashed(7701, N, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, clip_param=0.2)
    eng.load_params(params)
    # a batch whose old log-probs are the current policy's: all ratios are 1; one step moves them apart (at 1e-4 the
    # oracle's |rho - 1| is below 0.1 on 132, between 0.1 and 0.2 on 44 and above on 37 of the 213 unmasked samples)
    logits, _ = orc.net_forward(params, H, A, batch[0])
    batch = (batch[0], batch[1], orc.log_softmax(logits)) + batch[3:]
    eng.set_batch(*batch)
    eng.train(1e-4, 1, M)
    p1 = eng.export_params()

    def run(**hyper):
        eng.load_params(p1)  # (resets Adam: every run below is the same step from the same state)
        eng.set_hyper(**hyper)
        return read_state(eng, eng.train(LR, 1, M), 1, M)

    wide = run(clip_param=0.2)
    mk = batch[5] != 0
    dev = np.abs(wide["ratio"][0, 0].astype(np.float64) - 1)
    between = (dev > 0.1 + 1e-6) & (dev < 0.2 - 1e-6) & mk
    assert between.sum() > 5, between.sum()  # ratios between the two ranges
    narrow = run(clip_param=0.1)
    cf_w, cf_n = wide["diag"]["clip_fraction"][0, 0], narrow["diag"]["clip_fraction"][0, 0]
    np.testing.assert_allclose(cf_n - cf_w, between.sum() / mk.sum(), atol=1e-6)
    np.testing.assert_array_equal(narrow["ratio"], wide["ratio"])
    # entropy_coef = 0: loss == -clipped + c_v value  (aleppo.h: total = -clipped + c_v value - c_e entropy), at the
    # existing loss bound 1e-4, per sample and in the minibatch means
    c_v = 0.7
    noent = run(clip_param=0.2, entropy_coef=0.0, value_loss_coef=c_v)
    np.testing.assert_allclose(noent["total_losses"], -noent["clipped_losses"] + np.float32(c_v) * noent["value_losses"],
                               atol=1e-4, rtol=0)
    m = noent["m"]
    np.testing.assert_allclose(m["loss"], -m["clipped_loss"] + _f32(c_v) * m["value_loss"], atol=1e-4, rtol=0)
    withent = run(entropy_coef=0.01)
    assert np.abs(withent["total_losses"] - noent["total_losses"]).max() > 1e-3
    # a tiny max_grad_norm scales the exported gradients to that norm; the reported pre-clip norm does not depend on it
    big = run(max_grad_norm=1e6)
    tiny = run(max_grad_norm=1e-3)
    np.testing.assert_array_equal(big["m"]["grad_norm"], tiny["m"]["grad_norm"])
    pre = float(big["m"]["grad_norm"][0, 0])
    assert pre > 0.1
    np.testing.assert_allclose(np.linalg.norm(tiny["grads"].astype(np.float64)), 1e-3, rtol=1e-4)
    np.testing.assert_allclose(np.linalg.norm(big["grads"].astype(np.float64)), pre, rtol=1e-4)  # (not clipped)
    np.testing.assert_allclose(tiny["grads"], big["grads"] * np.float32(_f32(1e-3) / (np.float32(pre) + np.float32(1e-6))),
                               rtol=1e-5, atol=1e-12)
    eng.close()


@pytest.mark.gpu
def test_validation_and_defaults(pkg):
    cfgv = dict(clip_param=0.125, value_loss_coef=0.75, entropy_coef=0.0, max_gradient_norm=3.0)
    eng = pkg.Engine(8, 8, 4, 32, precision=pkg.FP32, **cfgv)
    opt = {n: getattr(pkg, n) for n in OPTS}
    # before any set: the config's bits (the value-clip range: the clip parameter's)
    want = dict(OPT_CLIP_PARAM=0.125, OPT_VALUE_CLIP_RANGE=0.125, OPT_VALUE_LOSS_COEF=0.75, OPT_ENTROPY_COEF=0.0,
                OPT_MAX_GRAD_NORM=3.0)
    for n, v in want.items():
        assert eng.get_option(opt[n]) == _bits(v), n
    # the range follows the clip parameter until it is set itself, then stays
    eng.set_hyper(clip_param=0.3)
    assert eng.get_option(opt["OPT_VALUE_CLIP_RANGE"]) == _bits(0.3)
    eng.set_hyper(value_clip_range=0.07)
    eng.set_hyper(clip_param=0.125)  # (setting the config's own value is allowed)
    assert eng.get_option(opt["OPT_VALUE_CLIP_RANGE"]) == _bits(0.07)
    assert eng.get_option(opt["OPT_CLIP_PARAM"]) == _bits(0.125)
    want["OPT_VALUE_CLIP_RANGE"] = 0.07
    # invalid bit patterns: refused, and the previous value survives
    neg0, neg, inf, nan, nnan, ninf = (_bits(-0.0), _bits(-0.5), 0x7F800000, 0x7FC00000, _bits(-float("nan")),
                                       _bits(-float("inf")))
    for n in OPTS:
        bad = [neg0, neg, inf, nan, nnan, ninf, 0x7F800001, 0x7FFFFFFF]
        if n not in ("OPT_VALUE_LOSS_COEF", "OPT_ENTROPY_COEF"):
            bad.append(0)  # zero where > 0 is required
        for b in bad:
            with pytest.raises(pkg.AleppoInvalidArgument):
                eng.set_option(opt[n], b)
            assert eng.get_option(opt[n]) == _bits(want[n]), (n, hex(b & 0xFFFFFFFF))
    # the edges of the valid sets are accepted: the smallest denormal, the largest finite float, and +0.0 for the two
    # coefficients
    for n in OPTS:
        for b in (1, 0x7F7FFFFF) + ((0,) if n in ("OPT_VALUE_LOSS_COEF", "OPT_ENTROPY_COEF") else ()):
            eng.set_option(opt[n], b)
            assert eng.get_option(opt[n]) == b
    # unknown options are still refused, by both entry points
    for bad_opt in (22, 8, 99, -1):
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.set_option(bad_opt, 1)
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.get_option(bad_opt)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_rank_communicator_is_bit_identical(pkg, prec):
    """data parallel through the 1-rank communicator (ALEPPO_OPT_FORCE_COMM) against the single-GPU route, like for
    like: the fused backward kernel is off under data parallelism, so off on both sides.  Real multi-rank runs are not
    covered (every rank has to set the same values: aleppo.h)."""
    E, T, A, H, epochs, M = 16, 32, 4, 256, 2, 2
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(7800, H, A)
    batch = _hashed(7801, E * T, A)
    _, v0 = orc.net_forward(params, H, A, batch[0])
    vold = (v0 + hf.hf_range(7802, (E * T,), -0.3, 0.3)).astype(np.float32)
    outs = []
    for comm in (False, True):
        eng = pkg.Engine(E, T, A, H, precision=p, **OTHER)
        if comm:
            eng.comm_init(pkg.Engine.comm_unique_id())
            eng.set_option(pkg.OPT_FORCE_COMM, 1)
        for k, v in _all_on(pkg) + [(pkg.OPT_FUSED_BWD, 0)]:
            eng.set_option(k, v)
        eng.set_kl_coef(0.2)
        eng.load_params(params)
        eng.set_batch(*batch, values=vold)
        _set_x(eng, X, value_clip_range=0.06)
        outs.append(read_state(eng, eng.train(LR, epochs, M), epochs, M, kl=True))
        eng.close()
    assert_identical(outs[0], outs[1])
