"""The PPO update with every option at once, on a rollout batch: the eager, the captured and the serial schedule agree.

aleppo_train builds one plan per call (api_train.hip: UpdatePlan, and Planes - the contiguous-or-gathered choice of the
per-sample planes) and enqueues it eagerly, records it into a graph, or replays the graph.  This is the combination in
which every branch of that plan is taken together: minibatch shuffling (gathered planes, records per epoch and
minibatch), value clipping on a rollout batch (the old values are transposed inside the update and gathered), per-
minibatch advantage normalisation, the KL penalty with beta != 0, and the hyper-parameters from the device block.
Three contexts start from the same parameters and the same rollout and run three updates each:
  * eager:  ALEPPO_OPT_UPDATE_GRAPH off - three eager enqueues on two streams;
  * graph:  ALEPPO_OPT_UPDATE_GRAPH on  - an eager call, the capture and its first launch, a replay;
  * serial: ALEPPO_OPT_SERIAL_UPDATE on - every kernel on the main stream.
After every update they agree bit for bit in the parameters, the optimizer state, every aleppo_minibatch_metrics field,
the mean exact KL, the advantage statistics and the sample order: the update is deterministic (fixed summation orders),
so a difference is a difference of schedule, of a baked pointer, or of the record a minibatch read."""
import numpy as np
import pytest

import hashfill as hf
from shared_fixtures import pkg  # noqa: F401

E, T, H, EPOCHS, M = 8, 8, 32, 2, 2
N = E * T
LR = 2.5e-4
UPDATES = 3


@pytest.fixture(scope="module")
def trace():
    """one recorded rollout: frames, flags and rewards of T slots (shared, read-only)"""
    from test_gpu_at_size import _flags
    frames = hf.hf_bytes(9101, (T, E, 84, 84))
    te, tr, st = _flags(9102, T, E)
    rew = hf.hf_range(9103, (T, E), -2, 2)
    for a in (frames, te, tr, st, rew):
        a.setflags(write=False)
    return frames, te, tr, st, rew


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(pkg, trace, prec, A, params, graph=0, serial=0):
    """the three updates of one context: a list of {name: array} per update"""
    from test_gpu_at_size import DeviceBytes
    frames, te, tr, st, rew = trace
    eng = pkg.Engine(E, T, A, H, precision=prec, seed=5)
    for opt in (pkg.OPT_MINIBATCH_SHUFFLE, pkg.OPT_VALUE_CLIP, pkg.OPT_ADV_NORM_MINIBATCH, pkg.OPT_KL_PENALTY):
        eng.set_option(opt, 1)
    eng.set_kl_coef(0.2)
    eng.set_hyper(entropy_coef=0.02)  # (one of the five: the device block is in use from here on)
    eng.set_option(pkg.OPT_SERIAL_UPDATE, serial)
    eng.set_option(pkg.OPT_UPDATE_GRAPH, graph)
    eng.load_params(params)
    dev = DeviceBytes(frames)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st)
    eng.finish_rollout()  # (a rollout batch: ALEPPO_OPT_VALUE_CLIP's old values are values_tm, transposed in the update)
    dev.free()
    outs = []
    for k in range(UPDATES):
        m = eng.train(LR, EPOCHS, M)
        # eager -> capture + first launch -> replay: the launch counter says which of the three this call was
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) == (k if graph else 0)
        sd = eng.state_dict()
        mean, std = eng.advantage_stats(EPOCHS, M)
        out = {"m." + name: v for name, v in m.items()}
        out.update(params=sd["params"], exp_avg=sd["exp_avg"], exp_avg_sq=sd["exp_avg_sq"], step=np.int64(sd["step"]),
                   mean_kl=eng.kl_divergence(EPOCHS, M), adv_mean=mean, adv_std=std, order=eng.sample_order(EPOCHS))
        outs.append(out)
    eng.close()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("A", [6, 18])
def test_eager_captured_and_serial_updates_agree_bit_for_bit(pkg, trace, prec, A):
    p = pkg.BF16 if prec == "bf16" else pkg.FP32
    params = hf.fill_params(9100 + A, H, A)
    eager = _run(pkg, trace, p, A, params)
    others = {"graph": _run(pkg, trace, p, A, params, graph=1), "serial": _run(pkg, trace, p, A, params, serial=1)}
    for k, ref in enumerate(eager):
        # the characterised thing ran: shuffled orders that are permutations, a penalty that bites, finite numbers
        assert ref["step"] == (k + 1) * EPOCHS * M
        assert (np.sort(ref["order"], axis=1) == np.arange(N)).all() and (ref["order"] != np.arange(N)).any()
        assert all(np.isfinite(v).all() for v in ref.values())
        assert (ref["mean_kl"] > 0).any() and (ref["adv_std"] > 0).all()
        for name, outs in others.items():
            assert set(outs[k]) == set(ref)
            for key, want in ref.items():
                np.testing.assert_array_equal(_bits(outs[k][key]), _bits(want), err_msg=f"{name}, update {k}: {key}")
    assert not np.array_equal(eager[0]["params"], params) and not np.array_equal(eager[0]["order"], eager[1]["order"])
