"""Evaluation lanes (aleppo_eval_open / _push_frames / _act / _read; pytest -m gpu on the MI355X).

1. the lanes run aleppo_act's kernels: L == E, the same frames, SAMPLE at tau = 1 with aleppo_act's noise -> bit-identical
2. the forward for L != E against the oracles, the stacks byte-exact, lanes restarting mid-sequence
3. the three rules on the engine's own logits against tests/eval_ref.py
4. the built-in generator: reproducible, keyed by the seed, restarted by aleppo_eval_open, the documented indexing,
   a binomial count, and no influence on aleppo_act's stream
5. isolation: a scripted training run with and without evaluation calls is bit-identical (eager, captured update,
   slot-ahead loop)
6. every refusal, and that a refused call changes nothing
7. the trainer's eval_* keys: the four eval/* scalars, and a training run that is bit-identical to the run without them"""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bf16_check as bc
import eval_ref as er
import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401
from conftest import ROOT
from test_gpu_at_size import DeviceBytes

pytestmark = pytest.mark.gpu


def _exp_noise(seed, shape):
    n = int(np.prod(shape))
    return (-np.log(np.clip(hf.hf_unit(seed, n), 1e-6, 1.0))).astype(np.float32).reshape(shape)


def _f84(frames, raw):
    return frames if not raw else orc.preprocess(frames, np.arange(256, dtype=np.uint8))


def _frames(seed, n, raw):
    return hf.hf_bytes(seed, (n, 2, 210, 160) if raw else (n, 84, 84))


# ------------------------------------------------------------------ 1. same kernels as acting
def _lanes_equal_acting(pkg, prec, raw, A, E, T, H):
    """L == E lanes fed the frames the rollout is fed: actions, logits and values of SAMPLE at tau = 1 with aleppo_act's
    noise equal aleppo_act's (fp32 planes), every lane, every slot - the rollout side through aleppo_step (fused ingest +
    acting launch on bf16 with 84x84 frames), the lanes through eval_push_frames + eval_act"""
    kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
    eng.load_params(hf.fill_params(4100, H, A))
    eng.eval_open(E)
    noise = _exp_noise(4101, (T, E, A))
    rng = np.random.default_rng(4102)
    start = np.ones(E, np.uint8)
    acts, ev = [], []
    for t in range(T):
        acts.append(eng.act(noise[t]).copy())
        a = eng.eval_act("sample", temperature=1.0, noise=noise[t]).copy()
        ev.append((a, eng.eval_read("logits"), eng.eval_read("values"), eng.eval_read("actions")))
        fr = _frames(4103 + t, E, raw)
        eng.step(fr, np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8), start, kind=kind)
        eng.eval_push_frames(fr, start, kind=kind)
        start = (rng.random(E) < 0.2).astype(np.uint8)
    np.testing.assert_array_equal(eng.eval_read("observations"), eng.read_batch("current_obs"))
    eng.finish_rollout(noise[0])
    logits, values, actions = eng.read_batch("logits"), eng.read_batch("values"), eng.read_batch("actions")
    for t in range(T):
        np.testing.assert_array_equal(ev[t][0], acts[t], err_msg=f"slot {t}: pinned actions")
        np.testing.assert_array_equal(ev[t][3], actions[:, t], err_msg=f"slot {t}: actions")
        np.testing.assert_array_equal(ev[t][1], logits[:, t], err_msg=f"slot {t}: logits")
        np.testing.assert_array_equal(ev[t][2], values[:, t], err_msg=f"slot {t}: values")
    eng.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("raw", [0, 1], ids=["frames84", "rawpair"])
@pytest.mark.parametrize("A", [4, 18])
def test_sample_at_unit_temperature_is_aleppo_act_bit_for_bit(pkg, prec, raw, A):
    _lanes_equal_acting(pkg, prec, raw, A, E=37, T=5, H=128)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [32, 512])
def test_sample_at_unit_temperature_is_aleppo_act_at_the_head_tile_extremes(pkg, prec, H):
    """the branches of the shared head pieces that H = 128, E = 37 never reach: H = 32, where only 4 lanes of a wave own
    hidden units; H = 512, where all 64 do and the LDS tile is at its largest, (18 + 1) * 512 * 4 = 38,912 bytes; and
    E = 5, a second workgroup with one live wave and three that only meet the barrier of the ticket publish"""
    _lanes_equal_acting(pkg, prec, 0, 18, E=5, T=2, H=H)


# ------------------------------------------------------------------ 2. forward against the oracle for L != E
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("L,how", [(1, "mapped"), (37, "raw"), (257, "device"), (4096, "host")])
def test_lane_forward_and_stacks_vs_oracle(pkg, prec, L, how):
    """E = 8 training environments, L lanes: four pushes (every lane starts at the first, some restart at the third), the
    stacks byte-exact against orc.update_observations (orc.preprocess for raw pairs) after every push; logits / values of a
    GREEDY act against orc.net_forward at 1e-4 (fp32) or the bf16-emulating oracle under bf16_check's bounds (bf16) after
    every push, every lane"""
    E, T, A, H = 8, 4, 6, 64
    raw = how == "raw"
    kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    params = hf.fill_params(4200, H, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
    eng.load_params(params)
    eng.eval_open(L)
    fbytes = L * (2 * 210 * 160 if raw else 7056)
    mapped = eng.host_alloc(fbytes) if how == "mapped" else None
    obs = np.zeros((L, 4, 84, 84), np.uint8)
    c = bc.Checker()
    steps = 4
    for k in range(steps):
        fr = _frames(4201 + 7 * k + L, L, raw)
        st = np.ones(L, np.uint8) if k == 0 else ((hf.hf_unit(4250 + k, L) < 0.3).astype(np.uint8) if k == 2
                                                  else np.zeros(L, np.uint8))
        if how == "device":
            d = DeviceBytes(fr)
            eng.eval_push_frames(None, st, kind=kind, device_ptr=d.addr)
            eng.synchronize()
            d.free()
        elif how == "mapped":
            ctypes.memmove(mapped, fr.ctypes.data, fbytes)
            eng._c(pkg.lib().aleppo_eval_push_frames(eng._ctx, ctypes.c_void_p(mapped), kind, pkg.HOST_MAPPED,
                                                     st.ctypes.data_as(ctypes.c_void_p)))
            eng.synchronize()
        else:
            eng.eval_push_frames(fr, st, kind=kind)
        obs = orc.update_observations(obs, _f84(fr, raw), st)
        np.testing.assert_array_equal(eng.eval_read("observations"), obs, err_msg=f"push {k}")
        a = eng.eval_act("greedy").copy()
        logits, values = eng.eval_read("logits"), eng.eval_read("values")
        np.testing.assert_array_equal(a, er.greedy(logits))
        if prec == "fp32":
            wl, wv = orc.net_forward(params, H, A, obs)
            np.testing.assert_allclose(logits, wl, atol=1e-4, rtol=0)
            np.testing.assert_allclose(values, wv, atol=1e-4, rtol=0)
        else:
            c.forward(logits, values, bc.emulated_forward(params, H, A, obs), f"push{k}_")
    if mapped is not None:
        eng.host_free(mapped)
    eng.close()
    if prec == "bf16":
        print(c.summary(f"eval lanes L={L}"))
        assert not c.failures, c.failures


# ------------------------------------------------------------------ 3. the rules on the engine's own logits
RULE_L, RULE_A, RULE_H = 2048, 6, 64


def _rule_engine(pkg, params=None, L=RULE_L, A=RULE_A, seed=42):
    eng = pkg.Engine(8, 4, A, RULE_H, precision=pkg.FP32, seed=seed)
    eng.load_params(hf.fill_params(4300, RULE_H, A) if params is None else params)
    eng.eval_open(L)
    eng.eval_push_frames(hf.hf_bytes(4301, (L, 84, 84)), np.ones(L, np.uint8))
    eng.eval_push_frames(hf.hf_bytes(4302, (L, 84, 84)), np.zeros(L, np.uint8))
    return eng


def test_greedy_is_the_first_maximum_also_on_exact_ties(pkg):
    eng = _rule_engine(pkg)
    a = eng.eval_act("greedy").copy()
    z = eng.eval_read("logits")
    np.testing.assert_array_equal(a, er.greedy(z))
    np.testing.assert_array_equal(eng.eval_read("actions"), a)
    assert len(np.unique(a)) > 1  # (the hash-filled lanes do not all prefer one action)
    eng.close()
    # zero action-head weights and biases: every lane's logits tie exactly, the first maximum is action 0
    p = hf.fill_params(4300, RULE_H, RULE_A)
    offs = orc.param_offsets(RULE_H, RULE_A)
    p[offs[8]:offs[10]] = 0
    eng = _rule_engine(pkg, p)
    a = eng.eval_act("greedy").copy()
    assert (eng.eval_read("logits") == 0).all()
    assert (a == 0).all()
    # a two-way tie that is not at index 0: only actions 2 and 4 carry a (common) bias
    p[offs[9] + 2] = p[offs[9] + 4] = 0.5
    eng.load_params(p)
    assert (eng.eval_act("greedy") == 2).all()
    eng.close()


def test_epsilon_greedy_with_given_uniforms_is_exact(pkg):
    eng = _rule_engine(pkg)
    L, A = RULE_L, RULE_A
    uw = np.stack([hf.hf_unit(4310, L), hf.hf_unit(4311, L)], 1).astype(np.float32)
    uw[:64, 0] = np.float32(0.25)                      # u == epsilon: not < epsilon, so greedy
    uw[64:128, 0] = np.nextafter(np.float32(0.25), np.float32(0))  # just below: explores
    top = np.nextafter(np.float32(1), np.float32(0))   # the largest w: maps to A - 1
    uw[:32, 1] = uw[64:96, 1] = top
    uw[32:64, 1] = np.float32((A - 1) / A)
    for eps in (0.0, 1.0, 0.25):
        a = eng.eval_act("epsilon", epsilon=eps, noise=uw).copy()
        z = eng.eval_read("logits")
        want = er.epsilon_greedy(z, eps, uw)
        np.testing.assert_array_equal(a, want, err_msg=f"epsilon {eps}")
        if eps == 0.0:
            np.testing.assert_array_equal(a, er.greedy(z))
        if eps == 1.0:
            assert (a[:32] == A - 1).all() and (a == np.minimum((uw[:, 1] * np.float32(A)).astype(np.int64), A - 1)).all()
        if eps == 0.25:
            np.testing.assert_array_equal(a[:64], er.greedy(z)[:64])
            assert (a[64:96] == A - 1).all()
    eng.close()


@pytest.mark.parametrize("tau", [0.25, 4.0])
def test_tempered_sampling_vs_float64_restatement(pkg, tau):
    """SAMPLE at tau = 0.25 and 4 with given Exp(1) noise against eval_ref.sample on the engine's logits.  A lane is left
    out only when the restatement's two largest p / q are within 1e-5 relative; at most 1 % (20 of 2048) may be.  On the
    CPU, with the oracle's logits for these inputs (seeds 4300-4302, noise 4320) the restatement leaves out 0 of 2048
    lanes at tau = 0.25 and 0 of 2048 at tau = 4."""
    eng = _rule_engine(pkg)
    q = _exp_noise(4320, (RULE_L, RULE_A))
    a = eng.eval_act("sample", temperature=tau, noise=q).copy()
    want, gap = er.sample(eng.eval_read("logits"), tau, q)
    keep = gap >= er.SAMPLE_GAP
    print(f"tau {tau}: {int((~keep).sum())} of {RULE_L} lanes within {er.SAMPLE_GAP} of a tie")
    assert (~keep).sum() <= RULE_L // 100
    np.testing.assert_array_equal(a[keep], want[keep])
    assert len(np.unique(a)) > 1
    eng.close()


# ------------------------------------------------------------------ 4. the built-in generator
def _builtin_sequence(eng, calls=3):
    out = []
    for _ in range(calls):
        out.append(eng.eval_act("sample", temperature=1.0).copy())
        out.append(eng.eval_act("epsilon", epsilon=0.5).copy())
    return np.stack(out)


def test_builtin_generator_is_keyed_counted_and_restartable(pkg):
    a, b, other = _rule_engine(pkg, seed=7), _rule_engine(pkg, seed=7), _rule_engine(pkg, seed=8)
    sa, sb, so = _builtin_sequence(a), _builtin_sequence(b), _builtin_sequence(other)
    np.testing.assert_array_equal(sa, sb)
    assert (sa != so).any(axis=1).all()  # another seed: every call differs somewhere
    assert (sa[0] != sa[2]).any() and (sa[1] != sa[3]).any()  # the counter advances
    # aleppo_eval_open again: zero stacks, the stream from its start
    a.eval_open(RULE_L)
    assert (a.eval_read("observations") == 0).all()
    a.eval_push_frames(hf.hf_bytes(4301, (RULE_L, 84, 84)), np.ones(RULE_L, np.uint8))
    a.eval_push_frames(hf.hf_bytes(4302, (RULE_L, 84, 84)), np.zeros(RULE_L, np.uint8))
    np.testing.assert_array_equal(_builtin_sequence(a), sa)
    # the documented indexing: call n = 6 is a GREEDY call (it still counts), n = 7 epsilon, n = 8 sample
    b.eval_act("greedy")
    e7 = b.eval_act("epsilon", epsilon=0.5).copy()
    z = b.eval_read("logits")
    np.testing.assert_array_equal(e7, er.epsilon_greedy(z, 0.5, er.eval_noise(7, 7, RULE_L, RULE_A, "epsilon")))
    s8 = b.eval_act("sample", temperature=1.0).copy()
    want, gap = er.sample(z, 1.0, er.eval_noise(7, 8, RULE_L, RULE_A, "sample"))
    keep = gap >= er.SAMPLE_GAP
    assert (~keep).sum() <= RULE_L // 100
    np.testing.assert_array_equal(s8[keep], want[keep])
    for e in (a, b, other):
        e.close()


def test_builtin_epsilon_explores_at_the_binomial_rate(pkg):
    """epsilon = 0.5, L = 4096, A = 4, 8 calls: n = 32768 draws; a draw is non-greedy with probability eps (1 - 1/A) = 0.375,
    so the count has mean 12288 and standard deviation sqrt(32768 * 0.375 * 0.625) = 87.64; 5 sigma = 438.2: [11850, 12726]"""
    eng = _rule_engine(pkg, L=4096, A=4)
    count = 0
    for _ in range(8):
        a = eng.eval_act("epsilon", epsilon=0.5).copy()
        count += int((a != er.greedy(eng.eval_read("logits"))).sum())
    eng.close()
    print("non-greedy actions:", count)
    assert 11850 <= count <= 12726, count


def test_acting_stream_does_not_depend_on_evaluation_calls(pkg):
    got = {}
    for n_eval in (0, 1, 3):
        eng = pkg.Engine(8, 6, 4, 64, precision=pkg.FP32, seed=11)
        eng.load_params(hf.fill_params(4400, 64, 4))
        eng.eval_open(5)
        acts = []
        start = np.ones(8, np.uint8)
        for t in range(6):
            acts.append(eng.act().copy())
            for _ in range(n_eval):
                eng.eval_act("sample", temperature=2.0)
            eng.step(hf.hf_bytes(4401 + t, (8, 84, 84)), np.zeros(8, np.float32), np.zeros(8, np.uint8),
                     np.zeros(8, np.uint8), start)
            start = np.zeros(8, np.uint8)
        got[n_eval] = np.stack(acts)
        eng.close()
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[0], got[3])


# ------------------------------------------------------------------ 5. isolation
ISO_KEYS = ("observations", "actions", "rewards", "masks", "logits", "values", "advantages", "returns", "log_probs",
            "terminals", "truncations", "current_obs", "next_values")


def _scripted_run(pkg, prec, graph, armed, with_eval):
    """2 rollouts of T = 8 (aleppo_act + aleppo_step, or the slot-ahead arm / release loop), finish_rollout, one
    aleppo_train of 2 epochs x 2 minibatches each; with_eval: eval_push_frames + eval_act after every aleppo_act (not in
    the armed loop, where a step is armed then), after every aleppo_step / release_step, after finish_rollout and after
    every aleppo_train (so also between the two aleppo_train calls)"""
    E, T, A, H, L = 8, 8, 6, 64, 5
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=3)
    eng.load_params(hf.fill_params(4500, H, A))
    if graph:
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    if prec == "bf16":
        assert eng.get_option(pkg.OPT_FUSED_ACT) == 1  # fused ingest + acting launch: aleppo_step pre-computes the next act
    n_ev = [0]

    def ev():
        if not with_eval:
            return
        k = n_ev[0]
        n_ev[0] += 1
        if k == 0:
            eng.eval_open(L)
        eng.eval_push_frames(hf.hf_bytes(4600 + k, (L, 84, 84)), (hf.hf_unit(4700 + k, L) < 0.3).astype(np.uint8))
        rule = ("greedy", "sample", "epsilon")[k % 3]
        a = eng.eval_act(rule, temperature=0.5, epsilon=0.3)
        assert a.min() >= 0 and a.max() < A

    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    out = {"acts": [], "batches": [], "metrics": []}
    rng = np.random.default_rng(4501)
    start = np.ones(E, np.uint8)
    for r in range(2):
        for t in range(T):
            out["acts"].append(eng.act().copy())
            if not armed:
                ev()
            fr = hf.hf_bytes(4510 + r * T + t, (E, 84, 84))
            rew = hf.hf_range(4550 + r * T + t, (E,), -2, 2)
            te = ((rng.random(E) < 0.1) & (start == 0)).astype(np.uint8)
            if armed:
                eng.arm_step(fbuf, sbuf)
                ctypes.memmove(fbuf, fr.ctypes.data, E * 7056)
                ctypes.memmove(sbuf, start.ctypes.data, E)
                eng.release_step(rew, te, np.zeros(E, np.uint8))
            else:
                eng.step(fr, rew, te, np.zeros(E, np.uint8), start)
            ev()
            start = te.copy()
        eng.finish_rollout()
        ev()
        out["batches"].append({k: eng.read_batch(k) for k in ISO_KEYS})
        m = eng.train(2.5e-4, 2, 2)
        out["metrics"].append(np.stack([m[k] for k in sorted(m)]))
        ev()
    out["state"] = eng.state_dict()
    if graph:
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) >= 1  # the second update was a replay
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
    return out


@pytest.mark.parametrize("prec,graph,armed", [("bf16", 0, 0), ("fp32", 0, 0), ("bf16", 1, 0), ("fp32", 1, 0),
                                              ("bf16", 0, 1), ("fp32", 0, 1)])
def test_training_run_is_bit_identical_with_evaluation_calls_inserted(pkg, prec, graph, armed):
    plain = _scripted_run(pkg, prec, graph, armed, False)
    mixed = _scripted_run(pkg, prec, graph, armed, True)
    np.testing.assert_array_equal(np.stack(plain["acts"]), np.stack(mixed["acts"]))
    for r in range(2):
        for k in ISO_KEYS:
            np.testing.assert_array_equal(plain["batches"][r][k], mixed["batches"][r][k], err_msg=f"rollout {r}: {k}")
        np.testing.assert_array_equal(plain["metrics"][r], mixed["metrics"][r], err_msg=f"rollout {r}: metrics")
    for k in ("params", "exp_avg", "exp_avg_sq", "step"):
        np.testing.assert_array_equal(plain["state"][k], mixed["state"][k], err_msg=k)


# ------------------------------------------------------------------ 6. errors
def test_refusals_change_nothing(pkg):
    E, T, A, H, L = 8, 4, 4, 64, 6
    lib = pkg.lib()

    def rollout(armed_probe):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, seed=9)
        eng.load_params(hf.fill_params(4800, H, A))
        fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
        if armed_probe:
            eng.eval_open(L)
            eng.eval_push_frames(hf.hf_bytes(4801, (L, 84, 84)), np.ones(L, np.uint8))
            eng.eval_act("greedy")
        start = np.ones(E, np.uint8)
        for t in range(T):
            eng.act()
            eng.arm_step(fbuf, sbuf)
            if armed_probe:  # all four calls are refused while a step is armed
                with pytest.raises(pkg.AleppoError, match="armed"):
                    eng.eval_open(L)
                with pytest.raises(pkg.AleppoError, match="armed"):
                    eng.eval_push_frames(hf.hf_bytes(4802, (L, 84, 84)), np.ones(L, np.uint8))
                with pytest.raises(pkg.AleppoError, match="armed"):
                    eng.eval_act("greedy")
                with pytest.raises(pkg.AleppoError, match="armed"):
                    eng.eval_read("logits")
            fr = hf.hf_bytes(4810 + t, (E, 84, 84))
            ctypes.memmove(fbuf, fr.ctypes.data, E * 7056)
            ctypes.memmove(sbuf, start.ctypes.data, E)
            eng.release_step(hf.hf_range(4820 + t, (E,), -1, 1), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
            start = np.zeros(E, np.uint8)
        eng.finish_rollout()
        b = {k: eng.read_batch(k) for k in ISO_KEYS}
        eng.host_free(fbuf)
        eng.host_free(sbuf)
        eng.close()
        return b

    plain, probed = rollout(False), rollout(True)
    for k in ISO_KEYS:
        np.testing.assert_array_equal(plain[k], probed[k], err_msg=k)

    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=9)
    eng.load_params(hf.fill_params(4800, H, A))
    # before aleppo_eval_open
    with pytest.raises(pkg.AleppoError, match="aleppo_eval_open"):
        eng.eval_push_frames(hf.hf_bytes(1, (L, 84, 84)), np.ones(L, np.uint8))
    with pytest.raises(pkg.AleppoError, match="aleppo_eval_open"):
        eng.eval_act("greedy")
    with pytest.raises(pkg.AleppoError, match="aleppo_eval_open"):
        eng.eval_read("observations")
    for bad in (0, -1, 4097):
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.eval_open(bad)
    eng.eval_open(L)
    with pytest.raises(pkg.AleppoError):
        eng.eval_open(L + 1)
    eng.eval_lanes = L
    for name in ("logits", "values", "actions"):  # nothing to read yet
        with pytest.raises(pkg.AleppoError, match="eval_act"):
            eng.eval_read(name)
    assert (eng.eval_read("observations") == 0).all()
    eng.eval_push_frames(hf.hf_bytes(4830, (L, 84, 84)), np.ones(L, np.uint8))
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng._c(lib.aleppo_eval_push_frames(eng._ctx, None, pkg.FRAMES_84, pkg.HOST, None))
    st = np.ones(L, np.uint8)
    fr = hf.hf_bytes(4830, (L, 84, 84))
    for kind, loc in ((7, pkg.HOST), (pkg.FRAMES_84, 9)):
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng._c(lib.aleppo_eval_push_frames(eng._ctx, fr.ctypes.data_as(ctypes.c_void_p), kind, loc,
                                               st.ctypes.data_as(ctypes.c_void_p)))
    obs0 = eng.eval_read("observations")
    uw = np.stack([hf.hf_unit(4840, L), hf.hf_unit(4841, L)], 1).astype(np.float32)
    first = eng.eval_act("epsilon", epsilon=0.5).copy()  # n = 0
    before = {k: eng.eval_read(k) for k in ("observations", "logits", "values", "actions")}
    nan, inf = float("nan"), float("inf")
    bad_calls = [dict(rule=3), dict(rule=-1), dict(rule="greedy", noise=uw), dict(rule="sample", temperature=0.0),
                 dict(rule="sample", temperature=-1.0), dict(rule="sample", temperature=nan),
                 dict(rule="sample", temperature=inf), dict(rule="epsilon", epsilon=-0.01),
                 dict(rule="epsilon", epsilon=1.01), dict(rule="epsilon", epsilon=nan), dict(rule="epsilon", epsilon=inf)]
    for kw in bad_calls:
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng.eval_act(**kw)
    for rule, param in ((pkg.EVAL_GREEDY, 0.5), (pkg.EVAL_GREEDY, nan)):  # GREEDY's param must be 0
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng._c(lib.aleppo_eval_act(eng._ctx, rule, ctypes.c_float(param), None, None))
    for name, arr in (("observations", np.zeros(3, np.uint8)), ("logits", np.zeros(L * A + 1, np.float32)),
                      ("values", np.zeros(L - 1, np.float32)), ("actions", np.zeros(L, np.int32))):
        with pytest.raises(pkg.AleppoInvalidArgument):
            eng._c(lib.aleppo_eval_read(eng._ctx, pkg.EVAL_FIELDS[name], arr.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.c_size_t(arr.nbytes)))
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng._c(lib.aleppo_eval_read(eng._ctx, 4, before["values"].ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(L * 4)))
    # nothing changed: the fields, and the evaluation counter (the next built-in call is n = 1 of a fresh sequence)
    for k, v in before.items():
        np.testing.assert_array_equal(eng.eval_read(k), v, err_msg=k)
    np.testing.assert_array_equal(obs0, before["observations"])
    second = eng.eval_act("epsilon", epsilon=0.5).copy()
    eng.close()
    ref = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=9)
    ref.load_params(hf.fill_params(4800, H, A))
    ref.eval_open(L)
    ref.eval_push_frames(hf.hf_bytes(4830, (L, 84, 84)), np.ones(L, np.uint8))
    np.testing.assert_array_equal(ref.eval_act("epsilon", epsilon=0.5), first)
    np.testing.assert_array_equal(ref.eval_act("epsilon", epsilon=0.5), second)
    z = ref.eval_read("logits")
    np.testing.assert_array_equal(second, er.epsilon_greedy(z, 0.5, er.eval_noise(9, 1, L, A, "epsilon")))
    ref.close()


# ------------------------------------------------------------------ 7. the trainer
TRAIN = os.path.join(ROOT, "trainer", "train")


@pytest.fixture(scope="module")
def trainer():
    from __graft_entry__ import build
    build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer")])
    return TRAIN


def _crc32c(data):
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    c = 0xFFFFFFFF
    for b in data:
        c = table[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _masked(data):
    c = _crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def read_events(path):
    """yield raw Event payloads, checking both CRCs of every TFRecord (a copy of test_trainer.read_events)"""
    with open(path, "rb") as f:
        while True:
            hdr = f.read(8)
            if not hdr:
                return
            (n,) = struct.unpack("<Q", hdr)
            assert struct.unpack("<I", f.read(4))[0] == _masked(hdr)
            data = f.read(n)
            assert struct.unpack("<I", f.read(4))[0] == _masked(data)
            yield data


def _pb_fields(buf):
    """(field, wire type, value) of one protobuf message (varint / fixed64 / bytes / fixed32)"""
    i = 0
    while i < len(buf):
        key = sh = 0
        while True:
            b = buf[i]
            i += 1
            key |= (b & 127) << sh
            sh += 7
            if b < 128:
                break
        f, w = key >> 3, key & 7
        if w == 0:
            v = sh = 0
            while True:
                b = buf[i]
                i += 1
                v |= (b & 127) << sh
                sh += 7
                if b < 128:
                    break
        elif w == 1:
            v, i = buf[i:i + 8], i + 8
        elif w == 5:
            v, i = buf[i:i + 4], i + 4
        else:
            n = sh = 0
            while True:
                b = buf[i]
                i += 1
                n |= (b & 127) << sh
                sh += 7
                if b < 128:
                    break
            v, i = buf[i:i + n], i + n
        yield f, w, v


def scalars(path):
    """[(tag, step, value bits)] of every simple_value scalar of an event file, in file order"""
    out = []
    for ev in read_events(path):
        step, summ = 0, None
        for f, w, v in _pb_fields(ev):
            if f == 2 and w == 0:
                step = v
            if f == 5 and w == 2:
                summ = v
        if summ is None:
            continue
        for f, w, v in _pb_fields(summ):
            if f == 1 and w == 2:
                tag, val = None, None
                for g, gw, gv in _pb_fields(v):
                    if g == 1 and gw == 2:
                        tag = gv.decode()
                    if g == 2 and gw == 5:
                        val = struct.unpack("<I", gv)[0]
                if tag is not None and val is not None:
                    out.append((tag, step, val))
    return out


@pytest.mark.parametrize("ahead", ["true", "false"])
def test_trainer_evaluates_without_changing_the_training_run(trainer, tmp_path, ahead):
    """debug shape, bf16, eval_interval: 1: the four eval/* scalars once per rollout on the training step axis, eval/episodes =
    eval_episodes; against the same run without the eval_* keys: bit-identical final parameters, the same steps / episodes /
    pending_starts / slots, every training scalar equal bit for bit"""
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read().replace("num_rollouts: 10", "num_rollouts: 3")
    txt = txt.replace("precision: fp32", "precision: bf16") + f"slot_ahead: {ahead}\n"
    keys = "eval_interval: 1\neval_environments: 3\neval_episodes: 4\neval_rule: epsilon\neval_epsilon: 0.05\n"
    out = {}
    for name, extra in (("plain", ""), ("eval", keys)):
        d = tmp_path / name
        os.makedirs(d / "tb")
        cfg = d / "debug.yaml"
        cfg.write_text(txt + extra)
        dump = d / "final.bin"
        r = subprocess.run([trainer, "breakout.bin", str(d / "tb" / "run.log"), str(d), "grp", str(cfg)],
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ALEPPO_TRAINER_DUMP_FINAL=str(dump)))
        assert r.returncode == 0, r.stderr
        mo = re.search(r"steps (\d+) episodes (\d+) pending_starts (\d+) slots (\d+)", r.stdout)
        files = [f for f in os.listdir(d / "tb") if f.startswith("run.tfevents.")]
        assert len(files) == 1
        out[name] = (tuple(map(int, mo.groups())), np.fromfile(dump, np.float32), scalars(str(d / "tb" / files[0])))
    assert out["plain"][0] == out["eval"][0] and out["plain"][0][1] > 0
    np.testing.assert_array_equal(out["plain"][1], out["eval"][1])
    train_scalars = [s for s in out["eval"][2] if not s[0].startswith("eval/")]
    assert train_scalars == out["plain"][2] and len(train_scalars) >= 3 * 8
    assert not [s for s in out["plain"][2] if s[0].startswith("eval/")]
    ev = [s for s in out["eval"][2] if s[0].startswith("eval/")]
    steps = sorted({s[1] for s in train_scalars if s[0] == "learning_rate"})
    assert len(steps) == 3
    for tag in ("eval/episode_return_mean", "eval/episode_return_max", "eval/episode_length_mean", "eval/episodes"):
        mine = [s for s in ev if s[0] == tag]
        assert [s[1] for s in mine] == steps, tag
        vals = [struct.unpack("<f", struct.pack("<I", s[2]))[0] for s in mine]
        assert np.isfinite(vals).all()
        if tag == "eval/episodes":
            assert vals == [4.0, 4.0, 4.0]
        if tag == "eval/episode_length_mean":
            assert all(v >= 1 for v in vals)
