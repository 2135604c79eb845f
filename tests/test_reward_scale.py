"""ALEPPO_OPT_REWARD_SCALE (include/aleppo.h): return-based reward scaling in place of the reward clamp.  CPU: the
definition of tests/reward_scale_ref.py against a literal per-step gym-style loop, hand-written cases, the device's
summation order inside the derived bounds, the input generator's own conditions, the header against the Python mirror.
GPU: everything through the C ABI - running state and rewards against the reference, GAE on the scaled rewards against the
oracle, determinism, option off, the three record routes, checkpoint, composition, communicator, the stateless operator
and the errors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hashfill as hf
import oracle_lib as orc
import reward_scale_ref as rr
from trainer_helpers import header_const as const
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.99
SHAPES = [(128, 128), (4096, 5), (257, 19)]  # (the last: E % 64 and T % 16 ragged)
PLANES = ("rewards", "values", "next_values", "terminals", "truncations", "masks", "advantages", "returns", "log_probs",
          "actions")


def _trace(seed, E, T, K):
    """K consecutive rollouts of the generator, the start flags carried from one to the next"""
    out, start = [], None
    for k in range(K):
        r, te, tr, st, start = rr.generate(seed + 17 * k, E, T, start)
        out.append((r, te, tr, st))
    return out


# ------------------------------------------------------------------ CPU
class _GymRunningMeanStd:
    """gym.wrappers.normalize.RunningMeanStd / SB3's, restated"""

    def __init__(self):
        self.mean, self.var, self.count = 0.0, 1.0, 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        if x.size == 0:  # (gym never updates with an empty batch; a slot where every environment starts has none)
            return
        bm, bv, bc = float(np.mean(x)), float(np.var(x)), x.size
        delta = bm - self.mean
        tot = self.count + bc
        new_mean = self.mean + delta * bc / tot
        m2 = self.var * self.count + bv * bc + delta * delta * self.count * bc / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


@pytest.mark.parametrize("E,T", [(128, 128), (4096, 5), (8, 8), (257, 19)])
def test_batched_merge_equals_the_per_step_gym_loop(E, T):
    """RunningMeanStd.update after every slot (gym's NormalizeReward) gives the state the per-rollout merge gives"""
    g = float(np.float32(GAMMA))
    ref = rr.Reference(E, GAMMA)
    rms, G = _GymRunningMeanStd(), np.zeros(E)
    for k, (r, te, tr, st) in enumerate(_trace(100 + E, E, T, 5)):
        ref.rollout(r, te, tr, st)
        for t in range(T):
            live = st[t] == 0
            G = np.where(live, G * g + r[t].astype(np.float64), G)
            rms.update(G[live])
            G = np.where(live & ((te[t] | tr[t]) != 0), 0.0, G)
        count, mean, var = ref.state
        print(E, T, k, "batched", ref.state, "per step", (rms.count, rms.mean, rms.var))
        assert abs(count - rms.count) <= 1e-12 * count
        assert abs(mean - rms.mean) <= 1e-12 * max(abs(mean), np.sqrt(var))
        assert abs(var - rms.var) <= 1e-12 * var
        np.testing.assert_array_equal(G, ref.G)


def test_hand_written_cases():
    g = float(np.float32(GAMMA))
    z = np.zeros((4, 1), np.uint8)
    # a terminal resets G after its own sample
    te = z.copy()
    te[1] = 1
    x, live, G = rr.scan(np.array([[1], [2], [3], [4]], np.float32), te, z, z, np.array([10.0]), GAMMA)
    assert live.all()
    np.testing.assert_array_equal(x[:, 0], [10 * g + 1, (10 * g + 1) * g + 2, 3.0, 3 * g + 4])
    assert G[0] == 3 * g + 4
    # a truncation resets too; at the last slot G leaves the rollout as 0
    tr = z.copy()
    tr[3] = 1
    _, _, G = rr.scan(np.ones((4, 1), np.float32), z, tr, z, np.zeros(1), GAMMA)
    assert G[0] == 0.0
    # a start slot is skipped: no sample, G untouched, its (stale) reward never enters
    st = z.copy()
    st[2] = 1
    x, live, G = rr.scan(np.array([[1], [2], [1000], [4]], np.float32), z, z, st, np.array([0.0]), GAMMA)
    assert live[:, 0].tolist() == [True, True, False, True]
    np.testing.assert_array_equal(x[live], [1.0, g + 2, (g + 2) * g + 4])
    # n = 0 (every slot a start slot) leaves the state alone
    ref = rr.Reference(3, GAMMA, state=(5.0, 0.25, 2.0), G=[1.0, 2.0, 3.0])
    xs = ref.rollout(np.ones((2, 3), np.float32), np.zeros((2, 3)), np.zeros((2, 3)), np.ones((2, 3)))
    assert xs.size == 0 and ref.state == (5.0, 0.25, 2.0) and ref.G.tolist() == [1.0, 2.0, 3.0] and ref.n == 0
    assert ref.scale == np.float32(1 / np.sqrt(2.0 + 1e-8))
    # the first merge from the initial state: count 1e-4 weighs next to nothing
    ref = rr.Reference(1, GAMMA)
    ref.rollout(np.array([[2], [2]], np.float32) * 0 + np.array([[1], [3]], np.float32), z[:2], z[:2], z[:2])
    xs = np.array([1.0, g + 3])
    assert ref.state[0] == 1e-4 + 2 and abs(ref.state[1] - xs.mean()) < 1e-3 and ref.state[2] > 0
    # step 5: multiply, then clip; the count is of |r * s| > c
    out, n = rr.scaled_rewards(np.array([[0, 1, -8, 40, -40, 6]], np.float32), np.float32(0.5), 3.0)
    assert out.tolist() == [[0, 0.5, -3, 3, -3, 3]] and n == 3 and out.dtype == np.float32


@pytest.mark.parametrize("E,T", SHAPES)
def test_generator_conditions_and_the_device_order_inside_the_bounds(E, T):
    """every generated rollout has a terminal, a truncation and a start slot; the reference clips more than none and fewer
    than 1 % of the rewards at c = CLIP (and none of the ordinary 1-4 rewards); the device's summation order, restated,
    stays far inside the derived bounds, which are themselves small"""
    ref = rr.Reference(E, GAMMA)
    dev_state = rr.INITIAL
    G = np.zeros(E)
    for k, (r, te, tr, st) in enumerate(_trace(200 + E, E, T, 4)):
        assert te.any() and tr.any() and st.any(), (E, T, k)
        assert not ((te + tr + st) > 1).any()
        x, live, G = rr.scan(r, te, tr, st, G, GAMMA)
        ref.rollout(r, te, tr, st)
        dev_state, dev_s = rr.state_from_sums(dev_state, *rr.one_pass_in_device_order(x, live))
        scaled, nclip = ref.scaled(r, rr.CLIP)
        share = nclip / r.size
        small = np.abs(r) <= 4
        print(E, T, k, "state", ref.state, "scale", ref.scale, "share", share, "bounds", ref.bm, ref.bv, "rel_b", ref.rel_b)
        assert 0 < nclip and share < 0.01, (E, T, k, share)
        assert (np.abs(r[small] * ref.scale) < rr.CLIP).all()  # only the rare large rewards reach the clip
        assert (scaled == rr.CLIP).any() and (scaled == -rr.CLIP).any()
        assert ref.rel_b < 1e-9
        rr.assert_state(dict(count=dev_state[0], mean=dev_state[1], var=dev_state[2], scale=float(dev_s),
                             batch_count=ref.n), ref, f"device order {E}x{T} #{k}")
        assert abs(dev_state[2] - ref.state[2]) <= 0.05 * ref.bv  # (the bound is a worst case: a fraction of it is used)
    np.testing.assert_array_equal(G, ref.G)


def test_header_constants_and_python_mirror():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()

    assert const("ALEPPO_OPT_REWARD_SCALE") == pkg.OPT_REWARD_SCALE == 23
    assert const("ALEPPO_OPT_REWARD_SCALE_CLIP") == pkg.OPT_REWARD_SCALE_CLIP == 24
    assert const("ALEPPO_F_REWARD_SCALE") == pkg.FIELDS["reward_scale"] == 14
    m = re.search(r"(?m)^#define ALEPPO_REWARD_SCALE_COUNT (\d+)", hdr)
    assert m and int(m.group(1)) == pkg.REWARD_SCALE_COUNT == 6 == len(rr.NAMES)
    for i, name in enumerate(rr.NAMES):
        assert const("ALEPPO_RS_" + name.upper()) == pkg.REWARD_SCALE[name] == i
    for fn in ("set_reward_scaling", "reward_scale", "reward_scale_state", "load_reward_scale_state"):
        assert hasattr(pkg.Engine, fn), fn
    assert callable(pkg._reward_scale)
    for sym in ("aleppo_export_reward_scale", "aleppo_import_reward_scale", "aleppo_reward_scale"):
        assert sym in pkg.EXPORTS and hasattr(pkg.lib(), sym)
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


# ------------------------------------------------------------------ GPU
class _DeviceBytes:
    """device copy of a numpy array (no torch in the test process)"""

    def __init__(self, arr):
        self.hip = ctypes.CDLL("libamdhip64.so")
        arr = np.ascontiguousarray(arr)
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(arr.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes), 1) == 0

    @property
    def addr(self):
        return self.ptr.value

    def free(self):
        self.hip.hipFree(self.ptr)


def _frames(seed, E, T):
    eb = min(E, 32)
    base = hf.hf_bytes(seed, (T, eb, 84, 84))
    return np.concatenate([base ^ np.uint8(37 * k % 256) for k in range((E + eb - 1) // eb)], axis=1)[:, :E]


def _engine(pkg, E, T, seed, prec=None, A=4, H=32, **kw):
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec is None else prec, seed=3, gamma=GAMMA, **kw)
    eng.load_params(hf.fill_params(seed, H, A))
    return eng


def _read(eng, keys=PLANES):
    b = {k: eng.read_batch(k) for k in keys}
    b["state"] = eng.read_batch("reward_scale")
    return b


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _replay(eng, dev, rec, pkg):
    r, te, tr, st = rec
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, eng.E * 7056, r, te, tr, st)
    eng.finish_rollout()


def _check_rollout(eng, b, ref, rec, what, rt16=False):
    """state within the bounds, rewards exact from the engine's own s, GAE bit-exact from the engine's own rewards"""
    r, te, tr, st = rec
    ref.rollout(r, te, tr, st)
    got = dict(zip(rr.NAMES, b["state"]))
    rr.assert_state(got, ref, what)
    want, nclip = rr.scaled_rewards(r.T, np.float32(got["scale"]), rr.CLIP)  # env-major [E,T]
    np.testing.assert_array_equal(b["rewards"], want, err_msg=what)
    assert got["clipped"] == nclip, (what, got["clipped"], nclip)
    np.testing.assert_array_equal(b["terminals"], te.T)
    np.testing.assert_array_equal(b["masks"], 1 - st.T)
    adv = orc.gae(b["rewards"], b["values"], b["next_values"], te.T, tr.T, st.T, gamma=GAMMA, lam=0.95)
    ret = adv + b["values"]
    if rt16:  # the planes are rounded to half when stored; the recursion keeps fp32
        adv, ret = (x.astype(np.float16).astype(np.float32) for x in (adv, ret))
    np.testing.assert_array_equal(b["advantages"], adv, err_msg=what)
    np.testing.assert_array_equal(b["returns"], ret, err_msg=what)


STATE_CASES = [(E, T, prec, planes) for E, T in SHAPES for prec, planes in (("fp32", "fp32"), ("bf16", "fp16"))] + \
    [(257, 19, "bf16", "fp32"), (257, 19, "fp32", "fp16")]


@pytest.mark.gpu
@pytest.mark.parametrize("E,T,prec,planes", STATE_CASES)
def test_running_state_rewards_and_gae(pkg, E, T, prec, planes):
    K = 3
    trace = _trace(200 + E, E, T, K)  # (the traces whose conditions the CPU test above asserts)
    rt16 = planes == "fp16"
    eng = _engine(pkg, E, T, 310, prec=pkg.BF16 if prec == "bf16" else pkg.FP32,
                  rollout_precision=pkg.ROLLOUT_FP16 if rt16 else pkg.ROLLOUT_FP32)
    first = dict(zip(rr.NAMES, eng.read_batch("reward_scale")))
    assert first == dict(count=1e-4, mean=0.0, var=1.0, scale=1.0, batch_count=0.0, clipped=0.0)
    eng.set_reward_scaling(True, clip=rr.CLIP)
    assert eng.get_option(pkg.OPT_REWARD_SCALE) == 1
    assert pkg.bits_float(eng.get_option(pkg.OPT_REWARD_SCALE_CLIP)) == rr.CLIP
    dev = _DeviceBytes(_frames(320, E, T))
    ref = rr.Reference(E, GAMMA)
    for k in range(K):
        _replay(eng, dev, trace[k], pkg)
        b = _read(eng)
        _check_rollout(eng, b, ref, trace[k], f"{E}x{T} {prec}/{planes} #{k}", rt16)
        assert 0 < b["state"][5] < 0.01 * E * T  # both branches of the clip, and the clip is not the whole test
    np.testing.assert_array_equal(eng.reward_scale_state()["returns"], ref.G)  # the running returns are the reference's bits
    dev.free()
    eng.close()


@pytest.mark.gpu
def test_default_clip_is_ten_and_ordinary_rewards_keep_their_ratios(pkg):
    """the trainer's own rewards (1 or 4 per brick) stay 1 : 4 after scaling, where the clamp makes them equal"""
    E, T = 64, 32
    r, te, tr, st, _ = rr.generate(330, E, T)
    r = np.where(np.abs(r) > 4, 0, r).astype(np.float32)
    dev = _DeviceBytes(_frames(331, E, T))
    eng = _engine(pkg, E, T, 332)
    assert pkg.bits_float(eng.get_option(pkg.OPT_REWARD_SCALE_CLIP)) == 10.0
    eng.set_option(pkg.OPT_REWARD_SCALE, 1)
    _replay(eng, dev, (r, te, tr, st), pkg)
    got, s = eng.read_batch("rewards"), np.float32(eng.reward_scale()["scale"])
    np.testing.assert_array_equal(got, r.T * s)
    assert eng.reward_scale()["clipped"] == 0 and (r == 4).any() and (r == 1).any()
    eng.set_option(pkg.OPT_REWARD_SCALE, 0)
    _replay(eng, dev, (r, te, tr, st), pkg)
    np.testing.assert_array_equal(eng.read_batch("rewards"), np.clip(r.T, -1, 1))
    dev.free()
    eng.close()


@pytest.mark.gpu
def test_two_contexts_give_identical_bits(pkg):
    E, T = 257, 19
    trace = _trace(340, E, T, 2)
    dev = _DeviceBytes(_frames(341, E, T))
    outs = []
    for _ in range(2):
        eng = _engine(pkg, E, T, 342, prec=pkg.BF16)
        eng.set_reward_scaling(True, clip=rr.CLIP)
        per = []
        for rec in trace:
            _replay(eng, dev, rec, pkg)
            per.append(_read(eng))
        per.append(dict(g=eng.reward_scale_state()["returns"]))
        outs.append(per)
        eng.close()
    dev.free()
    for a, b in zip(*outs):
        _same(a, b, "two contexts")


@pytest.mark.gpu
def test_option_off_is_the_old_behaviour(pkg):
    """never touched == set to 0 == on for one rollout and off again, in every plane of the next rollout; with the option
    off the state stops changing"""
    E, T = 96, 24
    trace = _trace(350, E, T, 3)
    dev = _DeviceBytes(_frames(351, E, T))

    def run(mode):
        eng = _engine(pkg, E, T, 352)
        if mode == "zero":
            eng.set_option(pkg.OPT_REWARD_SCALE, 0)
        if mode == "on_off":
            eng.set_reward_scaling(True, clip=rr.CLIP)
        _replay(eng, dev, trace[0], pkg)
        state0 = eng.read_batch("reward_scale")
        if mode == "on_off":
            eng.set_option(pkg.OPT_REWARD_SCALE, 0)
        out = []
        for rec in trace[1:]:
            _replay(eng, dev, rec, pkg)
            out.append(_read(eng))
        eng.close()
        return state0, out

    s_never, never = run("never")
    s_zero, zero = run("zero")
    s_onoff, onoff = run("on_off")
    assert s_never.tolist() == s_zero.tolist() == [1e-4, 0.0, 1.0, 1.0, 0.0, 0.0]
    assert s_onoff[0] > 1 and s_onoff[4] > 0
    for k in range(2):
        np.testing.assert_array_equal(never[k]["rewards"], np.clip(trace[k + 1][0].T, -1, 1))  # the reference's clamp
        for key in PLANES:
            assert never[k][key].tobytes() == zero[k][key].tobytes() == onoff[k][key].tobytes(), key
        assert never[k]["state"].tobytes() == s_never.tobytes()
        assert onoff[k]["state"].tobytes() == s_onoff.tobytes()  # kept, not updated
    dev.free()


@pytest.mark.gpu
def test_the_three_record_routes_give_the_same_bits(pkg):
    E, T, K = 40, 19, 2
    trace = _trace(360, E, T, K)
    frames = _frames(361, E, T)
    dev = _DeviceBytes(frames)

    def run(route):
        eng = _engine(pkg, E, T, 362, prec=pkg.BF16)
        eng.set_reward_scaling(True, clip=rr.CLIP)
        fbuf = sbuf = None
        if route == "arm":
            fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
        out = []
        for r, te, tr, st in trace:
            if route == "replay":
                eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, r, te, tr, st)
            for t in range(T if route != "replay" else 0):
                eng.act()
                if route == "step":
                    eng.step(frames[t], r[t], te[t], tr[t], st[t])
                elif route == "record":
                    eng.push_frames(frames[t], st[t])
                    eng.record_step(r[t], te[t], tr[t], st[t])
                else:
                    eng.arm_step(fbuf, sbuf)
                    ctypes.memmove(fbuf, frames[t].ctypes.data, E * 7056)
                    ctypes.memmove(sbuf, st[t].ctypes.data, E)
                    eng.release_step(r[t], te[t], tr[t])
            eng.finish_rollout()
            out.append(_read(eng))
        if fbuf:
            eng.host_free(fbuf)
            eng.host_free(sbuf)
        eng.close()
        return out

    base = run("replay")
    ref = rr.Reference(E, GAMMA)
    for k in range(K):
        _check_rollout(None, base[k], ref, trace[k], f"replay #{k}")
    for route in ("step", "record", "arm"):
        other = run(route)
        for k in range(K):
            _same(base[k], other[k], route)
    dev.free()


@pytest.mark.gpu
def test_checkpoint_with_parameters_after_train(pkg):
    """export after rollout k, import into a fresh context together with parameters and optimiser, and continue: state,
    planes and - after aleppo_train - parameters equal the uninterrupted run bit for bit.  (Explicit sampling noise: the acting
    generator's counter is not part of a checkpoint.)"""
    E, T, H = 32, 16, 64
    trace = _trace(380, E, T, 3)
    dev = _DeviceBytes(_frames(381, E, T))

    def run(resume_at):
        eng = _engine(pkg, E, T, 382, H=H)
        assert "reward_scale" not in eng.state_dict()  # only while the option is on
        eng.set_reward_scaling(True, clip=rr.CLIP)
        out = []
        for k in range(3):
            if k == resume_at:
                sd = eng.state_dict()
                assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step", "reward_scale"}
                eng.close()
                eng = _engine(pkg, E, T, 382, H=H)
                eng.set_reward_scaling(True, clip=rr.CLIP)
                # (slot 0 is acted on the observation the previous rollout left behind - the emulator's part of a
                # resume.  Replaying that rollout restores it; what it does to the learner is overwritten next.)
                eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, *trace[k - 1])
                eng.finish_rollout()
                eng.load_state_dict(sd)
                np.testing.assert_array_equal(eng.read_batch("reward_scale")[:3], sd["reward_scale"]["stats"])
            noise =hf.hf_range(390 + k, (T, E, 4), 0.05, 3.0)  # explicit sampling noise: no generator state to carry
            r, te, tr, st = trace[k]
            eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, r, te, tr, st, noise=noise)
            eng.finish_rollout(hf.hf_range(395 + k, (E, 4), 0.05, 3.0))
            out.append(_read(eng))
            eng.train(2.5e-4, 1, 2)
            out.append(dict(params=eng.export_params()))
        out.append(dict(g=eng.reward_scale_state()["returns"]))
        eng.close()
        return out

    whole, resumed = run(None), run(2)
    for a, b in zip(whole, resumed):
        _same(a, b, "resumed")
    dev.free()


@pytest.mark.gpu
def test_composition_with_advantage_norm_batch_stats_and_evaluation(pkg):
    import batch_stats_ref as br
    E, T, L = 64, 24, 5
    trace = _trace(400, E, T, 2)
    dev = _DeviceBytes(_frames(401, E, T))

    def run(advantage_norm, with_eval):
        eng = _engine(pkg, E, T, 402, advantage_norm=advantage_norm)
        eng.set_reward_scaling(True, clip=rr.CLIP)
        out = []
        if with_eval:
            eng.eval_open(L)
        for rec in trace:
            if with_eval:
                eng.eval_push_frames(hf.hf_bytes(403, (L, 84, 84)), np.ones(L, np.uint8))
                eng.eval_act("greedy")
            _replay(eng, dev, rec, pkg)
            if with_eval:
                eng.eval_act("epsilon", epsilon=0.3)
            b = _read(eng)
            b["bstats"] = eng.read_batch("batch_stats")
            out.append(b)
        eng.close()
        return out

    plain, normed, evald = run(False, False), run(True, False), run(False, True)
    ref = rr.Reference(E, GAMMA)
    for k in range(2):
        _check_rollout(None, plain[k], ref, trace[k], f"plain #{k}")
        _same(plain[k], evald[k], "evaluation lanes interleaved")  # the lanes and the scaling do not see each other
        for key in ("rewards", "returns", "masks", "state", "values"):
            assert plain[k][key].tobytes() == normed[k][key].tobytes(), key
        want = orc.adv_norm(plain[k]["advantages"], plain[k]["masks"])
        np.testing.assert_allclose(normed[k]["advantages"], want, rtol=1e-4, atol=1e-5)
        b = plain[k]
        stats, bounds = br.reference(b["values"], b["returns"], b["advantages"], b["masks"])
        br.assert_close(dict(zip(br.NAMES, b["bstats"])), stats, bounds, f"batch stats on a scaled rollout #{k}")


@pytest.mark.gpu
def test_fp32_train_on_a_scaled_rollout_against_the_oracle(pkg):
    E, T, A, H, M = 16, 8, 4, 64, 2
    r, te, tr, st, _ = rr.generate(410, E, T)
    params = hf.fill_params(411, H, A)
    dev = _DeviceBytes(_frames(412, E, T))
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=3, gamma=GAMMA)
    eng.load_params(params)
    eng.set_reward_scaling(True, clip=rr.CLIP)
    _replay(eng, dev, (r, te, tr, st), pkg)
    dev.free()
    b = {k: eng.read_batch(k) for k in ("observations", "actions", "log_probs", "advantages", "returns", "masks", "rewards")}
    assert np.abs(b["rewards"]).max() > 1.0  # (beyond the clamp's range: this batch exists only with the option)
    N = E * T
    m = eng.train(2.5e-4, 2, M)
    w = orc.train(params, H, A, b["observations"].reshape(N, 4, 84, 84), b["actions"].ravel(),
                  b["log_probs"].reshape(N, A), b["advantages"].ravel(), b["returns"].ravel(), b["masks"].ravel(), 2, M)
    print("loss", m["loss"].ravel(), w["loss"].ravel(), "params max err", np.abs(eng.export_params() - w["params"]).max())
    np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=1e-3)
    np.testing.assert_allclose(eng.export_params(), w["params"], atol=1e-4)
    eng.close()


@pytest.mark.gpu
def test_one_rank_communicator_is_bit_identical(pkg):
    E, T = 257, 19
    trace = _trace(420, E, T, 2)
    dev = _DeviceBytes(_frames(421, E, T))

    def run(comm):
        eng = _engine(pkg, E, T, 422)
        if comm:
            eng.comm_init(pkg.Engine.comm_unique_id())
            eng.set_option(pkg.OPT_FORCE_COMM, 1)
        eng.set_reward_scaling(True, clip=rr.CLIP)
        out = []
        for rec in trace:
            _replay(eng, dev, rec, pkg)
            out.append(_read(eng))
        eng.close()
        return out

    for a, b in zip(run(False), run(True)):
        _same(a, b, "1-rank communicator")
    dev.free()


_DP_SCRIPT = r'''
import os, sys, ctypes, time
root, rank, idfile, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import hashfill as hf, reward_scale_ref as rr
from __graft_entry__ import load_package
pkg = load_package()
WORLD, EG, T, H, A, K = 2, 96, 19, 32, 4, 3
if rank == 0:
    open(idfile + ".tmp", "wb").write(pkg.Engine.comm_unique_id()); os.replace(idfile + ".tmp", idfile)
t0 = time.time()
while not os.path.exists(idfile):
    assert time.time() - t0 < 120
    time.sleep(0.05)
uid = open(idfile, "rb").read()
eng = pkg.Engine(EG, T, A, H, precision=pkg.FP32, device=rank, world_size=WORLD, rank=rank, gamma=0.99)
eng.comm_init(uid)
eng.load_params(hf.fill_params(431, H, A))
eng.set_reward_scaling(True, clip=rr.CLIP)
cols = slice(rank * EG, (rank + 1) * EG)
start, states = None, []
frames = hf.hf_bytes(432, (EG, 84, 84))
for k in range(K):
    r, te, tr, st, start = rr.generate(430 + 17 * k, WORLD * EG, T, start)
    for t in range(T):
        eng.act()
        eng.step(frames, r[t, cols], te[t, cols], tr[t, cols], st[t, cols])
    eng.finish_rollout()
    states.append(eng.read_batch("reward_scale"))
np.save(os.path.join(outdir, f"states{rank}.npy"), np.array(states))
eng.close()
print("DP_RANK_OK", rank)
'''


def _gpu_count():
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


@pytest.mark.gpu
def test_two_ranks_hold_the_state_of_the_concatenated_environments(tmp_path):
    """Two processes, one GPU each, real RCCL: both ranks hold bit-identical (count, mean, var, s), equal to the reference
    on the concatenated environments within the bounds.  Skips on a one-GPU box."""
    if _gpu_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    script = tmp_path / "dp_rank.py"
    script.write_text(_DP_SCRIPT)
    idfile = str(tmp_path / "nccl_id.bin")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), idfile, str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=420)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"DP_RANK_OK {r}" in o, o[-4000:]
    s0, s1 = np.load(tmp_path / "states0.npy"), np.load(tmp_path / "states1.npy")
    assert s0[:, :5].tobytes() == s1[:, :5].tobytes()  # (index 5, the clip count, is per rank)
    ref, start = rr.Reference(2 * 96, GAMMA), None
    for k in range(3):
        r, te, tr, st, start = rr.generate(430 + 17 * k, 2 * 96, 19, start)
        ref.rollout(r, te, tr, st)
        got = dict(zip(rr.NAMES, s0[k]))
        rr.assert_state(got, ref, f"two ranks #{k}")
        _, nclip = rr.scaled_rewards(r, np.float32(got["scale"]), rr.CLIP)
        assert s0[k][5] + s1[k][5] == nclip


@pytest.mark.gpu
def test_stateless_operator_equals_the_engine(pkg):
    E, T = 257, 19
    trace = _trace(440, E, T, 3)
    dev = _DeviceBytes(_frames(441, E, T))
    eng = _engine(pkg, E, T, 442)
    eng.set_reward_scaling(True, clip=rr.CLIP)
    stats, G = np.array(rr.INITIAL), np.zeros(E)
    for k, (r, te, tr, st) in enumerate(trace):
        _replay(eng, dev, (r, te, tr, st), pkg)
        scaled, stats, G, s, clipped = pkg.rewards.scale(r.T, te.T, tr.T, st.T, GAMMA, rr.CLIP, stats, G)
        e = dict(zip(rr.NAMES, eng.read_batch("reward_scale")))
        assert [e["count"], e["mean"], e["var"]] == stats.tolist(), k
        assert e["scale"] == float(s) and e["clipped"] == clipped and clipped > 0
        assert eng.read_batch("rewards").tobytes() == scaled.tobytes()
        assert eng.reward_scale_state()["returns"].tobytes() == G.tobytes()
    dev.free()
    eng.close()
    # validation, as aleppo_gae's: shapes, overlapping flags; and the state's own
    r, te, tr, st = (a.T.copy() for a in trace[0])
    with pytest.raises(pkg.AleppoInvalidArgument, match="2D"):
        pkg.rewards.scale(r[0], te[0], tr[0], st[0], GAMMA, 10.0, rr.INITIAL, np.zeros(E))
    with pytest.raises(pkg.AleppoInvalidArgument, match="compatible dimensions"):
        pkg.rewards.scale(r, te[:, :5], tr, st, GAMMA, 10.0, rr.INITIAL, np.zeros(E))
    with pytest.raises(pkg.AleppoInvalidArgument, match="compatible dimensions"):
        pkg.rewards.scale(r, te, tr, st, GAMMA, 10.0, rr.INITIAL, np.zeros(E + 1))
    bad = te.copy()
    bad[3, 4] = 1
    st2 = st.copy()
    st2[3, 4] = 1
    with pytest.raises(pkg.AleppoInvalidArgument, match="mutually exclusive"):
        pkg.rewards.scale(r, bad, tr, st2, GAMMA, 10.0, rr.INITIAL, np.zeros(E))
    for clip in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(pkg.AleppoInvalidArgument, match="clip"):
            pkg.rewards.scale(r, te, tr, st, GAMMA, clip, rr.INITIAL, np.zeros(E))
    for stats in ((0.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 0.0, -1.0)):
        with pytest.raises(pkg.AleppoInvalidArgument, match="count"):
            pkg.rewards.scale(r, te, tr, st, GAMMA, 10.0, stats, np.zeros(E))


@pytest.mark.gpu
def test_errors(pkg):
    E, T, A, H = 8, 4, 4, 32
    lib = pkg.lib()
    eng = _engine(pkg, E, T, 450)
    # invalid option values leave the old value in place
    eng.set_reward_scaling(True, clip=2.5)
    for v in (2, -1, 7):
        with pytest.raises(pkg.AleppoInvalidArgument, match="ALEPPO_OPT_REWARD_SCALE"):
            eng.set_option(pkg.OPT_REWARD_SCALE, v)
    assert eng.get_option(pkg.OPT_REWARD_SCALE) == 1
    for x in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(pkg.AleppoInvalidArgument, match="ALEPPO_OPT_REWARD_SCALE_CLIP"):
            eng.set_option(pkg.OPT_REWARD_SCALE_CLIP, pkg.float_bits(x))
    assert pkg.bits_float(eng.get_option(pkg.OPT_REWARD_SCALE_CLIP)) == 2.5
    # wrong byte count
    buf = np.zeros(8, np.float64)
    for nbytes in (40, 56, 0):
        assert lib.aleppo_read_batch(eng._ctx, pkg.FIELDS["reward_scale"], buf.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_size_t(nbytes)) == pkg.ERR_INVALID_ARGUMENT
    # wrong num_envs, invalid imported state: refused, nothing changes
    good = eng.reward_scale_state()
    stats, g = good["stats"].copy(), good["returns"].copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for n in (E - 1, E + 1, 0):
        assert lib.aleppo_export_reward_scale(eng._ctx, p(stats), p(g), ctypes.c_size_t(n)) == pkg.ERR_INVALID_ARGUMENT
        assert lib.aleppo_import_reward_scale(eng._ctx, p(stats), p(g), ctypes.c_size_t(n)) == pkg.ERR_INVALID_ARGUMENT
    for bad in ((0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, -1e-9), (float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0),
                (1.0, 0.0, float("inf"))):
        with pytest.raises(pkg.AleppoInvalidArgument, match="import_reward_scale"):
            eng.load_reward_scale_state(dict(stats=np.array(bad), returns=g))
    gbad = g.copy()
    gbad[3] = float("nan")
    with pytest.raises(pkg.AleppoInvalidArgument, match="not finite"):
        eng.load_reward_scale_state(dict(stats=stats, returns=gbad))
    after = eng.reward_scale_state()
    assert after["stats"].tobytes() == good["stats"].tobytes() and after["returns"].tobytes() == good["returns"].tobytes()
    eng.load_reward_scale_state(dict(stats=np.array([7.0, 0.5, 4.0]), returns=np.arange(E, dtype=np.float64)))
    assert eng.read_batch("reward_scale")[:3].tolist() == [7.0, 0.5, 4.0]
    assert eng.reward_scale_state()["returns"].tolist() == list(range(E))
    # a rollout whose flags overlap is refused and leaves the state as it was
    before = eng.read_batch("reward_scale"), eng.reward_scale_state()["returns"]
    for t in range(T):
        eng.act()
        both = np.zeros(E, np.uint8)
        both[2] = t == 1
        eng.step(hf.hf_bytes(451 + t, (E, 84, 84)), np.ones(E, np.float32), both, both, np.zeros(E, np.uint8))
    with pytest.raises(pkg.AleppoInvalidArgument, match="mutually exclusive"):
        eng.finish_rollout()
    assert eng.read_batch("reward_scale").tobytes() == before[0].tobytes()
    assert eng.reward_scale_state()["returns"].tobytes() == before[1].tobytes()
    # every new call while a step is armed is ALEPPO_ERR_RUNTIME
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    for call in (lambda: eng.set_option(pkg.OPT_REWARD_SCALE, 0),
                 lambda: eng.set_option(pkg.OPT_REWARD_SCALE_CLIP, pkg.float_bits(1.0)),
                 lambda: eng.get_option(pkg.OPT_REWARD_SCALE), lambda: eng.read_batch("reward_scale"),
                 lambda: eng.reward_scale_state(), lambda: eng.load_reward_scale_state(good)):
        with pytest.raises(pkg.AleppoError, match="armed"):
            call()
    ctypes.memmove(fbuf, hf.hf_bytes(460, (E, 84, 84)).ctypes.data, E * 7056)
    ctypes.memmove(sbuf, np.ones(E, np.uint8).ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    assert eng.get_option(pkg.OPT_REWARD_SCALE) == 1
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
