"""Parity of the PRODUCTION kernels at the sizes the bench runs them (pytest -m gpu, on the MI355X).

tests/test_gpu_parity.py pins every operator against the reference's golden vectors at fixture sizes; here the same
C-ABI path is checked against the pinned CPU oracle at BASELINE configs[1] size (128 envs x T = 128, 4096-sample
minibatches, H = 512, bf16) and on the GAE kernel's chunked scan, i.e. the code paths that only engage at size:
static-atom loops, the register-tiled conv3 dgrad, XCD job maps, the 1-D swizzled fc wgrad launch, the pipelined fc
GEMMs, 16-step GAE chunks with both register sets.

Bounds.  Integer / byte / index planes and the GAE planes (same fp32 op order): bit-exact.  fp32 network outputs:
1e-4 (north star).  bf16 operands (8-bit mantissa) with fp32 accumulation: the documented looser bounds are written
next to each assert; they were set from measured errors on MI355X with ~2x margin.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DeviceBytes:
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


def _flags(seed, T, E, p_term=0.08, p_trunc=0.04):
    """slot protocol of SURVEY app. A: a terminated / truncated slot is followed by one episode-start slot"""
    rng = np.random.default_rng(seed)
    te = np.zeros((T, E), np.uint8)
    tr = np.zeros((T, E), np.uint8)
    st = np.zeros((T, E), np.uint8)
    start = np.ones(E, np.uint8)
    for t in range(T):
        u = rng.random(E)
        st[t] = start
        te[t] = ((u < p_term) & (start == 0))
        tr[t] = ((u >= p_term) & (u < p_term + p_trunc) & (start == 0))
        start = (te[t] | tr[t]).astype(np.uint8)
    return te, tr, st


def _rollout_vs_oracle(b, frames84, st, rew, te, tr, obs0, params, H, A, tol, noise=None, checker=None):
    """One rollout's read-back planes `b` (read_batch dict) against the ORACLE on the same trace (rollout.cc:198-278 +
    buffer.cc:58-77): observation stacks byte-exact (update_observations), logits / values within `tol` of the oracle's
    fp32 forward, sampled actions bit-exact on ITS logits (when the noise is known), flag / reward planes exact, GAE planes
    bit-exact from ITS values.  checker (a bf16_check.Checker, bf16 acting): logits, values and next_values against the
    bf16-emulating forward under the checker's bounds instead of `tol` (its failures are left to the caller).
    Returns the stack after the last slot (= the next rollout's first observation)."""
    T, E = st.shape
    obs, stacks = obs0.copy(), []
    for t in range(T):
        stacks.append(obs.copy())
        obs = orc.update_observations(obs, frames84[t], st[t])
    obs_em = np.stack(stacks, 1)
    np.testing.assert_array_equal(b["observations"], obs_em)
    np.testing.assert_array_equal(b["masks"], 1 - st.T)
    if checker is not None:  # every slot's stack and the stack after the last slot in ONE emulated forward
        n = E * T
        wl, wv, (fl, fv) = bc.emulated_forward(params, H, A, np.concatenate([obs_em.reshape(n, 4, 84, 84), obs]))
        checker.forward(b["logits"].reshape(n, A), np.concatenate([b["values"].ravel(), b["next_values"]]),
                        (wl[:n], wv, (fl[:n], fv)), "rollout_")
    else:
        wl, wv = orc.net_forward(params, H, A, obs_em.reshape(E * T, 4, 84, 84))
        rtol = 1e-2 if tol > 1e-3 else 0  # bf16 operands: the documented bound is 1 % relative + 3e-2 absolute
        np.testing.assert_allclose(b["logits"].reshape(E * T, A), wl, atol=tol, rtol=rtol)
        np.testing.assert_allclose(b["values"].ravel(), wv, atol=tol, rtol=rtol)
        _, nv = orc.net_forward(params, H, A, obs)
        np.testing.assert_allclose(b["next_values"], nv, atol=tol, rtol=rtol)
    if noise is not None:
        want = orc.sample(orc.softmax(b["logits"].reshape(E * T, A)), noise.transpose(1, 0, 2).reshape(E * T, A))
        np.testing.assert_array_equal(b["actions"].ravel(), want)
    o = orc.buffer_get(rew.T, b["values"], b["next_values"], te.T, tr.T, st.T)
    np.testing.assert_array_equal(b["advantages"], o["advantages"])
    np.testing.assert_array_equal(b["returns"], o["returns"])
    return obs


# ------------------------------------------------------------------ GAE scan kernel: chunked path inside finish_rollout
@pytest.mark.parametrize("E,T", [(70, 41), (128, 128), (3, 16), (65, 32), (5, 48), (130, 7)])
def test_finish_rollout_gae_chunks_vs_oracle(pkg, E, T):
    """Buffer::get (buffer.cc:58-77) as aleppo_finish_rollout runs it: reward clamp in place, GAE, returns, masks.
    T = 41: 9-step tail + 2 chunks (both register sets); 128: 8 chunks (the benched shape); 16 / 32 / 48: chunks only
    with 1 / 2 / 3 loads; 7: tail only; E = 70 / 65 / 130: partial last wave.  Rewards leave [-1, 1] (the clamp acts),
    flags follow the slot protocol.  Same fp32 op order as the oracle -> bit-exact on OUR stored values."""
    A, H = 4, 32
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=5)
    eng.load_params(hf.fill_params(1310, H, A))
    te, tr, st = _flags(E * 1000 + T, T, E)
    rew = hf.hf_range(1311, (T, E), -3, 3)
    frames = DeviceBytes(hf.hf_bytes(1312, (2, E, 84, 84)))  # two alternating frame sets: content is irrelevant here
    for ro in range(2):  # the second rollout starts from the carried-over slot (state persists across rollouts)
        for t in range(T):
            eng.act_fast()
            eng.step_ptr(frames.addr + (t & 1) * E * 7056, pkg.DEVICE, pkg.FRAMES_84, rew[t].ctypes.data,
                         te[t].ctypes.data, tr[t].ctypes.data, st[t].ctypes.data)
        eng.finish_rollout()
        b = {k: eng.read_batch(k) for k in ("rewards", "values", "next_values", "advantages", "returns", "masks",
                                            "terminals", "truncations")}
        o = orc.buffer_get(rew.T, b["values"], b["next_values"], te.T, tr.T, st.T)
        np.testing.assert_array_equal(b["rewards"], np.clip(rew.T, -1, 1))
        np.testing.assert_array_equal(b["rewards"], o["rewards"])
        np.testing.assert_array_equal(b["terminals"], te.T)
        np.testing.assert_array_equal(b["truncations"], tr.T)
        np.testing.assert_array_equal(b["masks"], 1 - st.T)
        np.testing.assert_array_equal(b["advantages"], o["advantages"])
        np.testing.assert_array_equal(b["returns"], o["returns"])
        assert np.abs(b["advantages"]).max() > 0
    frames.free()
    eng.close()


def test_finish_rollout_rejects_overlapping_flags_in_a_chunk(pkg):
    """gae.cc:49-53 inside the chunked loop (the flag check accumulates into a register there)"""
    E, T, A, H = 9, 32, 4, 32
    eng = pkg.Engine(E, T, A, H)
    eng.load_params(hf.fill_params(1310, H, A))
    z = np.zeros(E, np.uint8)
    for t in range(T):
        eng.act_fast()
        bad = z.copy()
        if t == 20:
            bad[4] = 1
        eng.step(np.zeros((E, 84, 84), np.uint8), np.zeros(E, np.float32), bad, bad, z if t else np.ones(E, np.uint8))
    with pytest.raises(pkg.AleppoInvalidArgument, match="mutually exclusive"):
        eng.finish_rollout()
    eng.close()


# ------------------------------------------------------------------ the benched bf16 update against the oracle
def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


@pytest.mark.parametrize("A", [4, 6])
def test_bf16_update_at_benched_size_vs_oracle(pkg, A):
    """BASELINE configs[1] minibatch: B = 4096, H = 512, bf16 operands, A = 4 (Breakout) and 6 (Pong): loss, pre-clip
    gradient norm, EVERY gradient tensor, the per-sample metric planes and the parameters after 1 and after 4
    optimizer steps against orc.train (fp32) on the same batch.  Every kernel variant that only engages at large B
    is on this path."""
    H, N = 512, 4096
    params = hf.fill_params(1410, H, A)
    base = hf.hf_bytes(1411, (N // 8, 4, 84, 84))
    obs = np.concatenate([base ^ np.uint8(29 * k) for k in range(8)])
    actions = (hf.hf_u32(1412, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(1413, (N, A), -1, 1))
    adv, ret = hf.hf_range(1414, (N,), -1, 1), hf.hf_range(1415, (N,), -1, 1)
    masks = (hf.hf_unit(1416, N) >= np.float32(0.05)).astype(np.uint8)
    eng = pkg.Engine(128, 32, A, H, precision=pkg.BF16)  # E*T = 4096 samples
    eng.load_params(params)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    lr = 2.5e-4  # the reference's learning rate (configs/v0.yaml)
    offs = orc.param_offsets(H, A)
    names = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
             "value.w", "value.b"]
    adam, wparams, report, bad = None, params, {}, []

    def check(name, value, bound):
        report[name] = float(value)
        if not value <= bound:
            bad.append((name, float(value), bound))

    # step 1 on identical parameters; steps 2-3 on separate trajectories (each side on its own parameters); then the
    # engine is RE-SYNCHRONISED with the oracle's parameters and Adam state, so that step 4's gradients are again taken
    # on identical parameters and the step-1 bounds apply to them (no 25 % bound)
    for step, epochs, resync in ((1, 1, False), (3, 2, False), (4, 1, True)):
        if resync:
            eng.load_state_dict(dict(params=wparams, exp_avg=adam["m"], exp_avg_sq=adam["v"], step=adam["step"]))
        before, adam_before = wparams, adam
        m = eng.train(lr, epochs, 1)
        w = orc.train(wparams, H, A, obs, actions, old_lp, adv, ret, masks, epochs, 1, lr=lr, adam=adam)
        adam, wparams = w["adam"], w["params"]
        same = step != 3  # this step's gradient was taken on the oracle's own parameters
        # scalar loss / pre-clip norm of every step: 1 % relative + 3e-2 absolute on the loss (documented bf16 bound),
        # 5 % on the norm (measured: 0.1-0.5 % at step 1, 1.4-3 % at step 4)
        check(f"step{step}_loss", np.max(np.abs(m["loss"] - w["loss"]) - 1e-2 * np.abs(w["loss"])), 3e-2)
        check(f"step{step}_grad_norm_rel", np.max(np.abs(m["grad_norm"] / w["grad_norm"] - 1)), 5e-2)
        np.testing.assert_array_equal(m["mask_count"], np.full_like(m["mask_count"], masks.sum()))
        planes = {}
        # per-sample metric planes (Metrics::set, train.h:93-108): |error| <= 5e-2 + 5 % of the value on every sample
        # (value losses reach ~4 here: a 3e-2 error of v moves 0.5 (v - R)^2 by |v - R| * 3e-2), 1e-2 on the mean
        for ours, ref in (("total_losses", "total_losses"), ("ratio", "ratio"), ("entropies", "entropies"),
                          ("value_losses", "value_losses"), ("clipped_losses", "clipped")):
            got = planes[ours] = eng.read_train_metric(ours, epochs, 1, N)
            err = np.abs(got - w[ref])
            check(f"step{step}_{ours}_excess", np.max(err - 5e-2 * np.abs(w[ref])), 5e-2)
            check(f"step{step}_{ours}_mean_excess", err.mean() - 2e-2 * np.abs(w[ref]).mean(), 1e-2)
        # every gradient tensor of the last minibatch, as clip_grad_norm_ left it: relative L2 error per tensor
        g, wg = eng.export_grads(), w["last_grads"]
        cw = min(1.0, 0.5 / (float(w["grad_norm"][-1, -1]) + 1e-6))
        c0 = min(1.0, 0.5 / (float(m["grad_norm"][-1, -1]) + 1e-6))
        # measured on MI355X: 0.4-1.7 % per tensor on identical parameters, 1.3-2.3 % over all tensors on separate
        # trajectories
        if same:
            # (the action head at step 4: 4.3 / 6.4 % from the fp32 oracle for its weight / bias at A = 4 on identical
            # parameters.  The emulated oracle shows that gap is bf16 quantisation, not a kernel error: the emulation
            # itself is 4.3 / 6.4 % (A = 4) and 2.6 / 2.3 % (A = 6) from the fp32 oracle there
            # (step4_emu_vs_fp32_grad_action.*, printed in the report) while the engine is within 2.1e-4 of the
            # emulation (step4_emu_grad_action.*, bound bf16_check.BOUNDS["grad"]).  So 1e-1 stays on the fp32
            # comparison of the action head after step 1 only as that quantisation envelope; 3e-2 elsewhere)
            for k, nm in enumerate(names):
                bound = 1e-1 if step > 1 and nm.startswith("action") else 3e-2  # quantisation envelope (see above)
                check(f"step{step}_grad_{nm}_rel", _rel(g[offs[k]:offs[k + 1]] / c0, wg[offs[k]:offs[k + 1]] / cw), bound)
            check(f"step{step}_grad_all_rel", _rel(g / c0, wg / cw), 2e-2)
        else:  # separate trajectories: only the whole gradient, loosely (measured 1.3-2.3 %)
            check(f"step{step}_grad_all_rel", _rel(g / c0, wg / cw), 5e-2)
        # parameters: Adam's first steps move every weight by ~lr whatever the gradient's size, so a bf16 sign flip of
        # a near-zero gradient entry costs up to 2 lr per step: bound 2.5 lr * steps on the max, lr / 5 * steps on the mean
        p = eng.export_params()
        if same:  # the same step against the bf16-emulating oracle, on the same parameters and Adam state
            we = bc.emulated_train(before, H, A, obs, actions, old_lp, adv, ret, masks, epochs, 1, lr=lr,
                                   adam=adam_before)
            c = bc.Checker()
            c.train(H, A, m, planes, g, we, params0=before, params=p)
            report.update({f"step{step}_emu_{k}": v for k, v in c.report.items()})
            bad.extend((f"step{step}_emu_{k}", v, b) for k, v, b in c.failures)
            ce = min(1.0, 0.5 / (float(we["grad_norm"][-1, -1]) + 1e-6))
            for k in (8, 9):  # how far bf16 quantisation alone moves the action head (report only)
                report[f"step{step}_emu_vs_fp32_grad_{names[k]}"] = _rel(we["last_grads"][offs[k]:offs[k + 1]] / ce,
                                                                         wg[offs[k]:offs[k + 1]] / cw)
        d = np.abs(p - wparams)
        drift = 1 if resync else step  # optimizer steps since the two sides last had identical parameters
        check(f"step{step}_param_maxabs_over_lr", d.max() / lr, 2.5 * drift)
        check(f"step{step}_param_meanabs_over_lr", d.mean() / lr, 0.2 * drift)
        assert np.abs(p - before).max() > 0.5 * lr
    print("bf16-at-size report A=%d" % A, {k: round(v, 5) for k, v in report.items()})
    assert not bad, bad
    eng.close()


# ------------------------------------------------------------------ the north star's 1e-4, at the benched size
def test_fp32_update_at_benched_size_vs_oracle(pkg):
    """The fp32 path (exact fp32 MFMA chains on the generic gather-GEMMs, split-K slabs, the 1-D swizzled gemm_tn launch,
    gemm_nt_dma fc) at BASELINE configs[1]'s minibatch - B = 4096, H = 512 - and at 2 x 2048 against orc.train
    (train.h:114-157): loss 1e-4, pre-clip gradient norm 1e-4 relative, every per-sample metric plane 1e-4, every
    gradient tensor 1e-4 relative L2, parameters 1e-4 (and 2 % of lr) after each optimizer step.  BASELINE.json:
    "losses/returns within 1e-4 fp32"."""
    H, N, A = 512, 4096, 4
    params = hf.fill_params(1450, H, A)
    base = hf.hf_bytes(1451, (N // 8, 4, 84, 84))
    obs = np.concatenate([base ^ np.uint8(37 * k % 256) for k in range(8)])
    actions = (hf.hf_u32(1452, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(1453, (N, A), -1, 1))
    adv, ret = hf.hf_range(1454, (N,), -1, 1), hf.hf_range(1455, (N,), -1, 1)
    masks = (hf.hf_unit(1456, N) >= np.float32(0.05)).astype(np.uint8)
    eng = pkg.Engine(128, 32, A, H, precision=pkg.FP32)
    eng.load_params(params)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    lr = 2.5e-4
    offs = orc.param_offsets(H, A)
    names = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
             "value.w", "value.b"]
    adam, wparams, report, bad = None, params, {}, []

    def check(name, value, bound):
        report[name] = float(value)
        if not value <= bound:
            bad.append((name, float(value), bound))

    for tag, M in (("B4096", 1), ("B2048", 2)):  # the second call continues from the first one's parameters / Adam state
        m = eng.train(lr, 1, M)
        w = orc.train(wparams, H, A, obs, actions, old_lp, adv, ret, masks, 1, M, lr=lr, adam=adam)
        adam, wparams = w["adam"], w["params"]
        check(f"{tag}_loss", np.abs(m["loss"] - w["loss"]).max(), 1e-4)
        check(f"{tag}_grad_norm_rel", np.abs(m["grad_norm"] / w["grad_norm"] - 1).max(), 1e-4)
        for ours, ref in (("total_losses", "total_losses"), ("ratio", "ratio"), ("entropies", "entropies"),
                          ("value_losses", "value_losses"), ("clipped_losses", "clipped")):
            got = eng.read_train_metric(ours, 1, M, N // M)
            check(f"{tag}_{ours}", np.abs(got - w[ref]).max(), 1e-4)
        g, wg = eng.export_grads(), w["last_grads"]
        cw = min(1.0, 0.5 / (float(w["grad_norm"][-1, -1]) + 1e-6))
        c0 = min(1.0, 0.5 / (float(m["grad_norm"][-1, -1]) + 1e-6))
        for k, nm in enumerate(names):
            check(f"{tag}_grad_{nm}_rel", _rel(g[offs[k]:offs[k + 1]] / c0, wg[offs[k]:offs[k + 1]] / cw), 1e-4)
        p = eng.export_params()
        d = np.abs(p - wparams)
        check(f"{tag}_param_maxabs", d.max(), 1e-4)
        check(f"{tag}_param_maxabs_over_lr", d.max() / lr, 2e-2)
    print("fp32-at-size report", {k: float("%.3g" % v) for k, v in report.items()})
    assert not bad, bad
    eng.close()


# ------------------------------------------------------------------ the bench's rollout path, all together
def test_replay_rollout_raw_bf16_e128_vs_oracle(pkg):
    """aleppo_replay_rollout + ALEPPO_FRAMES_RAW_PAIR + bf16 acting + E = 128 (bench.py's rollout leg) against the
    oracle's planes: observation / flag / reward / action planes bit-exact, logits / values within the bf16 bound of
    the oracle's fp32 forward, GAE planes bit-exact from OUR values.  T = 24 = 8-step tail + one chunk."""
    E, T, A, H = 128, 24, 4, 512
    params = hf.fill_params(1510, H, A)
    lut = (np.arange(256) // 2 * 2).astype(np.uint8)
    raw = (hf.hf_bytes(1511, (T, E, 2, 210, 160)) & np.uint8(0xFE))  # ALE palette codes are even
    dev = DeviceBytes(raw)
    te, tr, st = _flags(1512, T, E, 0.05, 0.02)
    rew = np.where(hf.hf_unit(1513, T * E) < np.float32(0.2), hf.hf_range(1514, (T * E,), -4, 7), 0).astype(
        np.float32).reshape(T, E)
    noise = np.random.default_rng(1515).exponential(size=(T, E, A)).astype(np.float32)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, seed=3)
    eng.load_params(params)
    eng.set_gray_lut(lut)
    eng.replay_rollout(dev.addr, pkg.FRAMES_RAW_PAIR, E * 2 * 210 * 160, rew, te, tr, st, noise=noise)
    eng.finish_rollout(np.random.default_rng(1516).exponential(size=(E, A)).astype(np.float32))
    b = {k: eng.read_batch(k) for k in pkg.FIELDS if k != "current_obs"}
    # oracle planes
    obs_ref = np.zeros((E, 4, 84, 84), np.uint8)
    obs_all = []
    for t in range(T):
        obs_all.append(obs_ref.copy())
        obs_ref = orc.update_observations(obs_ref, orc.preprocess(raw[t], lut), st[t])
    obs_em = np.stack(obs_all, 1)
    np.testing.assert_array_equal(b["observations"], obs_em)
    np.testing.assert_array_equal(eng.read_batch("current_obs"), obs_ref)
    np.testing.assert_array_equal(b["terminals"], te.T)
    np.testing.assert_array_equal(b["truncations"], tr.T)
    np.testing.assert_array_equal(b["masks"], 1 - st.T)
    np.testing.assert_array_equal(b["rewards"], np.clip(rew.T, -1, 1))
    wl, wv = orc.net_forward(params, H, A, obs_em.reshape(E * T, 4, 84, 84))
    np.testing.assert_allclose(b["logits"].reshape(E * T, A), wl, atol=3e-2)  # bf16 operands: documented bound
    np.testing.assert_allclose(b["values"].ravel(), wv, atol=3e-2)
    _, nv = orc.net_forward(params, H, A, obs_ref)
    np.testing.assert_allclose(b["next_values"], nv, atol=3e-2)
    want = orc.sample(orc.softmax(b["logits"].reshape(E * T, A)), noise.transpose(1, 0, 2).reshape(E * T, A))
    np.testing.assert_array_equal(b["actions"].ravel(), want)  # integer indices: bit-exact on ITS logits
    o = orc.buffer_get(rew.T, b["values"], b["next_values"], te.T, tr.T, st.T)
    np.testing.assert_array_equal(b["advantages"], o["advantages"])
    np.testing.assert_array_equal(b["returns"], o["returns"])
    np.testing.assert_allclose(b["log_probs"].reshape(E * T, A), orc.log_softmax(b["logits"].reshape(E * T, A)),
                               atol=2e-6)
    dev.free()
    eng.close()


def test_replay_from_mapped_host_memory_equals_device_frames(pkg):
    """ALEPPO_HOST_MAPPED: the ingest kernel reads the frames in place from page-locked host memory (the ring the
    emulator threads would write, rollout.cc:325-326) - same rollout as with the frames resident in HBM"""
    E, T, A, H = 16, 5, 4, 64
    hip = ctypes.CDLL("libamdhip64.so")
    frames = hf.hf_bytes(1611, (T, E, 84, 84))
    hptr = ctypes.c_void_p()
    assert hip.hipHostMalloc(ctypes.byref(hptr), ctypes.c_size_t(frames.nbytes), ctypes.c_uint(2)) == 0  # Mapped
    ctypes.memmove(hptr, frames.ctypes.data, frames.nbytes)
    dev = DeviceBytes(frames)
    te, tr, st = _flags(1612, T, E)
    rew = hf.hf_range(1613, (T, E), -2, 2)
    got = []
    for loc, addr in ((pkg.DEVICE, dev.addr), (pkg.HOST_MAPPED, hptr.value)):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, seed=11)
        eng.load_params(hf.fill_params(1610, H, A))
        eng.replay_rollout(addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st, location=loc)
        eng.finish_rollout()
        got.append({k: eng.read_batch(k) for k in ("observations", "actions", "values", "logits", "next_values", "masks",
                                                   "advantages", "returns")})
        eng.close()
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    np.testing.assert_array_equal(got[0]["observations"][:, 1, 0], frames[0])
    # ... and the mapped-memory rollout itself against the oracle (not only against the HBM-resident one)
    _rollout_vs_oracle(got[1], frames, st, rew, te, tr, np.zeros((E, 4, 84, 84), np.uint8), hf.fill_params(1610, H, A), H, A,
                       3e-2)
    hip.hipHostFree(hptr)
    dev.free()


@pytest.mark.parametrize("kind", ["84", "raw"])
def test_fused_ingest_acting_launch_equals_separate_launches(pkg, kind):
    """bf16 acting: aleppo_step's ONE launch (frame ingest + conv1-3, act_conv_kernel<1 / 2>) against the separate
    ingest_kernel + act_conv_kernel<0> launches (ALEPPO_OPT_FUSED_ACT = 0): identical bytes in every plane.  E = 300 >
    256 CUs: workgroups loop over environments (weights stay in registers, LDS regions are recycled)."""
    E, T, A, H = 300, 4, 6, 512
    per_env = 84 * 84 if kind == "84" else 2 * 210 * 160
    frames = hf.hf_bytes(2011, (T, E, per_env))
    dev = DeviceBytes(frames)
    te, tr, st = _flags(2012, T, E, 0.2, 0.1)
    rew = hf.hf_range(2013, (T, E), -2, 2)
    noise = np.random.default_rng(2015).exponential(size=(T, E, A)).astype(np.float32)
    lut = ((np.arange(256) * 3 + 7) % 256).astype(np.uint8)
    got = []
    for fused in (0, 2):  # 2: fused for every frame kind and location
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, seed=4)
        eng.set_option(pkg.OPT_FUSED_ACT, fused)
        eng.load_params(hf.fill_params(2010, H, A))
        eng.set_gray_lut(lut)
        for ro in range(2):
            eng.replay_rollout(dev.addr, pkg.FRAMES_84 if kind == "84" else pkg.FRAMES_RAW_PAIR, E * per_env, rew, te,
                               tr, st, noise=noise)
            eng.finish_rollout(noise[0])
        got.append({k: eng.read_batch(k) for k in ("observations", "current_obs", "actions", "logits", "values",
                                                   "next_values", "advantages", "returns")})
        eng.close()
    dev.free()
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    assert got[0]["observations"].any()
    # the fused launch against the ORACLE: both rollouts of the trace replayed on the CPU (the second starts from the
    # first one's last stack); the read-back planes are the second rollout's
    f84 = frames.reshape(T, E, 84, 84) if kind == "84" else np.stack(
        [orc.preprocess(frames[t].reshape(E, 2, 210, 160), lut) for t in range(T)])
    obs1 = np.zeros((E, 4, 84, 84), np.uint8)
    for t in range(T):
        obs1 = orc.update_observations(obs1, f84[t], st[t])
    got[1]["masks"] = 1 - st.T
    last = _rollout_vs_oracle(got[1], f84, st, rew, te, tr, obs1, hf.fill_params(2010, H, A), H, A, 3e-2, noise=noise)
    np.testing.assert_array_equal(got[1]["current_obs"], last)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_captured_update_graph_is_bit_identical_to_eager(pkg, prec):
    """ALEPPO_OPT_UPDATE_GRAPH (capture_train_cuda_graph, train.h:163-195): call 1 runs eagerly, call 2 captures the
    epochs x minibatches loop (two streams, cross-stream events) into a hipGraph, calls 3-4 replay it.  The learning
    rate is annealed between calls (train.cc:424-428) and Adam's bias corrections advance: both are device scalars, so a
    replay must follow them (the reference's captured graph bakes them) - every call bit-identical to the eager engine."""
    E, T, A, H, M, epochs = (128, 32, 4, 512, 2, 2) if prec == "bf16" else (16, 8, 6, 64, 2, 2)
    N = E * T
    params = hf.fill_params(2110, H, A)
    base = hf.hf_bytes(2111, (N // 8, 4, 84, 84))
    obs = np.concatenate([base ^ np.uint8(17 * k) for k in range(8)])
    actions = (hf.hf_u32(2112, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(2113, (N, A), -1, 1))
    adv, ret = hf.hf_range(2114, (N,), -1, 1), hf.hf_range(2115, (N,), -1, 1)
    masks = (hf.hf_unit(2116, N) >= np.float32(0.05)).astype(np.uint8)
    outs = []
    for graph in (0, 1):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32)
        eng.set_option(pkg.OPT_UPDATE_GRAPH, graph)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        hist = []
        for call in range(4):
            m = eng.train(pkg.learning_rate(2.5e-4, call, 8), epochs, M)
            hist.append((m["loss"].copy(), m["grad_norm"].copy(), eng.export_params()))
        sd = eng.state_dict()
        outs.append((hist, sd["exp_avg"].copy(), sd["exp_avg_sq"].copy(), int(sd["step"])))
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) == (3 if graph else 0)  # calls 2-4 went through the graph
        eng.close()
    eager, graph = outs
    assert eager[3] == graph[3] == 4 * epochs * M
    for call in range(4):
        for a, b in zip(eager[0][call], graph[0][call]):
            np.testing.assert_array_equal(a, b, err_msg=f"call {call}")
    np.testing.assert_array_equal(eager[1], graph[1])
    np.testing.assert_array_equal(eager[2], graph[2])
    assert np.abs(eager[0][3][2] - eager[0][2][2]).max() > 0  # the replays kept learning
    if prec == "fp32":
        # the replayed graph itself against the ORACLE: four annealed calls of train() (train.h:133-157).  Before every call
        # the engine takes the oracle's parameters and Adam state (the buffers keep their addresses, so the captured graph
        # stays valid): each call's four optimizer steps then start from identical state and the fp32 bounds apply to the
        # replays (calls 2 and 3) as they do to the eager call 0
        eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        adam, wparams = None, params
        for call in range(4):
            if call:
                eng.load_state_dict(dict(params=wparams, exp_avg=adam["m"], exp_avg_sq=adam["v"], step=adam["step"]))
            lr = pkg.learning_rate(2.5e-4, call, 8)
            m = eng.train(lr, epochs, M)
            w = orc.train(wparams, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, lr=lr, adam=adam)
            adam, wparams = w["adam"], w["params"]
            np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4, err_msg=f"call {call}: loss")
            np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=2e-4, err_msg=f"call {call}: norm")
            np.testing.assert_allclose(eng.export_params(), wparams, atol=1e-4, err_msg=f"call {call}: parameters")
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) == 3 and int(eng.state_dict()["step"]) == adam["step"]
        eng.close()


def test_contexts_used_alternately_match_contexts_used_alone(pkg):
    """Three contexts alive at the same time (different kernel switches, different precisions) and driven ALTERNATELY from
    one thread - update calls and whole rollouts interleaved: every context carries its own streams, scratch, switches,
    pinned hand-off words and error state, so each gives the bits it gives when it is the only context of the process
    (rollout.h keeps everything per Rollout object; ADVICE r1: process-global switches)."""
    cfgs = [dict(E=64, T=8, A=4, H=512, prec=pkg.BF16, generic=0, seed=2610),
            dict(E=16, T=8, A=6, H=64, prec=pkg.FP32, generic=0, seed=2620),
            dict(E=64, T=8, A=6, H=512, prec=pkg.BF16, generic=1, seed=2630)]
    keys = ("observations", "actions", "values", "advantages", "returns")

    def build(c):
        E, T = c["E"], c["T"]
        eng = pkg.Engine(E, T, c["A"], c["H"], precision=c["prec"], seed=c["seed"])
        eng.set_generic_conv(c["generic"])
        eng.load_params(hf.fill_params(c["seed"], c["H"], c["A"]))
        dev = DeviceBytes(hf.hf_bytes(c["seed"] + 1, (T, E, 84, 84)))
        te, tr, st = _flags(c["seed"] + 2, T, E)
        return eng, dev, (hf.hf_range(c["seed"] + 3, (T, E), -2, 2), te, tr, st)

    def round_of(item):
        eng, dev, (rew, te, tr, st) = item
        eng.replay_rollout(dev.addr, pkg.FRAMES_84, eng.E * 7056, rew, te, tr, st)
        eng.finish_rollout()
        planes = [eng.read_batch(q) for q in keys]
        m = eng.train(2.5e-4, 2, 2)
        return planes + [m["loss"].copy(), m["grad_norm"].copy(), eng.export_params()]

    alone = []
    for c in cfgs:
        item = build(c)
        alone.append([round_of(item) for _ in range(3)])
        item[0].close()
        item[1].free()
    items = [build(c) for c in cfgs]
    together = [[] for _ in cfgs]
    for r in range(3):
        for k in (2, 0, 1) if r % 2 else (0, 1, 2):
            together[k].append(round_of(items[k]))
    for it in items:
        it[0].close()
        it[1].free()
    for k in range(len(cfgs)):
        for r in range(3):
            for a, b in zip(alone[k][r], together[k][r]):
                np.testing.assert_array_equal(a, b, err_msg=f"context {k}, round {r}")


def test_engines_trained_concurrently_from_threads_match_engines_trained_alone(pkg):
    """Two contexts in one process, each driven by its own host thread at the same time (different kernel switches,
    different precisions): every context carries its own streams, scratch, switches and error state, every entry point
    selects its device and its context's switches, so the results must be bit-identical to the same engines run one after
    the other (rollout.h keeps everything per Rollout object; ADVICE r1: process-global switches)."""
    import threading
    cfgs = [dict(E=64, T=32, A=4, H=512, prec=pkg.BF16, generic=0, seed=2310),
            dict(E=16, T=8, A=6, H=64, prec=pkg.FP32, generic=0, seed=2320),
            dict(E=64, T=32, A=6, H=512, prec=pkg.BF16, generic=1, seed=2330)]

    def build(c):
        N = c["E"] * c["T"]
        eng = pkg.Engine(c["E"], c["T"], c["A"], c["H"], precision=c["prec"])
        eng.set_generic_conv(c["generic"])
        eng.load_params(hf.fill_params(c["seed"], c["H"], c["A"]))
        eng.set_batch(hf.hf_bytes(c["seed"] + 1, (N, 4, 84, 84)), (hf.hf_u32(c["seed"] + 2, N) % np.uint32(c["A"])).astype(np.int64),
                      orc.log_softmax(hf.hf_range(c["seed"] + 3, (N, c["A"]), -1, 1)), hf.hf_range(c["seed"] + 4, (N,), -1, 1),
                      hf.hf_range(c["seed"] + 5, (N,), -1, 1), np.ones(N, np.uint8))
        return eng

    def work(eng, out, k):
        try:
            hist = []
            for call in range(3):
                m = eng.train(2.5e-4, 2, 2)
                hist.append((m["loss"].copy(), m["grad_norm"].copy()))
            out[k] = (hist, eng.export_params())
        except Exception as e:  # surfaced by the asserts below
            out[k] = e

    alone, together = {}, {}
    for k, c in enumerate(cfgs):
        eng = build(c)
        work(eng, alone, k)
        eng.close()
    engs = [build(c) for c in cfgs]
    threads = [threading.Thread(target=work, args=(e, together, k)) for k, e in enumerate(engs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for e in engs:
        e.close()
    for k in range(len(cfgs)):
        assert not isinstance(alone[k], Exception), alone[k]
        assert not isinstance(together[k], Exception), together[k]
        for (l0, g0), (l1, g1) in zip(alone[k][0], together[k][0]):
            np.testing.assert_array_equal(l0, l1, err_msg=f"engine {k}: loss")
            np.testing.assert_array_equal(g0, g1, err_msg=f"engine {k}: grad norm")
        np.testing.assert_array_equal(alone[k][1], together[k][1], err_msg=f"engine {k}: parameters")


@pytest.mark.parametrize("prec,kind,generic", [("bf16", "84", 0), ("bf16", "raw", 0), ("fp32", "84", 0), ("bf16", "84", 1)])
def test_armed_live_loop_equals_the_plain_act_step_loop(pkg, prec, kind, generic):
    """aleppo_arm_step / aleppo_release_step (the stream one slot ahead of the emulator, behind the gate kernel): the
    emulator here is this test - after every aleppo_act it writes the slot's frames and episode-start bytes into mapped
    host memory and only then releases.  Every stored plane equals the plain aleppo_act / aleppo_step loop on the same
    trace (fused ingest + acting launch, stand-alone ingest kernel, fp32 generic kernels), two rollouts back to back."""
    E, T, A, H = 37, 9, 6, 64 if prec == "fp32" else 512
    raw = kind == "raw"
    fbytes = E * (2 * 210 * 160 if raw else 7056)
    fkind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    frames = hf.hf_bytes(2510, (2 * T, fbytes))
    te, tr, st = _flags(2511, 2 * T, E)
    rew = hf.hf_range(2512, (2 * T, E), -2, 2)
    noise = -np.log(np.clip(hf.hf_unit(2513, (2 * T + 2) * E * A).reshape(2 * T + 2, E, A), 1e-6, 1.0)).astype(np.float32)
    keys = ("observations", "actions", "values", "logits", "advantages", "returns", "masks", "rewards", "terminals",
            "next_values")
    got = {}
    for armed in (0, 1):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=5)
        eng.set_generic_conv(generic)
        eng.load_params(hf.fill_params(2514, H, A))
        fbuf, sbuf = eng.host_alloc(fbytes), eng.host_alloc(E)
        planes, k = [], 0
        for r in range(2):
            for t in range(T):
                g = r * T + t
                actions = eng.act(noise[k]).copy() if not (armed and t > 0) else eng.act().copy()
                k += 1
                assert actions.min() >= 0 and actions.max() < A
                if armed:
                    # the next slot's head is enqueued now, with ITS noise; the emulator has not produced anything yet
                    eng.arm_step(fbuf, sbuf, fkind, noise_next=noise[k] if t + 1 < T else None)
                    with pytest.raises(pkg.AleppoError):
                        eng.finish_rollout()  # every other stateful call is refused while a step is armed
                    ctypes.memmove(fbuf, frames[g].ctypes.data, fbytes)
                    ctypes.memmove(sbuf, st[g].ctypes.data, E)
                    eng.release_step(rew[g], te[g], tr[g])
                else:
                    ctypes.memmove(fbuf, frames[g].ctypes.data, fbytes)
                    self_st = st[g]
                    lib = pkg.lib()
                    rc = lib.aleppo_step(eng._ctx, ctypes.c_void_p(fbuf), fkind, pkg.HOST_MAPPED, rew[g].ctypes.data_as(ctypes.c_void_p),
                                         te[g].ctypes.data_as(ctypes.c_void_p), tr[g].ctypes.data_as(ctypes.c_void_p),
                                         self_st.ctypes.data_as(ctypes.c_void_p))
                    assert rc == 0, eng.last_error() if hasattr(eng, "last_error") else rc
            eng.finish_rollout(noise[k])
            k += 1
            planes.append({q: eng.read_batch(q) for q in keys})
        got[armed] = planes
        eng.host_free(fbuf)
        eng.host_free(sbuf)
        eng.close()
    for r in range(2):
        for q in keys:
            np.testing.assert_array_equal(got[0][r][q], got[1][r][q], err_msg=f"rollout {r}: {q}")
    # the armed loop against the ORACLE, both rollouts (identity gray table; noise k = r (T + 1) + t)
    f84 = frames.reshape(2 * T, E, 84, 84) if not raw else np.stack(
        [orc.preprocess(frames[g].reshape(E, 2, 210, 160), np.arange(256, dtype=np.uint8)) for g in range(2 * T)])
    obs = np.zeros((E, 4, 84, 84), np.uint8)
    for r in range(2):
        sl = slice(r * T, (r + 1) * T)
        obs = _rollout_vs_oracle(got[1][r], f84[sl], st[sl], rew[sl], te[sl], tr[sl], obs, hf.fill_params(2514, H, A), H, A,
                                 1e-4 if prec == "fp32" else 3e-2, noise=noise[r * (T + 1):r * (T + 1) + T])


def test_gated_replay_equals_launch_per_slot_replay():
    """aleppo_replay_rollout with the stream one slot ahead of the host (a gate kernel polling the release word, the
    default) against ALEPPO_REPLAY_GATED=0 (a launch per slot after the actions arrived): the same bits in every stored
    plane at T = 1, T = 2, more environments than CUs, 18 actions, and the benched E = 128"""
    out = {}
    for gated in ("1", "0"):
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "replay_digest.py")],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, ALEPPO_REPLAY_GATED=gated))
        assert r.returncode == 0, r.stderr[-2000:]
        out[gated] = [l for l in r.stdout.splitlines() if l.startswith("digest")][-1]
    assert out["1"] == out["0"]


def test_rollouts_run_concurrently_from_threads_match_rollouts_run_alone(pkg):
    """the acting path of two contexts at the same time (own pinned action buffer, ticket word and device counter each):
    every stored plane equals the same rollout run alone"""
    import threading
    cfgs = [dict(E=40, T=12, A=4, H=512, prec=pkg.BF16, seed=2410), dict(E=9, T=20, A=6, H=64, prec=pkg.FP32, seed=2420)]
    keys = ("observations", "actions", "values", "logits", "advantages", "returns", "masks")

    def build(c):
        E, T = c["E"], c["T"]
        dev = DeviceBytes(hf.hf_bytes(c["seed"] + 1, (T, E, 84, 84)))
        te, tr, st = _flags(c["seed"] + 2, T, E)
        eng = pkg.Engine(E, T, c["A"], c["H"], precision=c["prec"], seed=c["seed"])
        eng.load_params(hf.fill_params(c["seed"], c["H"], c["A"]))
        return eng, dev, (hf.hf_range(c["seed"] + 3, (T, E), -2, 2), te, tr, st)

    def work(item, out, k):
        eng, dev, (rew, te, tr, st) = item
        try:
            for _ in range(2):  # two rollouts: the second starts from the first one's last stack
                eng.replay_rollout(dev.addr, pkg.FRAMES_84, eng.E * 7056, rew, te, tr, st)
                eng.finish_rollout()
            out[k] = {q: eng.read_batch(q) for q in keys}
        except Exception as e:
            out[k] = e

    alone, together = {}, {}
    for k, c in enumerate(cfgs):
        item = build(c)
        work(item, alone, k)
        item[0].close()
        item[1].free()
    items = [build(c) for c in cfgs]
    threads = [threading.Thread(target=work, args=(it, together, k)) for k, it in enumerate(items)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for it in items:
        it[0].close()
        it[1].free()
    for k in range(len(cfgs)):
        assert not isinstance(alone[k], Exception), alone[k]
        assert not isinstance(together[k], Exception), together[k]
        for q in keys:
            np.testing.assert_array_equal(alone[k][q], together[k][q], err_msg=f"engine {k}: {q}")


# ------------------------------------------------------------------ the slot-ahead hand-off under several contexts
def test_other_contexts_and_operators_never_wait_for_a_parked_stream():
    """The cause of round 2's two-thread hang, made deterministic (tests/parked_contexts.py, run in a process of its own
    because it lays out the process's hardware queues itself).  Context A has a step ARMED: its stream is parked behind
    the release word, which only A's owner lifts.  hipFree / hipHostFree / hipDeviceSynchronize wait for EVERY stream of the
    device AND block the owner's next enqueue on the parked stream while they wait (tests/tools/parkprobe.hip,
    profiles/r03_parkprobe.log) - so an entry point that calls one of them on behalf of context B while A's owner is between
    its gate and its release dead-locks the process.  No entry point but aleppo_destroy / aleppo_host_free calls them any
    more: creating a second context, a whole rollout and update on it, every read-back (which used to hipMalloc + hipFree
    per call), staging buffers that have to grow and the stateless operators all complete while A stays armed."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "parked_contexts.py")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "parked-contexts ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_gate_exit_condition_fails_the_context_instead_of_hanging(pkg):
    """The gate kernel never waits for ever: with a 100 ms limit and a host that comes 0.6 s late, the gate gives up, the
    stream drains (slot t + 1 ran on frames the host had not delivered), and the late aleppo_release_step fails the context
    - sticky until aleppo_destroy - instead of handing back a rollout built on undelivered frames."""
    E, T, A, H = 8, 4, 4, 32
    eng = pkg.Engine(E, T, A, H, seed=3)
    eng.load_params(hf.fill_params(2720, H, A))
    eng.set_option(pkg.OPT_GATE_TIMEOUT_MS, 100)
    assert eng.get_option(pkg.OPT_GATE_TIMEOUT_MS) == 100
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    z32, z8 = np.zeros(E, np.float32), np.zeros(E, np.uint8)
    lib = pkg.lib()
    eng.act()
    eng.arm_step(fbuf, sbuf, pkg.FRAMES_84)
    # a null argument is reported while the step is still armed and can be repeated
    rc = lib.aleppo_release_step(eng._ctx, None, z8.ctypes.data_as(ctypes.c_void_p), z8.ctypes.data_as(ctypes.c_void_p))
    assert rc == -1
    eng.release_step(z32, z8, z8)  # in time: fine
    eng.act()
    eng.arm_step(fbuf, sbuf, pkg.FRAMES_84)
    time.sleep(0.6)
    with pytest.raises(pkg.AleppoError, match="gate"):
        eng.release_step(z32, z8, z8)
    with pytest.raises(pkg.AleppoError, match="unusable"):
        eng.act()
    with pytest.raises(pkg.AleppoError, match="unusable"):
        eng.finish_rollout()
    eng.close()  # (releases what is left and drains the stream)
    e2 = pkg.Engine(E, T, A, H, seed=3)  # the device is fine
    e2.load_params(hf.fill_params(2720, H, A))
    e2.act()
    e2.close()


# ------------------------------------------------------------------ advantage normalisation (extension; unpinned)
@pytest.mark.parametrize("E,T", [(6, 9), (128, 32)])
def test_advantage_norm_extension_vs_oracle(pkg, E, T):
    """advantage_norm = 1 (NOT in the reference, SURVEY Q2 - off by default; PARITY UNPINNED: checked against the
    oracle's own definition only): masked mean / unbiased std over the rollout's unmasked samples, applied before the
    update; returns stay un-normalised."""
    A, H = 4, 32
    te, tr, st = _flags(1712, T, E)
    rew = hf.hf_range(1713, (T, E), -2, 2)
    frames = DeviceBytes(hf.hf_bytes(1714, (E, 84, 84)))
    out = []
    for norm in (False, True):
        eng = pkg.Engine(E, T, A, H, seed=9, advantage_norm=norm)
        eng.load_params(hf.fill_params(1710, H, A))
        for t in range(T):
            eng.act_fast()
            eng.step_ptr(frames.addr, pkg.DEVICE, pkg.FRAMES_84, rew[t].ctypes.data, te[t].ctypes.data,
                         tr[t].ctypes.data, st[t].ctypes.data)
        eng.finish_rollout()
        out.append({k: eng.read_batch(k) for k in ("advantages", "returns", "masks")})
        eng.close()
    frames.free()
    plain, normed = out
    np.testing.assert_array_equal(plain["returns"], normed["returns"])
    want = orc.adv_norm(plain["advantages"], plain["masks"])
    np.testing.assert_allclose(normed["advantages"], want, rtol=2e-4, atol=2e-5)
    sel = normed["advantages"][normed["masks"] != 0]
    assert abs(sel.mean()) < 1e-4 and abs(sel.std(ddof=1) - 1) < 1e-3


def test_advantage_norm_with_every_sample_masked_is_a_no_op(pkg):
    E, T, A, H = 4, 3, 4, 32
    eng = pkg.Engine(E, T, A, H, advantage_norm=True)
    eng.load_params(hf.fill_params(1710, H, A))
    one, z = np.ones(E, np.uint8), np.zeros(E, np.uint8)
    for t in range(T):
        eng.act_fast()
        eng.step(np.zeros((E, 84, 84), np.uint8), np.zeros(E, np.float32), z, z, one)  # every slot an episode start
    eng.finish_rollout()
    a = eng.read_batch("advantages")
    assert np.isfinite(a).all() and (a == 0).all()
    eng.close()


# ------------------------------------------------------------------ configs[4]: fp16 rollout buffer + mixed precision
def _h(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def test_fp16_rollout_buffer_mixed_precision_vs_oracle(pkg):
    """BASELINE configs[4] per-GPU shape: E_g = 256 envs, A = 6 (SpaceInvaders), rollout_precision = FP16 (values,
    logits, advantages, returns, old log-probs stored as IEEE half; the reference's Buffer holds f32 planes,
    buffer.cc:12-38) with the bf16 / fp32-master update.  Oracle planes = the oracle's fp32 arithmetic on the
    half-rounded inputs, rounded to half where the library stores: GAE planes bit-exact (same op order, RNE both
    sides), log-probs within one half ulp, network outputs within the bf16 bound, update within the bf16 bound."""
    E, T, A, H = 256, 16, 6, 512
    params = hf.fill_params(1910, H, A)
    frames = hf.hf_bytes(1911, (T, E, 84, 84))
    dev = DeviceBytes(frames)
    te, tr, st = _flags(1912, T, E, 0.05, 0.02)
    rew = hf.hf_range(1913, (T, E), -2, 2)
    noise = np.random.default_rng(1915).exponential(size=(T, E, A)).astype(np.float32)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, rollout_precision=pkg.ROLLOUT_FP16, seed=3)
    eng.load_params(params)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rew, te, tr, st, noise=noise)
    eng.finish_rollout(np.random.default_rng(1916).exponential(size=(E, A)).astype(np.float32))
    b = {k: eng.read_batch(k) for k in pkg.FIELDS if k != "current_obs"}
    for k in ("values", "logits", "advantages", "returns", "log_probs", "next_values"):
        np.testing.assert_array_equal(b[k], _h(b[k]), err_msg=f"{k} is not a half-precision plane")
    obs_ref = np.zeros((E, 4, 84, 84), np.uint8)
    obs_all = []
    for t in range(T):
        obs_all.append(obs_ref.copy())
        obs_ref = orc.update_observations(obs_ref, frames[t], st[t])
    obs_em = np.stack(obs_all, 1)
    np.testing.assert_array_equal(b["observations"], obs_em)
    wl, wv = orc.net_forward(params, H, A, obs_em.reshape(E * T, 4, 84, 84))
    np.testing.assert_allclose(b["logits"].reshape(E * T, A), wl, atol=3e-2)  # bf16 operands + half storage
    np.testing.assert_allclose(b["values"].ravel(), wv, atol=3e-2)
    # actions were sampled from the fp32 logits BEFORE they were rounded for storage: check in-range and that the
    # stored half logits give the same action wherever the arg-max margin exceeds the rounding (tie-margin filter)
    sc = orc.softmax(b["logits"].reshape(E * T, A)) / noise.transpose(1, 0, 2).reshape(E * T, A)
    top = np.sort(sc, 1)
    clear = top[:, -1] > top[:, -2] * 1.01
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(b["actions"].ravel()[clear], sc.argmax(1)[clear])
    o = orc.buffer_get(rew.T, b["values"], b["next_values"], te.T, tr.T, st.T)
    np.testing.assert_array_equal(b["advantages"], _h(o["advantages"]))
    np.testing.assert_array_equal(b["returns"], _h(o["returns"]))
    lp = orc.log_softmax(b["logits"].reshape(E * T, A))
    np.testing.assert_allclose(b["log_probs"].reshape(E * T, A), lp, atol=2e-3, rtol=1e-3)  # one half ulp
    # mixed-precision update on the half planes vs the oracle's fp32 update on the same (rounded) batch
    m = eng.train(2.5e-4, 1, 1)
    w = orc.train(params, H, A, obs_em.reshape(E * T, 4, 84, 84), b["actions"].ravel(), b["log_probs"].reshape(E * T, A),
                  b["advantages"].ravel(), b["returns"].ravel(), b["masks"].ravel(), 1, 1)
    np.testing.assert_allclose(m["loss"], w["loss"], rtol=1e-2, atol=3e-2)
    np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=5e-2)
    g, wg = eng.export_grads(), w["last_grads"]
    cw = min(1.0, 0.5 / (float(w["grad_norm"][-1, -1]) + 1e-6))
    c0 = min(1.0, 0.5 / (float(m["grad_norm"][-1, -1]) + 1e-6))
    assert _rel(g / c0, wg / cw) < 3e-2
    # and against the bf16-emulating oracle on the same half planes (forward of the acting path, the update)
    c = bc.Checker()
    c.forward(b["logits"].reshape(E * T, A), b["values"].ravel(),
              bc.emulated_forward(params, H, A, obs_em.reshape(E * T, 4, 84, 84)), "act_")
    we = bc.emulated_train(params, H, A, obs_em.reshape(E * T, 4, 84, 84), b["actions"].ravel(),
                           b["log_probs"].reshape(E * T, A), b["advantages"].ravel(), b["returns"].ravel(),
                           b["masks"].ravel(), 1, 1)
    planes = {ours: eng.read_train_metric(ours, 1, 1, E * T) for ours, _ in bc.PLANES}
    c.train(H, A, m, planes, g, we, params0=params, params=eng.export_params())
    print(c.summary("fp16-rollout bf16 vs emulated oracle"))
    assert not c.failures, c.failures
    dev.free()
    eng.close()


def test_fp16_rollout_planes_set_batch_round_trip(pkg):
    """aleppo_set_batch into half planes rounds to nearest-even; the fp32 update path reads them back widened"""
    E, T, A, H = 8, 8, 4, 32
    N = E * T
    eng = pkg.Engine(E, T, A, H, rollout_precision=pkg.ROLLOUT_FP16)
    eng.load_params(hf.fill_params(1920, H, A))
    obs = hf.hf_bytes(1921, (N, 4, 84, 84))
    actions = (hf.hf_u32(1922, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(1923, (N, A), -1, 1))
    adv, ret = hf.hf_range(1924, (N,), -1, 1), hf.hf_range(1925, (N,), -1, 1)
    masks = (hf.hf_unit(1926, N) >= np.float32(0.1)).astype(np.uint8)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    np.testing.assert_array_equal(eng.read_batch("advantages").ravel(), _h(adv))
    np.testing.assert_array_equal(eng.read_batch("returns").ravel(), _h(ret))
    np.testing.assert_array_equal(eng.read_batch("log_probs").reshape(N, A), _h(old_lp))
    m = eng.train(2.5e-4, 1, 2)
    w = orc.train(hf.fill_params(1920, H, A), H, A, obs, actions, _h(old_lp), _h(adv), _h(ret), masks, 1, 2)
    np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4)  # fp32 network on the rounded planes: north-star bound
    np.testing.assert_allclose(eng.export_params(), w["params"], atol=1e-4)
    eng.close()


# ------------------------------------------------------------------ two ranks, real RCCL (needs >= 2 GPUs)
_DP_SCRIPT = r'''
import os, sys
root, rank, idfile, outdir, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import time
import numpy as np
import hashfill as hf, oracle_lib as orc
from __graft_entry__ import load_package
pkg = load_package()
WORLD, EG, T, M, H, A = 2, 8, 16, 2, 64, 6
if rank == 0:
    open(idfile + ".tmp", "wb").write(pkg.Engine.comm_unique_id()); os.replace(idfile + ".tmp", idfile)
t0 = time.time()
while not os.path.exists(idfile):
    assert time.time() - t0 < 120
    time.sleep(0.05)
uid = open(idfile, "rb").read()
N = WORLD * EG * T
obs = hf.hf_bytes(1801, (N, 4, 84, 84)); actions = (hf.hf_u32(1802, N) % np.uint32(A)).astype(np.int64)
old_lp = orc.log_softmax(hf.hf_range(1803, (N, A), -1, 1)); adv = hf.hf_range(1804, (N,), -1, 1)
ret = hf.hf_range(1805, (N,), -1, 1); masks = (hf.hf_unit(1806, N) >= np.float32(0.25)).astype(np.uint8)
rows = np.concatenate([np.arange(e * T, (e + 1) * T) for e in pkg.env_shard(WORLD * EG, WORLD, rank)])
eng = pkg.Engine(EG, T, A, H, precision=pkg.FP32 if mode == "fp32" else pkg.BF16, device=rank, world_size=WORLD,
                 rank=rank, advantage_norm=False)
eng.comm_init(uid)
eng.load_params(hf.fill_params(1810, H, A))
eng.set_batch(obs[rows], actions[rows], old_lp[rows], adv[rows], ret[rows], masks[rows])
m = eng.train(1e-3, 2, M)
np.savez(os.path.join(outdir, f"rank{rank}.npz"), params=eng.export_params(), loss=m["loss"], grad_norm=m["grad_norm"],
         mask_count=m["mask_count"], grads=eng.export_grads())
eng.close()
print("DP_RANK_OK", rank)
'''


def _gpu_count():
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


def test_two_rank_rccl_update_equals_one_rank_oracle(tmp_path):
    """The HIP data-parallel path with REAL RCCL on two GPUs (one process per GPU, started before either touches a
    device): bucketed gradient all-reduce on the side stream, global mask counts, replicated clip + Adam.  Parity
    definition of SURVEY 8(e): equals the 1-rank oracle on the batch whose minibatch k concatenates the ranks' local
    minibatch k; fp32 path, north-star bound 1e-4.  Skips on a one-GPU box."""
    if _gpu_count() < 2:
        pytest.skip("needs >= 2 GPUs (the round-end driver's node has 8)")
    script = tmp_path / "dp_rank.py"
    script.write_text(_DP_SCRIPT)
    idfile = str(tmp_path / "nccl_id.bin")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), idfile, str(tmp_path), "fp32"], env=env,
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
    WORLD, EG, T, M, H, A = 2, 8, 16, 2, 64, 6
    N = WORLD * EG * T
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    np.testing.assert_array_equal(r0["params"], r1["params"])  # replicated clip + Adam stay in lock-step
    np.testing.assert_array_equal(r0["grads"], r1["grads"])
    obs = hf.hf_bytes(1801, (N, 4, 84, 84)); actions = (hf.hf_u32(1802, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(1803, (N, A), -1, 1)); adv = hf.hf_range(1804, (N,), -1, 1)
    ret = hf.hf_range(1805, (N,), -1, 1); masks = (hf.hf_unit(1806, N) >= np.float32(0.25)).astype(np.uint8)
    B = EG * T // M
    order = np.concatenate([np.concatenate([np.arange(r * EG * T + k * B, r * EG * T + (k + 1) * B)
                                            for r in range(WORLD)]) for k in range(M)])
    w = orc.train(hf.fill_params(1810, H, A), H, A, obs[order], actions[order], old_lp[order], adv[order], ret[order],
                  masks[order], 2, M, lr=1e-3)
    np.testing.assert_allclose(r0["loss"], w["loss"], atol=1e-4)
    np.testing.assert_allclose(r0["grad_norm"], w["grad_norm"], rtol=1e-3)
    np.testing.assert_allclose(r0["params"], w["params"], atol=1e-4)
    np.testing.assert_allclose(r0["mask_count"][0], [masks[order][k * 2 * B:(k + 1) * 2 * B].sum() for k in range(M)])
