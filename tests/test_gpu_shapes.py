"""Every hidden size and acting batch size against the oracles (pytest -m gpu on the MI355X; part C runs on the CPU).

aleppo_create takes any hidden size H = 32 .. 512 in steps of 32, any A in 1 .. 18 and any number of environments, and
the kernels pick their route from those numbers.  This module runs the routes the other tests leave out:

A. the update and the forward at every hidden size.
   * bf16, H = 32, 64, ..., 512 at N = 520 (past the 256-sample route threshold), plus N <= 256 at H in {32, 96, 160,
     480}, and OPT_FC_PIPE = 0 at H in {128, 192} (the pipelined fc forward with N below / not a multiple of its 128-wide
     tile).  H % 64 == 32 is where the fc data gradient falls back to gemm_nt_kernel with a K tail (bf16 stages 64 k per
     step) and where the Wfc -> WfcT repack of adam_kernel and the load-time transpose_cast_kernel have a partial 64-row
     tile; gemm_tn_kernel then runs the fc weight gradient with a partial M tile before reduce_slabs_kernel.  Each row
     checks the forward, a first update and a SECOND update on another batch against the bf16-emulating oracle
     (bf16_check).  The second update starts the oracle from the engine's own parameters and Adam state after the first
     (read with state_dict, nothing is loaded back), so its fc data gradient reads the WfcT that adam_kernel repacked -
     the only check that sees the partial-tile repack.
   * fp32 at H in {32, 96, 128, 224, 480}: 2 epochs x 2 minibatches against orc.train at the north-star bounds of
     test_gpu_parity.test_train_vs_oracle, the parameters and gradients on re-synchronised steps (see the test).
B. the acting path at E in {1, 255, 256, 257, 513, 4096}: act_conv_kernel launches min(E, CUs) workgroups and a
   workgroup loops over samples n, n + gridDim.x, ... with its weights in registers and the ingest recycling LDS.  The
   MI355X has 256 CUs, so E = 255 / 256 / 257 straddle one sample per workgroup, E = 513 gives up to 3 samples and
   E = 4096 (the reference's v1.yaml shape) 16.  The fused-ingest option, the frame kind and location, H, A, the
   generic convolutions and the precision are spread over the rows pairwise.  Each rollout's logits, values and
   next_values are checked against the emulated forward (bf16) or the fp32 oracle at 1e-4 (fp32); observation, flag,
   reward and action planes exactly, GAE planes bit-exact from the engine's values.
C. (CPU) the floor-derived bounds have teeth at every (N, H, A) of part A: the plain fp32 oracle fails them on a
   gradient, the floor run passes."""
import ctypes

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401
from test_gpu_at_size import DeviceBytes, _flags, _rollout_vs_oracle
from test_gpu_bf16_emulated import sweep_batch
from test_oracle_bf16 import _batch, _check, _run


# ------------------------------------------------------------------ A. the update and forward at every hidden size
A_CYCLE = (1, 4, 6, 9, 18)
# (N, H, A, OPT_FC_PIPE)
BF16_ROWS = [(520, H, A_CYCLE[i % len(A_CYCLE)], 1) for i, H in enumerate(range(32, 513, 32))]
BF16_ROWS += [(200, 32, 9, 1), (256, 96, 18, 1), (136, 160, 4, 1), (248, 480, 1, 1)]  # the small-tile fc routes
BF16_ROWS += [(520, 128, 9, 0), (520, 192, 1, 0)]  # the same batches as their OPT_FC_PIPE = 1 rows
FP32_ROWS = [(520, 32, 4), (520, 96, 18), (520, 128, 1), (520, 224, 6), (520, 480, 9)]
LR = 2.5e-4


# Measured and explained: a legitimate bf16 rounding flip two layers up, not a kernel fault.  On this row's second step
# conv3 output channel 47 (nearly dead: 168 of 12544 positions active) is 2.5e-2 from the emulation against a bound of
# 1e-2 (the floor run: 6.5e-5); every other check of the row is inside its bound.  The whole difference is ONE ReLU gate:
# masking the batch down to sample 124 leaves the engine's channel-47 gradient row equal to one a2 patch, at pixel (6, 5),
# times a scalar (residual 3e-5 relative) where the emulation's row is zero.  There the emulation's conv3 sum (before the
# bias) is 0.0176509 and the bias -0.0176758, so the gate is off by 2.5e-5; the engine's sum is 4.3e-5 higher, the same on
# the fused, sample-stationary and generic forward kernels.
# The cause, from the exported activations (tests/test_gpu_layers.py asserts every link on all three routes, each layer
# checked exactly on the engine's own previous layer): the exact conv1 pre-activation of a1 element (124, 10, 12, 16) lies
# 0.09 u Sa - a tenth of the error an fp32 sum of its 256 products has - from a bf16 rounding boundary, and the engine stores
# the boundary's other neighbour.  a2 element (124, 31, 6, 7) reads it and crosses a rounding boundary of its own (0.062988
# against the emulation's 0.063477; on the engine's a1 its exact value rounds to what the engine stores), and that one bf16
# ulp times its W3 tap of -0.0884 is the 4.3154e-5 that lifts the conv3 pre-activation from -2.49e-5 to +1.82e-5.  On the
# engine's own a2 the conv3 value is exactly bf16 of the exact sum.  No weight copy is involved.  The comparison of a whole
# chain against the emulation cannot tell such a flip from a fault, so the excuse stays as narrow as it was: only that
# measurement, up to 3e-2, is excused; anything else, or more, fails the row.
KNOWN_GAPS = {(256, 96, 18, 1): ("step2_chan_conv3.w", 3e-2,
                                 "one conv3 gate (sample 124, channel 47) off the emulation on every forward route")}


def _bid(r):
    return "N%d-H%d-A%d-pipe%d" % r


def _second_batch(N, H, A):
    """(obs, actions, old_lp, adv, ret, masks) of the second update: another batch of the same size"""
    return _batch(2900 + N + H, H, A, N)[1:]


def _train_planes(eng, N):
    return {ours: eng.read_train_metric(ours, 1, 1, N) for ours, _ in bc.PLANES}


@pytest.mark.gpu
@pytest.mark.parametrize("row", BF16_ROWS, ids=[_bid(r) for r in BF16_ROWS])
def test_bf16_every_hidden_size_vs_emulated_oracle(pkg, row):
    N, H, A, pipe = row
    params, *batch1 = sweep_batch(N, H, A)
    batch2 = _second_batch(N, H, A)
    eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
    eng.set_option(pkg.OPT_FC_PIPE, pipe)
    assert eng.get_option(pkg.OPT_FC_PIPE) == pipe
    eng.load_params(params)
    c = bc.Checker()
    # fc_fwd picks its route by the sample count: 333 > 256 on the N = 520 rows, all N (<= 256) on the others
    nf = min(N, 333)
    logits, values = eng.forward(batch1[0][:nf])
    c.forward(logits, values, bc.emulated_forward(params, H, A, batch1[0][:nf]), "fwd_")
    # step 1: the engine and the oracle on the loaded parameters (WfcT from the load-time transpose)
    eng.set_batch(*batch1)
    m = eng.train(LR, 1, 1)
    w = bc.emulated_train(params, H, A, *batch1, 1, 1, lr=LR)
    c.train(H, A, m, _train_planes(eng, N), eng.export_grads(), w, "step1_", params0=params,
            params=eng.export_params())
    # step 2 on another batch, the oracle re-synchronised to the engine's state (WfcT as adam_kernel repacked it)
    sd = eng.state_dict()
    assert int(sd["step"]) == 1
    eng.set_batch(*batch2)
    m = eng.train(LR, 1, 1)
    w = bc.emulated_train(sd["params"], H, A, *batch2, 1, 1, lr=LR,
                          adam=dict(m=sd["exp_avg"], v=sd["exp_avg_sq"], step=int(sd["step"])))
    c.train(H, A, m, _train_planes(eng, N), eng.export_grads(), w, "step2_", params0=sd["params"],
            params=eng.export_params())
    eng.close()
    print(c.summary("bf16 every-H " + _bid(row)))
    if row in KNOWN_GAPS and len(c.failures) == 1:
        name, cap, why = KNOWN_GAPS[row]
        if c.failures[0][0] == name and c.failures[0][1] <= cap:
            pytest.xfail("%s (a rounding flip in a1, see KNOWN_GAPS): %r" % (why, c.failures))
    assert not c.failures, c.failures


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,A", FP32_ROWS)
def test_fp32_every_hidden_size_vs_oracle(pkg, N, H, A):
    """the north-star bounds of test_gpu_parity.test_train_vs_oracle: forward 1e-4; one call of 2 epochs x 2 minibatches:
    loss 1e-4 and pre-clip norm 1e-3 relative on every minibatch; and every one of those four minibatch steps replayed
    from the oracle's own parameters and Adam state (load_state_dict): its gradients 1e-5 + 2e-3 max|g|, its parameters
    1e-4.  The replayed steps read the load-time transpose of Wfc, and loss / norm are too coarse to see a stale tile of
    the WfcT that adam_kernel repacks, so that repack is checked on its own: after the call, one more step on the engine
    and on a fresh engine loaded from its state_dict must give bit-identical gradients.
    Why re-synchronised: in the free-running call the two sides' parameters part by ~1e-5 after the first step and a
    PPO clip state or ReLU gate that sits on its edge then flips (a step of the gradient, not a drift); Adam turns the
    difference into up to 1.3e-4 on a parameter and 3.3e-4 on a last-minibatch gradient entry (measured at H = 32 /
    96), while every step taken on identical state stays within 3.5e-5 on the gradients and 9.2e-6 on the parameters"""
    params, obs, actions, old_lp, adv, ret, masks = sweep_batch(N, H, A)
    eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.FP32)
    eng.load_params(params)
    logits, values = eng.forward(obs[:333])
    wl, wv = orc.net_forward(params, H, A, obs[:333])
    np.testing.assert_allclose(logits, wl, atol=1e-4, rtol=0)
    np.testing.assert_allclose(values, wv, atol=1e-4, rtol=0)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    m = eng.train(LR, 2, 2)
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, 2, lr=LR)
    # one more step from the same state on the engine (WfcT as adam_kernel repacked it) and on a fresh engine loaded from
    # its state_dict (WfcT from the load-time transpose): identical gradients, bit for bit
    again = pkg.Engine(N // 8, 8, A, H, precision=pkg.FP32)
    again.load_state_dict(eng.state_dict())
    grads = []
    for e in (eng, again):
        e.set_batch(obs, actions, old_lp, adv, ret, masks)
        e.train(LR, 1, 1)
        grads.append(e.export_grads())
        e.close()
    np.testing.assert_array_equal(grads[0], grads[1])
    np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=1e-3)
    B, wp, adam, worst = N // 2, params, None, [0.0, 0.0]
    for step in range(4):  # epoch step // 2, minibatch step % 2 (contiguous minibatches)
        s = slice(step % 2 * B, (step % 2 + 1) * B)
        eng = pkg.Engine(B // 4, 4, A, H, precision=pkg.FP32)
        if adam is None:
            eng.load_params(wp)
        else:
            eng.load_state_dict(dict(params=wp, exp_avg=adam["m"], exp_avg_sq=adam["v"], step=adam["step"]))
        eng.set_batch(obs[s], actions[s], old_lp[s], adv[s], ret[s], masks[s])
        ms = eng.train(LR, 1, 1)
        ws = orc.train(wp, H, A, obs[s], actions[s], old_lp[s], adv[s], ret[s], masks[s], 1, 1, lr=LR, adam=adam)
        g, p = eng.export_grads(), eng.export_params()
        eng.close()
        np.testing.assert_allclose(ms["loss"], ws["loss"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(ms["grad_norm"], ws["grad_norm"], rtol=1e-3)
        wg = ws["last_grads"]
        np.testing.assert_allclose(g, wg, atol=1e-5 + 2e-3 * np.abs(wg).max(), rtol=0, err_msg=f"step {step + 1}")
        np.testing.assert_allclose(p, ws["params"], atol=1e-4, rtol=0, err_msg=f"step {step + 1}")
        worst = [max(worst[0], np.abs(g - wg).max() / (1e-5 + 2e-3 * np.abs(wg).max())),
                 max(worst[1], np.abs(p - ws["params"]).max() / 1e-4)]
        wp, adam = ws["params"], ws["adam"]
    print("fp32 every-H N=%d H=%d A=%d: loss %.3g of 1e-4, norm %.3g of 1e-3, re-synchronised steps: gradients %.3g, "
          "parameters %.3g of their bounds" % (N, H, A, np.abs(m["loss"] - w["loss"]).max(),
                                               np.abs(m["grad_norm"] / w["grad_norm"] - 1).max(), *worst))


# ------------------------------------------------------------------ B. the acting path across batch sizes
# E in {1, 255, 256, 257, 513, 4096} against the MI355X's 256 CUs: act_conv_kernel runs min(E, 256) workgroups, so
# E = 255 / 256 leave one sample per workgroup, E = 257 puts a second one on a single workgroup, E = 513 gives up to 3
# and E = 4096 (the reference's v1.yaml shape) 16 per workgroup - the `for (n += gridDim.x; ...)` loop body.
# (E, T, OPT_FUSED_ACT, frame kind, location, H, A, precision, OPT_GENERIC_CONV)
ACT_ROWS = [
    (1, 6, 2, "84", "host", 32, 1, "bf16", 0),
    (1, 5, 0, "raw", "device", 480, 18, "bf16", 0),
    (255, 3, 1, "raw", "mapped", 96, 4, "bf16", 0),
    (256, 3, 2, "raw", "device", 512, 18, "bf16", 1),
    (257, 3, 0, "84", "mapped", 480, 1, "bf16", 0),
    (257, 3, 1, "raw", "host", 96, 18, "fp32", 0),
    (513, 3, 2, "84", "host", 480, 4, "bf16", 0),
    (513, 2, 1, "raw", "device", 32, 18, "bf16", 0),
    (513, 2, 0, "raw", "host", 512, 1, "bf16", 1),
    (4096, 2, 1, "84", "device", 512, 4, "bf16", 0),
    (4096, 2, 2, "84", "mapped", 96, 18, "bf16", 0),
    (4096, 2, 0, "84", "host", 32, 1, "bf16", 0),
]


def _aid(r):
    return "E%d-T%d-fused%d-%s-%s-H%d-A%d-%s-gen%d" % r


@pytest.mark.gpu
@pytest.mark.parametrize("row", ACT_ROWS, ids=[_aid(r) for r in ACT_ROWS])
def test_rollout_every_batch_size_vs_oracle(pkg, row):
    E, T, fused, kind, loc, H, A, prec, generic = row
    seed = 3100 + E + H + A
    params = hf.fill_params(seed, H, A)
    raw = kind == "raw"
    per_env = 2 * 210 * 160 if raw else 84 * 84
    frames = hf.hf_bytes(seed + 1, (T, E, per_env))
    lut = ((np.arange(256) * 5 + 3) % 256).astype(np.uint8)
    te, tr, st = _flags(seed + 2, T, E, 0.2, 0.1)
    rew = hf.hf_range(seed + 3, (T, E), -3, 3)
    rng = np.random.default_rng(seed + 4)
    noise = rng.exponential(size=(T, E, A)).astype(np.float32)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=seed)
    for opt, val in ((pkg.OPT_FUSED_ACT, fused), (pkg.OPT_GENERIC_CONV, generic)):
        eng.set_option(opt, val)
        assert eng.get_option(opt) == val
    eng.load_params(params)
    eng.set_gray_lut(lut)
    fkind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    if loc == "host":  # the act / step loop with host frames (staged by the call)
        for t in range(T):
            eng.act(noise[t])
            eng.step(frames[t], rew[t], te[t], tr[t], st[t], kind=fkind)
    else:
        if loc == "device":
            buf = DeviceBytes(frames)
            addr, where = buf.addr, pkg.DEVICE
        else:
            addr, where = eng.host_alloc(frames.nbytes), pkg.HOST_MAPPED
            ctypes.memmove(addr, frames.ctypes.data, frames.nbytes)
        eng.replay_rollout(addr, fkind, E * per_env, rew, te, tr, st, noise=noise, location=where)
    eng.finish_rollout(rng.exponential(size=(E, A)).astype(np.float32))
    b = {k: eng.read_batch(k) for k in pkg.FIELDS}
    if loc == "device":
        buf.free()
    elif loc == "mapped":
        eng.host_free(addr)
    eng.close()
    np.testing.assert_array_equal(b["terminals"], te.T)
    np.testing.assert_array_equal(b["truncations"], tr.T)
    np.testing.assert_array_equal(b["rewards"], np.clip(rew.T, -1, 1))
    f84 = np.stack([orc.preprocess(frames[t].reshape(E, 2, 210, 160), lut) for t in range(T)]) if raw else \
        frames.reshape(T, E, 84, 84)
    obs0 = np.zeros((E, 4, 84, 84), np.uint8)
    if prec == "bf16":
        c = bc.Checker()
        last = _rollout_vs_oracle(b, f84, st, rew, te, tr, obs0, params, H, A, None, noise=noise, checker=c)
        print(c.summary("rollout " + _aid(row)))
        assert not c.failures, c.failures
    else:
        last = _rollout_vs_oracle(b, f84, st, rew, te, tr, obs0, params, H, A, 1e-4, noise=noise)
    np.testing.assert_array_equal(b["current_obs"], last)
    assert b["observations"].any()


# ------------------------------------------------------------------ C. the bounds have teeth at every row of part A
TEETH = sorted({r[:3] for r in BF16_ROWS})


@pytest.mark.parametrize("N,H,A", TEETH)
def test_floor_derived_bounds_reject_the_fp32_oracle_at_every_hidden_size(N, H, A):
    """on part A's first-update batches: the plain fp32 oracle fails the floor-derived bounds on a gradient tensor or
    channel (so the GPU rows cannot pass without the bf16 rounding points), and the floor run (the emulation with fp32
    sums) passes them"""
    batch = sweep_batch(N, H, A)
    params = batch[0]
    ref = _run(H, A, *batch, reference=True)
    c = _check(_run(H, A, *batch, fp32=True), ref, params, params, H, A)
    print(c.summary(f"fp32 oracle vs emulation N={N} H={H} A={A}"))
    assert any(name.startswith(("grad_", "chan_")) and name != "grad_norm_rel" for name, _, _ in c.failures), \
        c.failures
    floor = _check((ref[0]["floor_run"], ref[1][2]), ref, params, params, H, A)
    assert not floor.failures, floor.failures
