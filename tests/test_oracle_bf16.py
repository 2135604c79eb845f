"""The bf16 emulation of the CPU oracle (oracle.h, ORACLE_BF16) - CPU only.

1. its rounding helper against torch's float32 -> bfloat16 conversion (round-to-nearest-even) at every edge;
2. an independent restatement of the emulated network in torch float64 (conv2d / linear / torch.nn.grad, autograd for
   the loss) with explicit bf16 roundings at the rounding points of oracle.h: losses, every gradient tensor and the
   per-sample planes within 1e-5 relative;
3. the floor under the GPU bounds of bf16_check.py: the emulation with double sums against the same emulation with
   sequential fp32 sums - summation order being the only legitimate difference between a correct kernel and the
   emulation - sits well inside them;
4. the bounds have teeth: the checker fails an emulation whose conv3 reads one wrong tap for one output channel, and
   fails the plain fp32 oracle (so the tight bounds cannot be met without the emulation)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
from test_gpu_bf16_emulated import ROWS, sweep_batch


# ------------------------------------------------------------------ 1. rounding helper
def _torch_bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def test_round_bf16_edges_match_torch():
    edge = [
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,   # exact ties: even (down) / odd (up), both signs
        0x3F808001, 0x3F807FFF, 0x3F80FFFF,                # just above / below a tie, carry into the exponent
        0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,    # largest finite: stays, ties / rounds to inf
        0x7F800000, 0xFF800000,                            # +-inf
        0x00000000, 0x80000000,                            # +-0
        0x00000001, 0x80000001, 0x00007FFF, 0x00008000,    # fp32 subnormals: to zero / tie to even zero
        0x00018000, 0x00008001, 0x007FFFFF, 0x807F8000,    # into bf16's subnormal range, up to the smallest normal
        0x00800000, 0x3F800000, 0xC0490FDB,                # already exact / ordinary values
    ]
    x = _f(edge)
    got, want = orc.round_bf16(x), _torch_bf16(x)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert np.isinf(got[_bits(x) == 0x7F7FFFFF]).all()       # overflow
    assert _bits(got)[edge.index(0x80000000)] == 0x80000000  # -0 keeps its sign
    nan = _f([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFFFFFFFF])
    assert np.isnan(orc.round_bf16(nan)).all() and np.isnan(_torch_bf16(nan)).all()


def test_round_bf16_hashed_bit_patterns_match_torch():
    bits = hf.hf_u32(4242, 1_000_000)
    x = _f(bits)
    got, want = _bits(orc.round_bf16(x)), _bits(_torch_bf16(x))
    nan = np.isnan(x)
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert np.isnan(_f(got[nan])).all()
    assert (_bits(x)[~nan] & 0xFFFF != 0).mean() > 0.99  # almost every pattern actually rounds


# ------------------------------------------------------------------ 2. independent restatement in torch float64
def _batch(seed, H, A, N, p_mask=0.1):
    params = hf.fill_params(seed, H, A)
    obs = hf.hf_bytes(seed + 1, (N, 4, 84, 84))
    actions = (hf.hf_u32(seed + 2, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(seed + 3, (N, A), -1, 1))
    adv, ret = hf.hf_range(seed + 4, (N,), -1, 1), hf.hf_range(seed + 5, (N,), -1, 1)
    masks = (hf.hf_unit(seed + 6, N) >= np.float32(p_mask)).astype(np.uint8)
    masks[0] = 1
    return params, obs, actions, old_lp, adv, ret, masks


def _bf(x):
    """the device's (__bf16) cast of an fp32 value, as float64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _f32(x):
    return x.to(torch.float32).to(torch.float64)


def _restated_step(params, H, A, obs, actions, old_lp, adv, ret, masks, clip=0.1, c_v=0.5, c_e=0.01):
    """one minibatch of the bf16 update in float64 torch, rounding where oracle.h's table says the device stores
    bf16: returns (loss, pre-clip grad norm, flat unclipped gradient, per-sample planes)"""
    d = torch.float64
    t = [torch.from_numpy(p.copy()).to(d).reshape(s) for p, s in
         zip(np.split(params, orc.param_offsets(H, A)[1:-1]), hf.param_shapes(H, A))]
    W1, b1, W2, b2, W3, b3, Wfc, bfc, Wa, ba, Wv, bv = t
    W1b, W2b, W3b, Wfcb = _bf(W1), _bf(W2), _bf(W3), _bf(Wfc)
    x = torch.from_numpy(obs).to(d)  # byte values: 1/255 is conv1's epilogue scale
    s255 = float(np.float32(1.0) / np.float32(255.0))
    a1 = _bf(F.relu(F.conv2d(x, W1b, stride=4) * s255 + b1[None, :, None, None]))
    a2 = _bf(F.relu(F.conv2d(a1, W2b, stride=2) + b2[None, :, None, None]))
    a3 = _bf(F.relu(F.conv2d(a2, W3b, stride=1) + b3[None, :, None, None]))
    h = _f32(F.linear(a3.flatten(1), Wfcb, bfc))  # fp32, no rounding to bf16, no ReLU
    logits = _f32(F.linear(h, Wa, ba)).requires_grad_()
    value = _f32(F.linear(h, Wv, bv)[:, 0]).requires_grad_()
    # the PPO loss (ai/ppo/losses.cc), differentiated by autograd
    act = torch.from_numpy(actions)
    m = torch.from_numpy(masks).to(d)
    lp = torch.log_softmax(logits, 1)
    ent = -(lp.exp() * lp).sum(1)
    rho = torch.exp(lp.gather(1, act[:, None])[:, 0] - torch.from_numpy(old_lp).to(d).gather(1, act[:, None])[:, 0])
    A_ = torch.from_numpy(adv).to(d)
    obj = torch.minimum(rho * A_, rho.clamp(1 - clip, 1 + clip) * A_)
    lv = 0.5 * (value - torch.from_numpy(ret).to(d)) ** 2
    L = -obj + c_v * lv - c_e * ent
    loss = (L * m).sum() / m.sum()
    dz, dv = torch.autograd.grad(loss, (logits, value))
    dz, dv = _f32(dz), _f32(dv)  # dlogits / dvalue: fp32
    logits, value = logits.detach(), value.detach()
    # backward, rounding dh and every dz to bf16 (gated by the stored bf16 activation)
    dh = _bf(dz @ Wa + dv[:, None] * Wv)
    g = {"action.w": dz.T @ h, "action.b": dz.sum(0), "value.w": (dv @ h)[None], "value.b": dv.sum()[None],
         "fc.w": dh.T @ a3.flatten(1), "fc.b": dh.sum(0)}
    dz3 = _bf((dh @ Wfcb).reshape(a3.shape)) * (a3 > 0)
    g["conv3.w"] = torch.nn.grad.conv2d_weight(a2, W3.shape, dz3, stride=1)
    g["conv3.b"] = dz3.sum((0, 2, 3))
    dz2 = _bf(torch.nn.grad.conv2d_input(a2.shape, W3b, dz3, stride=1)) * (a2 > 0)
    g["conv2.w"] = torch.nn.grad.conv2d_weight(a1, W2.shape, dz2, stride=2)
    g["conv2.b"] = dz2.sum((0, 2, 3))
    dz1 = _bf(torch.nn.grad.conv2d_input(a1.shape, W2b, dz2, stride=2)) * (a1 > 0)
    g["conv1.w"] = torch.nn.grad.conv2d_weight(x, W1.shape, dz1, stride=4) * s255
    g["conv1.b"] = dz1.sum((0, 2, 3))
    flat = np.concatenate([g[nm].to(torch.float32).numpy().ravel() for nm in bc.NAMES])
    norm = np.sqrt(sum(float(np.linalg.norm(g[nm].to(torch.float32).numpy().astype(np.float64))) ** 2
                       for nm in bc.NAMES))
    planes = dict(total_losses=L, ratio=rho, entropies=ent, value_losses=lv, clipped=obj)
    return (float(loss), norm, flat, {k: v.detach().numpy() for k, v in planes.items()},
            (logits.numpy(), value.numpy()))


@pytest.mark.parametrize("H", [32, 512])
@pytest.mark.parametrize("A", [1, 4, 18])
def test_emulated_oracle_matches_a_torch_float64_restatement(H, A):
    N = 6
    params, obs, actions, old_lp, adv, ret, masks = _batch(6100 + 7 * A + H, H, A, N)
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, 1, emulate_bf16=True)
    loss, norm, g, planes, (logits, values) = _restated_step(params, H, A, obs, actions, old_lp, adv, ret, masks)
    assert abs(float(w["loss"][0, 0]) - loss) <= 1e-5 * max(abs(loss), 1e-3)
    assert abs(float(w["grad_norm"][0, 0]) / norm - 1) <= 1e-5
    wg = w["last_grads"] / bc._clip_coef(w["grad_norm"][0, 0])
    offs = orc.param_offsets(H, A)
    for k, nm in enumerate(bc.NAMES):
        assert bc.rel(wg[offs[k]:offs[k + 1]], g[offs[k]:offs[k + 1]]) <= 1e-5, nm
    for ours, theirs in bc.PLANES:
        assert bc.rel(w[theirs].ravel(), planes[theirs]) <= 1e-5, theirs
    wl, wv = orc.net_forward(params, H, A, obs, emulate_bf16=True)
    assert bc.rel(wl, logits) <= 1e-5 and bc.rel(wv, values) <= 1e-5
    # and the flag matters: the fp32 oracle is a different function (the restatement's roundings are not no-ops)
    w32 = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, 1)
    assert bc.rel(w32["last_grads"], w["last_grads"]) > 1e-4


# ------------------------------------------------------------------ 3 / 4. the floor under the bounds, and their teeth
@pytest.fixture(scope="module")
def floor_batch():
    H, A, N = 512, 4, 512
    return (H, A) + _batch(6300, H, A, N, p_mask=0.05)


def _run(H, A, params, obs, actions, old_lp, adv, ret, masks, fp32=False, reference=False):
    """one emulated (or, fp32=True, plain fp32) update plus the forward of the first 64 samples; reference=True: the
    emulation with its floor run, as the GPU tests use it"""
    if reference:
        return (bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, 1),
                bc.emulated_forward(params, H, A, obs[:64]))
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, 1, emulate_bf16=not fp32)
    return w, orc.net_forward(params, H, A, obs[:64], emulate_bf16=not fp32)


def _check(got, ref, params_got, params_ref, H, A):
    (w, (l, v)), (r, rf) = got, ref
    c = bc.Checker()
    planes = {ours: w[theirs] for ours, theirs in bc.PLANES}
    c.train(H, A, w, planes, w["last_grads"], r, params0=params_got, params=w["params"], ref_params0=params_ref)
    c.forward(l, v, rf)
    return c


def test_floor_run_sets_the_bounds(floor_batch):
    """the checker measures the floor run (fp32 sums) against the emulation (double sums) on the batch it checks and
    bounds every measurement by max(base, 4 x floor): the floor run itself passes at a quarter of every bound, and the
    two summation orders really differ"""
    H, A, params = floor_batch[:3]
    ref = _run(H, A, params, *floor_batch[3:], reference=True)
    floor = (ref[0]["floor_run"], ref[1][2])
    c = _check(floor, ref, params, params, H, A)
    print(c.summary("summation-order floor (N=512, H=512)"))
    assert not c.failures
    assert all(c.report[k] <= c.limits[k] / bc.FLOOR_FACTOR + 1e-12 for k in c.report)
    assert c.report["grad_conv1.w"] > 0


def test_bounds_catch_one_wrong_conv3_tap(floor_batch):
    """an emulation whose conv3 reads tap (0, 0) instead of tap (1, 1) for output channel 37 only (forward and data
    gradient, as a kernel with a wrong tap offset would): the checker must fail it"""
    H, A, params = floor_batch[:3]
    args = floor_batch[3:]
    ref = _run(H, A, params, *args, reference=True)
    bad = params.copy()
    o3 = orc.param_offsets(H, A)[4]
    W3 = bad[o3:o3 + 64 * 64 * 9].reshape(64, 64, 3, 3)
    W3[37, :, 1, 1] = W3[37, :, 0, 0]
    got = _run(H, A, bad, *args)
    c = _check(got, ref, bad, params, H, A)
    print(c.summary("one wrong conv3 tap"), c.failures)
    assert any(name == "chan_conv3.w" for name, _, _ in c.failures)


SWEEP = [r[:3] for r in ROWS if r[0] <= 1400] + [(512, 512, 4)]


@pytest.mark.parametrize("N,H,A", SWEEP)
def test_floor_derived_bounds_reject_the_fp32_oracle(N, H, A):
    """on the sweep's batches (where the GPU tests apply the bounds; N = 512 / H = 512 is the floor batch): the plain
    fp32 oracle fails the floor-derived bounds on the gradient tensors, i.e. the bounds cannot be met without the
    emulation even where the batch's floor widens them"""
    batch = sweep_batch(N, H, A) if N != 512 else _batch(6300, H, A, N, p_mask=0.05)
    params = batch[0]
    ref = _run(H, A, *batch, reference=True)
    got = _run(H, A, *batch, fp32=True)
    c = _check(got, ref, params, params, H, A)
    print(c.summary(f"fp32 oracle vs emulation N={N} H={H} A={A}"))
    assert any(name.startswith("grad_") and name != "grad_norm_rel" for name, _, _ in c.failures), c.failures
    if A > 1:  # the action head too (A = 1 has no policy gradient)
        assert any(name.startswith("grad_action") for name, _, _ in c.failures), c.failures
