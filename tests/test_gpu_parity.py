"""Parity tests proper (run on the MI355X: pytest -m gpu).  Every check goes through the C ABI of
libaleppo.so (via the ctypes host mirror) and compares with
  * the reference's golden outputs (tests/golden/ref_golden.npz, from the compiled reference), and
  * the pinned CPU oracle (oracle/) on the same seeded inputs.
Tolerances: integer / byte / index work bit-exact; fp32 1e-4 (north star), tighter where the
arithmetic is order-identical; bf16 bounds are stated where used.
"""
import os
import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
from conftest import GAE_KATS, gae_kat_expected
from shared_fixtures import pkg  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ GAE (reads like test/ai/gae-test.cc)
@pytest.mark.parametrize("k", range(6))
def test_gae_known_answers(pkg, golden, k):
    r, v, nv, te, tr, st = GAE_KATS[k]
    adv = np.zeros(np.shape(r), np.float32)
    pkg.gae.gae(adv, r, v, nv, te, tr, st, 0.99, 0.95)
    np.testing.assert_allclose(adv, gae_kat_expected(r, v, nv, te, tr, st), atol=1e-5)
    np.testing.assert_allclose(adv, golden[f"kat{k}_adv"], atol=1e-6)


def test_gae_rejects_overlapping_flags(pkg):
    with pytest.raises(pkg.AleppoInvalidArgument, match="mutually exclusive"):
        pkg.gae.gae(np.zeros((1, 2), np.float32), [[1, 1]], [[0, 0]], [0], [[1, 0]], [[0, 0]], [[1, 0]], 0.99, 0.95)


def test_gae_g1_matches_reference_buffer_get(pkg, golden):
    r, v, nv, te, tr, st = hf.g1_inputs()
    adv = np.zeros_like(r)
    pkg.gae.gae(adv, np.clip(r, -1, 1), v, nv, te, tr, st, 0.99, 0.95)
    np.testing.assert_allclose(adv, golden["g1_adv"], atol=2e-6)
    np.testing.assert_array_equal(adv, orc.gae(np.clip(r, -1, 1), v, nv, te, tr, st))  # same op order: bit-exact


def test_gae_does_not_clamp_rewards(pkg):
    """ai::gae::gae uses the rewards as given (the clamp belongs to Buffer::get, buffer.cc:67): rewards outside [-1, 1]
    through the same production kernel with its clamp switched off"""
    r, v, nv, te, tr, st = hf.g1_inputs()
    assert np.abs(r).max() > 1
    adv = np.zeros_like(r)
    pkg.gae.gae(adv, r, v, nv, te, tr, st, 0.99, 0.95)
    np.testing.assert_array_equal(adv, orc.gae(r, v, nv, te, tr, st))


def test_gae_ragged_shapes(pkg):
    # aleppo_gae runs the rollout's gae_kernel: T % 16 steps one at a time, then double-buffered 16-step chunks
    # (T = 33: 1 + 2 chunks; 48: 3 chunks, both register sets twice; 128 in G1: 8 chunks; 7: tail only)
    for E, T in [(1, 1), (3, 7), (65, 5), (130, 33), (70, 41), (5, 48), (64, 16), (200, 17)]:
        r = hf.hf_range(11, (E, T), -1, 1)
        v = hf.hf_range(12, (E, T), -1, 1)
        nv = hf.hf_range(13, (E,), -1, 1)
        u = hf.hf_unit(14, E * T).reshape(E, T)
        te = (u < 0.05).astype(np.uint8)
        tr = ((u >= 0.05) & (u < 0.08)).astype(np.uint8)
        st = ((u >= 0.08) & (u < 0.12)).astype(np.uint8)
        adv = np.zeros((E, T), np.float32)
        pkg.gae.gae(adv, r, v, nv, te, tr, st, 0.99, 0.95)
        np.testing.assert_array_equal(adv, orc.gae(r, v, nv, te, tr, st))


# ------------------------------------------------------------------ vision (reads like test/ai/vision-test.cc)
def test_vision_constant_preservation(pkg):
    out = pkg.vision.resize_frame_stacked_grayscale_images(np.ones((1, 1, 210, 160), np.float32))
    assert out.shape == (1, 1, 84, 84) and (out == 1).all()
    inp = np.stack([np.full((210, 160), i, np.float32) for i in range(4)])[None]
    out = pkg.vision.resize_frame_stacked_grayscale_images(inp)
    assert out.shape == (1, 4, 84, 84) and out.dtype == np.float32
    for i in range(4):
        assert (out[0, i] == i).all()


def test_vision_g7(pkg, golden):
    inp = hf.hf_bytes(701, (1, 2, 210, 160)).astype(np.float32)
    np.testing.assert_allclose(pkg.vision.resize_frame_stacked_grayscale_images(inp), golden["g7_area"], rtol=1e-6,
                               atol=1e-4)
    rgb = hf.hf_bytes(702, (1, 1, 3, 84, 84)).astype(np.float32)
    np.testing.assert_allclose(pkg.vision.rgb_to_grayscale_frame_stacked_images(rgb), golden["g7_luma"], rtol=1e-6,
                               atol=1e-4)


def test_preprocess_bit_exact(pkg):
    raw = hf.hf_bytes(711, (5, 2, 210, 160))
    lut = ((np.arange(256) * 7 + 3) % 256).astype(np.uint8)
    np.testing.assert_array_equal(pkg.vision.preprocess(raw, lut), orc.preprocess(raw, lut))
    np.testing.assert_array_equal(pkg.vision.preprocess(raw), orc.preprocess(raw))
    flat = np.full((1, 2, 210, 160), 77, np.uint8)  # constants survive (vision-test.cc property)
    assert (pkg.vision.preprocess(flat) == 77).all()


# ------------------------------------------------------------------ frame stack
def _planes(obs):
    o = obs.reshape(obs.shape[0], obs.shape[1], -1).astype(np.int64)
    w = np.arange(1, o.shape[2] + 1, dtype=np.int64)
    return np.stack([o.sum(-1), (o * w).sum(-1)], -1)


def test_frame_stack_g6(pkg, golden):
    E = 4
    obs = np.zeros((E, 4, 84, 84), np.uint8)
    for step in range(6):
        frames = hf.hf_bytes(601 + step, (E, 84, 84))
        start = np.array([step == 0 or (step == 3 and e == 1) or (step == 4 and e == 2) for e in range(E)], np.uint8)
        obs = pkg.rollout.update_observations(obs, frames, start)
        np.testing.assert_array_equal(_planes(obs), golden["g6_checksums"][step])
    np.testing.assert_array_equal(obs[1], golden["g6_final_obs_env1"])


# ------------------------------------------------------------------ PPO loss
@pytest.mark.parametrize("A", [4, 6])
def test_losses_g2(pkg, golden, A):
    B = 256
    logits = hf.hf_range(201 + A, (B, A), -2, 2)
    actions = (hf.hf_u32(205 + A, B) % np.uint32(A)).astype(np.int64)
    masks = (hf.hf_unit(209, B) >= np.float32(0.05)).astype(np.uint8)
    s = f"g2_A{A}_"
    o = pkg.losses.compute(logits, golden[s + "old_logp"], actions, hf.hf_range(206, (B,), -2, 2),
                           hf.hf_range(207, (B,), -1, 1), hf.hf_range(208, (B,), -1.5, 1.5), masks, 0.1, 0.5, 0.01)
    np.testing.assert_allclose(o.loss[0], golden[s + "loss"][0], atol=1e-5)
    for k, g in (("clipped_losses", "clipped"), ("value_losses", "value_losses"), ("entropies", "entropies"),
                 ("total_losses", "total_losses"), ("ratio", "ratio")):
        np.testing.assert_allclose(getattr(o, k), golden[s + g], atol=1e-5, err_msg=k)
    np.testing.assert_allclose(o.dlogits, golden[s + "dlogits"], atol=1e-6)
    np.testing.assert_allclose(o.dvalues, golden[s + "dvalues"], atol=1e-7)


def test_losses_all_masked_and_single_row(pkg):
    o = pkg.losses.compute([[0.1, 0.2, 0.3, 0.4]], orc.log_softmax([[0., 0., 0., 0.]]), [2], [1.0], [0.5], [1.0],
                           [1], 0.2, 0.5, 0.01)
    w = orc.ppo_loss([[0.1, 0.2, 0.3, 0.4]], orc.log_softmax([[0., 0., 0., 0.]]), [2], [1.0], [0.5], [1.0], [1],
                     0.2, 0.5, 0.01)
    np.testing.assert_allclose(o.loss[0], w["loss"], atol=1e-6)
    np.testing.assert_allclose(o.dlogits, w["dlogits"], atol=1e-6)


# ------------------------------------------------------------------ sampling: integer indices bit-exact
@pytest.mark.parametrize("A", [4, 6])
def test_sampling_g5_bit_exact(pkg, golden, A):
    s = f"g5_A{A}_"
    np.testing.assert_array_equal(pkg.sampling.multinomial_with_noise(golden[s + "probs"], golden[s + "q"]),
                                  golden[s + "actions"])


@pytest.mark.parametrize("A", [1, 9, 18])
def test_sampling_and_losses_wide_action_sets_vs_oracle(pkg, A):
    """The reference's golden vectors hold A = 4 and 6 (Breakout, Pong); the full ALE action set has 18 and takes the
    third instantiation of the head kernels.  Same checks against the pinned oracle: sampled indices bit-exact, loss
    terms and gradients to 1e-5 / 1e-6.  A = 1 is the degenerate single-action policy."""
    E, B = 333, 200
    probs = orc.softmax(hf.hf_range(960 + A, (E, A), -3, 3))
    q = np.maximum(hf.hf_unit(961 + A, E * A).reshape(E, A), np.float32(1e-7))
    np.testing.assert_array_equal(pkg.sampling.multinomial_with_noise(probs, q), orc.sample(probs, q))
    logits = hf.hf_range(962 + A, (B, A), -2, 2)
    actions = (hf.hf_u32(963 + A, B) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(964 + A, (B, A), -2, 2))
    adv, val, ret = hf.hf_range(965, (B,), -2, 2), hf.hf_range(966, (B,), -1, 1), hf.hf_range(967, (B,), -1.5, 1.5)
    masks = (hf.hf_unit(968, B) >= np.float32(0.05)).astype(np.uint8)
    o = pkg.losses.compute(logits, old_lp, actions, adv, val, ret, masks, 0.1, 0.5, 0.01)
    w = orc.ppo_loss(logits, old_lp, actions, adv, val, ret, masks, 0.1, 0.5, 0.01)
    np.testing.assert_allclose(o.loss[0], w["loss"], atol=1e-5)
    np.testing.assert_allclose(o.dlogits, w["dlogits"], atol=1e-6)
    np.testing.assert_allclose(o.dvalues, w["dvalues"], atol=1e-7)


# ------------------------------------------------------------------ network forward
@pytest.mark.parametrize("H,A", [(32, 4), (32, 6), (512, 4), (512, 6)])
def test_forward_g3_fp32(pkg, golden, H, A):
    eng = pkg.Engine(8, 1, A, H, precision=pkg.FP32)
    eng.load_params(hf.fill_params(310, H, A))
    np.testing.assert_allclose(eng.export_params(), hf.fill_params(310, H, A), atol=0)  # layout round trip
    logits, values = eng.forward(hf.hf_bytes(301, (8, 4, 84, 84)))
    np.testing.assert_allclose(logits, golden[f"g3_H{H}_A{A}_logits"], atol=1e-4)
    np.testing.assert_allclose(values, golden[f"g3_H{H}_A{A}_values"], atol=1e-4)
    eng.close()


def test_forward_bf16_close(pkg, golden):
    # bf16 operands (8-bit mantissa), fp32 accumulate: documented looser bound 3e-2 abs on O(1) outputs
    H, A = 512, 6
    eng = pkg.Engine(8, 1, A, H, precision=pkg.BF16)
    eng.load_params(hf.fill_params(310, H, A))
    logits, values = eng.forward(hf.hf_bytes(301, (8, 4, 84, 84)))
    np.testing.assert_allclose(logits, golden[f"g3_H{H}_A{A}_logits"], atol=3e-2)
    np.testing.assert_allclose(values, golden[f"g3_H{H}_A{A}_values"], atol=3e-2)
    # and the bf16-emulating oracle at the tight bounds of bf16_check.py
    c = bc.Checker()
    c.forward(logits, values, bc.emulated_forward(hf.fill_params(310, H, A), H, A, hf.hf_bytes(301, (8, 4, 84, 84))))
    assert not c.failures, c.failures
    eng.close()


def test_forward_ragged_batch_vs_oracle(pkg):
    H, A, n = 64, 5, 37  # n not a multiple of any tile
    params = hf.fill_params(77, H, A)
    obs = hf.hf_bytes(78, (n, 4, 84, 84))
    eng = pkg.Engine(n, 1, A, H, precision=pkg.FP32)
    eng.load_params(params)
    logits, values = eng.forward(obs)
    wl, wv = orc.net_forward(params, H, A, obs)
    np.testing.assert_allclose(logits, wl, atol=1e-4)
    np.testing.assert_allclose(values, wv, atol=1e-4)
    eng.close()


# ------------------------------------------------------------------ full update vs the reference's train()
def _g4_inputs(golden):
    N, A = 64, 4
    return (hf.hf_bytes(401, (N, 4, 84, 84)), (hf.hf_u32(402, N) % np.uint32(A)).astype(np.int64), golden["g4_old_logp"],
            hf.hf_range(404, (N,), -1, 1), hf.hf_range(405, (N,), -1, 1),
            (hf.hf_unit(406, N) >= np.float32(0.1)).astype(np.uint8))


@pytest.mark.parametrize("name,epochs,M", [("a", 1, 1), ("b", 2, 4)])
def test_train_g4_fp32(pkg, golden, name, epochs, M):
    H, A, N = 32, 4, 64
    obs, actions, old_lp, adv, ret, masks = _g4_inputs(golden)
    eng = pkg.Engine(8, 8, A, H, precision=pkg.FP32)  # E*T = 64 samples
    eng.load_params(hf.fill_params(410, H, A))
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    m = eng.train(2.5e-4, epochs, M)
    s = f"g4{name}_"
    B = N // M
    np.testing.assert_allclose(m["loss"], golden[s + "loss"], atol=1e-4)
    np.testing.assert_allclose(m["grad_norm"], golden[s + "grad_norm"], rtol=1e-4)
    for ours, ref in (("total_losses", "total_losses"), ("ratio", "ratio"), ("entropies", "entropies"),
                      ("value_losses", "value_losses"), ("clipped_losses", "clipped")):
        np.testing.assert_allclose(eng.read_train_metric(ours, epochs, M, B), golden[s + ref], atol=1e-4,
                                   err_msg=ours)
    p = eng.export_params()
    g = eng.export_grads()
    offs = orc.param_offsets(H, A)
    shapes = hf.param_shapes(H, A)
    for k in range(12):
        pk = p[offs[k]:offs[k + 1]].astype(np.float64)
        gk = g[offs[k]:offs[k + 1]].astype(np.float64)
        idx = (hf.hf_u32(499, 64) % np.uint32(pk.size)).astype(np.int64)
        np.testing.assert_allclose(pk[idx], golden[s + "param_samples"][k], atol=1e-4, err_msg=f"param {k}")
        np.testing.assert_allclose(gk[idx], golden[s + "grad_samples"][k], atol=2e-5, rtol=2e-3, err_msg=f"grad {k}")
        np.testing.assert_allclose((gk * gk).sum(), golden[s + "grad_sums"][k][1], rtol=5e-3, atol=1e-9)
    for k in (0, 1, 3, 5, 7, 8, 9, 10, 11):
        np.testing.assert_allclose(p[offs[k]:offs[k + 1]].reshape(shapes[k]), golden[s + f"param{k}"], atol=1e-4)
    eng.close()


@pytest.mark.parametrize("prec,H,A,N,M", [("fp32", 512, 6, 96, 2), ("fp32", 64, 4, 40, 1), ("bf16", 512, 4, 96, 2),
                                          ("fp32", 64, 18, 40, 1), ("fp32", 512, 9, 96, 2), ("bf16", 512, 18, 96, 2)])
def test_train_vs_oracle(pkg, prec, H, A, N, M):
    params = hf.fill_params(510, H, A)
    obs = hf.hf_bytes(511, (N, 4, 84, 84))
    actions = (hf.hf_u32(512, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(513, (N, A), -1, 1))
    adv = hf.hf_range(514, (N,), -1, 1)
    ret = hf.hf_range(515, (N,), -1, 1)
    masks = (hf.hf_unit(516, N) >= np.float32(0.1)).astype(np.uint8)
    eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.FP32 if prec == "fp32" else pkg.BF16)
    eng.load_params(params)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    m = eng.train(2.5e-4, 2, M)
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M)
    # fp32: north-star 1e-4.  bf16 operands: documented looser bound (1% relative + 3e-2 absolute)
    np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4 if prec == "fp32" else 3e-2,
                               rtol=0 if prec == "fp32" else 1e-2)
    np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=1e-3 if prec == "fp32" else 5e-2)
    if prec == "fp32":
        np.testing.assert_allclose(eng.export_params(), w["params"], atol=1e-4)
        g, wg = eng.export_grads(), w["last_grads"]
        np.testing.assert_allclose(g, wg, atol=1e-5 + 2e-3 * np.abs(wg).max())
    else:  # bf16: every minibatch's loss / norm / planes and the whole update against the bf16-emulating oracle
        we = bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M)
        c = bc.Checker()
        planes = {ours: eng.read_train_metric(ours, 2, M, N // M) for ours, _ in bc.PLANES}
        c.train(H, A, m, planes, None, we, params0=params, params=eng.export_params())
        print(c.summary(f"train bf16 H={H} A={A} vs emulated oracle"))
        assert not c.failures, c.failures
    eng.close()


@pytest.mark.parametrize("N", [200, 1400])
def test_bf16_patch_kernels_match_generic_kernels(pkg, N):
    """the sample-stationary bf16 conv kernels and the generic gather-GEMMs compute the same bf16 math
    (only the fp32 summation order differs): forward, losses, gradient norm and gradients agree tightly.
    N = 200 -> 100-sample minibatches (acting-size kernel variants, ragged vs every group size: 2, 3, 8 samples per
    group); N = 1400 -> 700-sample minibatches (the training variants: static / unrolled atom loops, preloaded
    gates, two register sets, ragged last groups)."""
    H, A, M = 512, 6, 2
    params = hf.fill_params(710, H, A)
    obs = hf.hf_bytes(711, (N, 4, 84, 84))
    actions = (hf.hf_u32(712, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(713, (N, A), -1, 1))
    adv, ret = hf.hf_range(714, (N,), -1, 1), hf.hf_range(715, (N,), -1, 1)
    masks = (hf.hf_unit(716, N) >= np.float32(0.1)).astype(np.uint8)
    res = {}
    for generic in (1, 0):
        eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
        eng.set_generic_conv(generic)
        eng.load_params(params)
        logits, values = eng.forward(obs[:77])
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 1, M)
        res[generic] = (logits, values, m, eng.export_grads(), eng.export_params())
        eng.close()
    # each route on its own against the bf16-emulating oracle (two kernels that share a mistake agree with each other):
    # forward, both minibatches' loss / norm, the update; the exported gradients belong to the second minibatch, i.e. to
    # parameters that already differ by one step's rounding, where a 100-sample minibatch's clip states can flip - the
    # gradients themselves are compared on identical parameters in test_gpu_bf16_emulated.py
    we = bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, M)
    ef = bc.emulated_forward(params, H, A, obs[:77])
    for generic, (lg, vl, mm, gg, pp) in res.items():
        c = bc.Checker()
        c.forward(lg, vl, ef)
        c.train(H, A, mm, {}, None, we, params0=params, params=pp)
        print(c.summary(f"generic={generic} N={N} vs emulated oracle"))
        assert not c.failures, (generic, c.failures)
    (l1, v1, m1, g1, p1), (l0, v0, m0, g0, p0) = res[1], res[0]
    np.testing.assert_allclose(l0, l1, atol=2e-3)
    np.testing.assert_allclose(v0, v1, atol=2e-3)
    np.testing.assert_allclose(m0["loss"], m1["loss"], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(m0["grad_norm"], m1["grad_norm"], rtol=5e-3)
    np.testing.assert_allclose(g0, g1, atol=5e-3 * np.abs(g1).max())
    if N > 200:
        return
    # and both stay within the documented bf16 bound of the fp32 oracle
    w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, M)
    np.testing.assert_allclose(m0["loss"], w["loss"], rtol=1e-2, atol=3e-2)
    np.testing.assert_allclose(m0["grad_norm"], w["grad_norm"], rtol=5e-2)
    cw = min(1.0, 0.5 / (float(w["grad_norm"][0, -1]) + 1e-6))
    c0 = min(1.0, 0.5 / (float(m0["grad_norm"][0, -1]) + 1e-6))
    np.testing.assert_allclose(g0 / c0, w["last_grads"] / cw, atol=3e-2 * np.abs(w["last_grads"] / cw).max())


@pytest.mark.parametrize("N", [8, 200, 1400, 4104])
def test_bf16_fused_forward_is_bit_identical_to_the_three_launches(pkg, N):
    """csrc/conv_fwd_fused.hpp (conv1 -> conv2 -> conv3 of a sample in one workgroup, a1 / a2 handed over in LDS; hot loop in
    inline assembly with hand-counted waits) against the three sample-stationary forward launches it replaces
    (ALEPPO_OPT_FUSED_FWD = 0): the same MFMA k-order per output, so logits, values, losses, every gradient and the
    updated parameters must be IDENTICAL bits.  A stale fragment, an early `vmcnt` on the prefetched stack or a wrong a1 /
    a2 copy for the backward pass shows up here.  N = 8: fewer samples than workgroups; 200 / 1400: 100- / 700-sample
    minibatches (ragged last round of the persistent loop); 4104: 2052 samples = 8 full rounds + 4 on a 256-CU part."""
    H, A, M = 512, 6, 2
    params = hf.fill_params(720, H, A)
    obs = hf.hf_bytes(721, (N, 4, 84, 84))
    actions = (hf.hf_u32(722, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(723, (N, A), -1, 1))
    adv, ret = hf.hf_range(724, (N,), -1, 1), hf.hf_range(725, (N,), -1, 1)
    masks = (hf.hf_unit(726, N) >= np.float32(0.1)).astype(np.uint8)
    res = {}
    for fused in (1, 0):
        eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
        eng.set_option(pkg.OPT_FUSED_FWD, fused)
        assert eng.get_option(pkg.OPT_FUSED_FWD) == fused
        eng.load_params(params)
        logits, values = eng.forward(obs[:min(N, 333)])
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 2, M)
        res[fused] = (logits, values, m["loss"], m["grad_norm"], eng.export_grads(), eng.export_params())
        eng.close()
    for a, b, what in zip(res[1], res[0], ("logits", "values", "loss", "grad_norm", "grads", "params")):
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


@pytest.mark.parametrize("N,A", [(8, 6), (200, 6), (1400, 4), (4104, 18)])
def test_bf16_fused_backward_matches_the_three_launches(pkg, N, A):
    """csrc/conv_bwd_fused.hpp (opt-in, ALEPPO_OPT_FUSED_BWD: conv2 dgrad + conv2 wgrad + conv1 wgrad of a sample in one
    workgroup, dz1 never leaves the CU) against the three launches of the default schedule: dz1 is the same bits, so the
    gradients differ only by the fp32 summation order of the weight-gradient slabs (other sample -> workgroup assignment):
    every tensor to 1e-6 relative L2, losses and norm to 1e-6, parameters after two updates to 1e-6 absolute.  N = 8: fewer
    samples than workgroups; 200 / 1400: 100- / 700-sample minibatches (ragged last round); 4104: 8 full rounds + 4."""
    H, M = 512, 2
    params = hf.fill_params(730, H, A)
    obs = hf.hf_bytes(731, (N, 4, 84, 84))
    actions = (hf.hf_u32(732, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(733, (N, A), -1, 1))
    adv, ret = hf.hf_range(734, (N,), -1, 1), hf.hf_range(735, (N,), -1, 1)
    masks = (hf.hf_unit(736, N) >= np.float32(0.1)).astype(np.uint8)
    res = {}
    for fused in (2, 0):  # (2: also below the 2048-sample minibatches the default fuses at)
        eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
        eng.set_option(pkg.OPT_FUSED_BWD, fused)
        assert eng.get_option(pkg.OPT_FUSED_BWD) == fused
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m1 = eng.train(2.5e-4, 1, 1)  # one minibatch: the exported gradients of both runs belong to identical parameters
        g = eng.export_grads()
        m2 = eng.train(2.5e-4, 1, M)
        res[fused] = (m1["loss"], m1["grad_norm"], g, m2["loss"], eng.export_params())
        eng.close()
    (l1, n1, g1, k1, p1), (l0, n0, g0, k0, p0) = res[2], res[0]
    assert np.array_equal(l1, l0)  # the forward pass is untouched
    np.testing.assert_allclose(n1, n0, rtol=1e-6)
    o = 0
    for name, sz in (("w1", 32 * 4 * 8 * 8), ("b1", 32), ("w2", 64 * 32 * 16), ("b2", 64), ("w3", 64 * 64 * 9), ("b3", 64)):
        a, b = g1[o:o + sz], g0[o:o + sz]
        assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b) + 1e-12, name
        o += sz
    assert np.linalg.norm(g1 - g0) <= 1e-6 * np.linalg.norm(g0)
    np.testing.assert_allclose(k1, k0, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(p1, p0, atol=1e-6)


@pytest.mark.parametrize("N,M", [(8, 2), (8, 1), (24, 2), (264, 1), (520, 1), (1032, 1), (3080, 1)])
def test_bf16_conv1_weight_gradient_ragged_sizes(pkg, N, M):
    """conv1's weight / bias gradient from the tap-shift kernel (csrc/conv1_wgrad.hpp: half-sample groups dealt to
    <= 256 workgroups, four groups in flight, consumers skip groups past the end) against the generic gather-GEMM on the
    same bf16 operands, per tensor, at minibatch sizes that exercise every tail: fewer groups than workgroups (4, 8, 12
    samples), one group more than the workgroups (264 samples -> 528 groups: 2 or 3 per workgroup), group counts of
    4k + 1 .. 4k + 3 per workgroup (520, 1032, 3080 samples)."""
    H, A = 512, 4
    params = hf.fill_params(1210, H, A)
    obs = hf.hf_bytes(1211, (N, 4, 84, 84))
    actions = (hf.hf_u32(1212, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(1213, (N, A), -1, 1))
    adv, ret = hf.hf_range(1214, (N,), -1, 1), hf.hf_range(1215, (N,), -1, 1)
    masks = np.ones(N, np.uint8)
    offs = orc.param_offsets(H, A)
    res = {}
    for generic in (1, 0):
        eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
        eng.set_generic_conv(generic)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 1, M)
        res[generic] = (eng.export_grads(), m)
        eng.close()
    # each route against the bf16-emulating oracle, per tensor and per channel, where the exported gradients belong to
    # the first step (M = 1: identical parameters); with M = 2 the first minibatch's gradient norm
    we = bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 1, M)
    for generic, (g, m) in res.items():
        c = bc.Checker()
        if M == 1:
            c.train(H, A, m, {}, g, we)
        else:  # the first minibatch's loss and norm (the engine's metrics, both sides on identical parameters)
            first = {k: m[k][:, :1] for k in ("loss", "grad_norm")}
            c.train(H, A, first, {}, None, dict(loss=we["loss"][:, :1], grad_norm=we["grad_norm"][:, :1],
                                                floor_run={k: we["floor_run"][k][:, :1] for k in ("loss", "grad_norm")}))
        assert not c.failures, (generic, c.failures)
    (g1, m1), (g0, m0) = res[1], res[0]
    n1, n0 = m1["grad_norm"], m0["grad_norm"]
    np.testing.assert_allclose(n0, n1, rtol=5e-3)
    for k, name in ((0, "conv1.w"), (1, "conv1.b")):
        a, b = g0[offs[k]:offs[k + 1]], g1[offs[k]:offs[k + 1]]
        rel = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
        # same bf16 operands, different fp32 summation order (and bf16 dz1 produced by different conv2 dgrad kernels)
        assert rel <= 1e-2, f"{name}: relative L2 {rel:.3e} at N={N}, M={M}"


@pytest.mark.parametrize("N,M,H", [(1400, 2, 512), (2048, 2, 512), (4096, 1, 512), (1400, 2, 256), (1024, 1, 320)])
def test_bf16_pipelined_fc_gemms_match_small_tile_kernels(pkg, N, M, H):
    """minibatches > 256 samples route the bf16 fc forward / dgrad through the pipelined LDS-DMA GEMM
    (gemm_pipe.hpp); ALEPPO_OPT_FC_PIPE = 0 keeps the small-tile kernels.  Same bf16 operands, fp32 accumulation in a
    different order (split-K slabs): losses, gradient norm and gradients agree tightly.  700-sample minibatches are
    ragged against the 128-row tiles (identity job map), 1024 / 4096 use the XCD-grouped job map, 4096 gives every
    workgroup several jobs (the ring streams across tile boundaries).  H = 256 is the shortest K the dgrad ring
    accepts (4 k-stages); H = 320 has a ragged last 128-column tile in the forward and 5 k-stages."""
    A = 4
    params = hf.fill_params(910, H, A)
    obs = hf.hf_bytes(911, (N, 4, 84, 84))
    actions = (hf.hf_u32(912, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(913, (N, A), -1, 1))
    adv, ret = hf.hf_range(914, (N,), -1, 1), hf.hf_range(915, (N,), -1, 1)
    masks = (hf.hf_unit(916, N) >= np.float32(0.1)).astype(np.uint8)
    res = {}
    for pipe in (0, 1):
        eng = pkg.Engine(N // 8, 8, A, H, precision=pkg.BF16)
        eng.set_option(pkg.OPT_FC_PIPE, pipe)        # per-context switches (aleppo_set_option)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 2, M)
        res[pipe] = (m, eng.export_grads(), eng.export_params())
        eng.close()
    # each route against the bf16-emulating oracle: every minibatch's loss and norm, the update of 2 * M steps
    we = bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M)
    for pipe, (mm, gg, pp) in res.items():
        c = bc.Checker()
        c.train(H, A, mm, {}, None, we, params0=params, params=pp)
        print(c.summary(f"fc pipe={pipe} N={N} H={H} vs emulated oracle"))
        assert not c.failures, (pipe, c.failures)
    (m0, g0, p0), (m1, g1, p1) = res[0], res[1]
    np.testing.assert_allclose(m1["loss"], m0["loss"], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(m1["grad_norm"], m0["grad_norm"], rtol=5e-3)
    np.testing.assert_allclose(g1, g0, atol=5e-3 * np.abs(g0).max())
    np.testing.assert_allclose(p1, p0, atol=1e-3)
    if N <= 1400:  # and within the documented bf16 bound of the fp32 oracle
        w = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M)
        np.testing.assert_allclose(m1["loss"], w["loss"], rtol=1e-2, atol=3e-2)
        np.testing.assert_allclose(m1["grad_norm"], w["grad_norm"], rtol=5e-2)


def test_full_size_update_is_deterministic_and_schedule_independent(pkg):
    """BASELINE configs[1] update shape (128 envs x T=128 -> 16384 samples, 4 minibatches of 4096, H=512, bf16): the
    update's kernels do not depend on how they are scheduled.  The timed schedule runs the weight-gradient kernels and
    the slab reduce on a second stream beside the dgrad chain; ALEPPO_OPT_SERIAL_UPDATE runs every kernel on one stream.
    Every reduction has a fixed order (no atomics), so the two schedules - and a repeat of the first - must leave
    bit-identical parameters, Adam moments and metrics after two epochs; a missing stream dependency shows up here."""
    E, T, A, H, M = 128, 128, 4, 512, 4
    N = E * T
    params = hf.fill_params(940, H, A)
    base = hf.hf_bytes(941, (N // 8, 4, 84, 84))  # 8 distinct byte-permuted copies: cheap to generate
    obs = np.concatenate([base ^ np.uint8(31 * k) for k in range(8)])
    actions = (hf.hf_u32(942, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(943, (N, A), -1, 1))
    adv, ret = hf.hf_range(944, (N,), -1, 1), hf.hf_range(945, (N,), -1, 1)
    masks = (hf.hf_unit(946, N) >= np.float32(0.05)).astype(np.uint8)
    outs = []
    for serial in (0, 1, 0):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
        pkg.lib().aleppo_set_option(eng._ctx, pkg.OPT_SERIAL_UPDATE, serial)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 2, M)
        sd = eng.state_dict()
        outs.append((m, eng.export_params(), sd["exp_avg"].copy(), sd["exp_avg_sq"].copy()))
        eng.close()
    assert np.isfinite(outs[0][0]["loss"]).all() and np.abs(outs[0][1] - params).max() > 0
    for other in outs[1:]:
        for k in ("loss", "grad_norm"):
            np.testing.assert_array_equal(other[0][k], outs[0][0][k])
        for a, b in zip(other[1:], outs[0][1:]):
            np.testing.assert_array_equal(a, b)


def test_replay_rollout_equals_the_manual_slot_loop(pkg):
    """aleppo_replay_rollout (the native T-slot act/step loop over a recorded trace) leaves exactly the rollout the
    per-slot calls leave: same built-in RNG stream, same observations, scalars, actions and values"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")  # device memory for the recorded frames (no torch in the test process)
    E, T, A, H = 8, 6, 4, 64
    params = hf.fill_params(1010, H, A)
    frames = np.ascontiguousarray(hf.hf_bytes(1011, (T, E, 84, 84)))
    dptr = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(frames.nbytes)) == 0
    assert hip.hipMemcpy(dptr, frames.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(frames.nbytes), 1) == 0
    base = dptr.value
    rew = hf.hf_range(1012, (T, E), -2, 2)
    term = (hf.hf_unit(1013, T * E) < np.float32(0.1)).astype(np.uint8).reshape(T, E)
    trunc = np.zeros((T, E), np.uint8)
    start = (hf.hf_unit(1014, T * E) < np.float32(0.1)).astype(np.uint8).reshape(T, E)
    start[0, :] = 1
    term[start != 0] = 0  # flags are mutually exclusive (gae.cc:52-56)
    got = []
    for native in (False, True):
        eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=77)
        eng.load_params(params)
        if native:
            eng.replay_rollout(base, pkg.FRAMES_84, E * 84 * 84, rew, term, trunc, start)
        else:
            for t in range(T):
                eng.act_fast()
                eng.step_ptr(base + t * E * 84 * 84, pkg.DEVICE, pkg.FRAMES_84, rew[t].ctypes.data,
                             term[t].ctypes.data, trunc[t].ctypes.data, start[t].ctypes.data)
        eng.finish_rollout()
        got.append({k: eng.read_batch(k) for k in ("observations", "actions", "advantages", "returns", "masks",
                                                   "log_probs", "values", "rewards")})
        eng.close()
    hip.hipFree(dptr)
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


# ------------------------------------------------------------------ the whole rollout protocol
def _run_rollouts(pkg, E, T, A, H, rollouts, kind):
    params = hf.fill_params(610, H, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    eng.load_params(params)
    lut = ((np.arange(256) * 5 + 1) % 256).astype(np.uint8)
    if kind == "raw":
        eng.set_gray_lut(lut)
    rng = np.random.default_rng(3)
    obs_ref = np.zeros((E, 4, 84, 84), np.uint8)
    start = np.ones(E, np.uint8)
    rewards = np.zeros(E, np.float32)
    for ro in range(rollouts):
        rec = dict(obs=[], act=[], rew=[], term=[], trunc=[], start=[], noise=[])
        for t in range(T):
            noise = rng.exponential(size=(E, A)).astype(np.float32)
            actions = eng.act(noise).copy()
            np.testing.assert_array_equal(eng.read_batch("current_obs"), obs_ref)
            rec["obs"].append(obs_ref.copy())
            rec["act"].append(actions)
            rec["noise"].append(noise)
            if kind == "raw":
                raw = hf.hf_bytes(2000 + ro * T + t, (E, 2, 210, 160))
                frames = orc.preprocess(raw, lut)
            else:
                frames = hf.hf_bytes(2000 + ro * T + t, (E, 84, 84))
            u = rng.random(E)
            term = ((u < 0.15) & (start == 0)).astype(np.uint8)
            trunc = ((u >= 0.15) & (u < 0.2) & (start == 0)).astype(np.uint8)
            rewards = np.where(start == 1, rewards, rng.integers(-3, 4, E)).astype(np.float32)  # stale on start
            if kind == "raw":
                eng.push_frames(raw, start, kind=pkg.FRAMES_RAW_PAIR)
                eng.record_step(rewards, term, trunc, start)
            else:
                eng.step(frames, rewards, term, trunc, start)
            rec["rew"].append(rewards.copy()); rec["term"].append(term); rec["trunc"].append(trunc)
            rec["start"].append(start.copy())
            obs_ref = orc.update_observations(obs_ref, frames, start)
            start = (term | trunc).astype(np.uint8)
        eng.finish_rollout(rng.exponential(size=(E, A)).astype(np.float32))
        yield eng, params, rec, obs_ref
    eng.close()


@pytest.mark.parametrize("kind", ["84", "raw"])
def test_rollout_protocol_vs_oracle(pkg, kind):
    E, T, A, H = 6, 9, 6, 64
    adam = None  # the oracle's Adam moments / step persist across rollouts like the engine's
    for eng, params, rec, obs_after in _run_rollouts(pkg, E, T, A, H, 2, kind):
        em = lambda k: np.stack(rec[k], 1)  # [T][E] lists -> env-major [E,T]
        b = {k: eng.read_batch(k) for k in pkg.FIELDS if k != "current_obs"}
        # byte / flag / index planes: bit-exact
        np.testing.assert_array_equal(b["observations"], em("obs"))
        np.testing.assert_array_equal(b["terminals"], em("term"))
        np.testing.assert_array_equal(b["truncations"], em("trunc"))
        np.testing.assert_array_equal(b["masks"], 1 - em("start"))
        np.testing.assert_array_equal(b["rewards"], np.clip(em("rew"), -1, 1))  # clamped in place (buffer.cc:67)
        # network outputs vs oracle forward on the same observations
        wl, wv = orc.net_forward(params, H, A, em("obs").reshape(E * T, 4, 84, 84))
        np.testing.assert_allclose(b["logits"].reshape(E * T, A), wl, atol=1e-4)
        np.testing.assert_allclose(b["values"].ravel(), wv, atol=1e-4)
        _, nv = orc.net_forward(params, H, A, obs_after)
        np.testing.assert_allclose(b["next_values"], nv, atol=1e-4)
        # sampled actions: bit-exact given OUR logits and the same noise (tie-margin free definition)
        want = orc.sample(orc.softmax(b["logits"].reshape(E * T, A)), em("noise").reshape(E * T, A))
        np.testing.assert_array_equal(b["actions"].ravel(), want)
        np.testing.assert_array_equal(b["actions"], em("act"))
        # GAE / returns / log-probs from OUR stored values: same fp32 op order -> tight
        o = orc.buffer_get(em("rew"), b["values"], b["next_values"], em("term"), em("trunc"), em("start"))
        np.testing.assert_allclose(b["advantages"], o["advantages"], atol=1e-6)
        np.testing.assert_allclose(b["returns"], o["returns"], atol=1e-6)
        np.testing.assert_allclose(b["log_probs"].reshape(E * T, A), orc.log_softmax(b["logits"].reshape(E * T, A)),
                                   atol=2e-6)
        # and the update on that batch equals the oracle's update on the same batch
        m = eng.train(1e-3, 1, 3)
        w = orc.train(params, H, A, b["observations"].reshape(E * T, 4, 84, 84), b["actions"].ravel(),
                      b["log_probs"].reshape(E * T, A), b["advantages"].ravel(), b["returns"].ravel(),
                      b["masks"].ravel(), 1, 3, lr=1e-3, adam=adam)
        adam = w["adam"]
        np.testing.assert_allclose(m["loss"], w["loss"], atol=1e-4)
        np.testing.assert_allclose(m["grad_norm"], w["grad_norm"], rtol=1e-3)
        new = eng.export_params()
        np.testing.assert_allclose(new, w["params"], atol=1e-4)
        params[:] = new  # the next rollout acts with the updated weights on both sides


def test_bf16_acting_path_close_to_oracle(pkg):
    """bf16 acting path (fused conv1-3 kernel, split-K fc, head): logits/values within the documented bf16
    bound of the fp32 oracle; sampled actions bit-exact given ITS logits and the supplied noise"""
    E, T, A, H = 37, 3, 6, 512
    params = hf.fill_params(810, H, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
    eng.load_params(params)
    rng = np.random.default_rng(5)
    obs_ref = np.zeros((E, 4, 84, 84), np.uint8)
    start = np.ones(E, np.uint8)
    noises, acts, obs_all = [], [], []
    for t in range(T):
        noise = rng.exponential(size=(E, A)).astype(np.float32)
        acts.append(eng.act(noise).copy()); noises.append(noise); obs_all.append(obs_ref.copy())
        frames = hf.hf_bytes(3000 + t, (E, 84, 84))
        eng.step(frames, np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8), start)
        obs_ref = orc.update_observations(obs_ref, frames, start)
        start = np.zeros(E, np.uint8)
    eng.finish_rollout(rng.exponential(size=(E, A)).astype(np.float32))
    logits = eng.read_batch("logits")
    values = eng.read_batch("values")
    np.testing.assert_array_equal(eng.read_batch("observations"), np.stack(obs_all, 1))
    wl, wv = orc.net_forward(params, H, A, np.stack(obs_all, 1).reshape(E * T, 4, 84, 84))
    np.testing.assert_allclose(logits.reshape(E * T, A), wl, atol=3e-2)
    np.testing.assert_allclose(values.ravel(), wv, atol=3e-2)
    c = bc.Checker()  # and the bf16-emulating oracle at the tight bounds of bf16_check.py
    c.forward(logits.reshape(E * T, A), values.ravel(),
              bc.emulated_forward(params, H, A, np.stack(obs_all, 1).reshape(E * T, 4, 84, 84)))
    assert not c.failures, c.failures
    want = orc.sample(orc.softmax(logits.reshape(E * T, A)), np.stack(noises, 1).reshape(E * T, A))
    np.testing.assert_array_equal(np.stack(acts, 1).ravel(), want)
    eng.close()


def test_rccl_path_at_benched_size_with_one_rank_communicator(pkg):
    """the data-parallel schedule of aleppo_train at the size the multi-GPU bench runs it (B = 4096, H = 512, bf16: slab
    groups reduced early for bucket 0, bucket all-reduces on the communication stream beside the conv backward, no fused
    tail reduce) with a 1-rank RCCL communicator: bit-identical to the single-GPU schedule"""
    E, T, A, H, M = 128, 64, 4, 512, 2
    N = E * T
    params = hf.fill_params(2310, H, A)
    base = hf.hf_bytes(2311, (N // 8, 4, 84, 84))
    obs = np.concatenate([base ^ np.uint8(11 * k) for k in range(8)])
    actions = (hf.hf_u32(2312, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(2313, (N, A), -1, 1))
    adv, ret = hf.hf_range(2314, (N,), -1, 1), hf.hf_range(2315, (N,), -1, 1)
    masks = (hf.hf_unit(2316, N) >= np.float32(0.05)).astype(np.uint8)
    out = []
    for comm in (False, True):
        eng = pkg.Engine(E, T, A, H, precision=pkg.BF16)
        if comm:
            eng.comm_init(pkg.Engine.comm_unique_id())
            eng.set_option(pkg.OPT_FORCE_COMM, 1)
        else:  # (the data-parallel schedule keeps the backward tail as three launches: compare like with like)
            eng.set_option(pkg.OPT_FUSED_BWD, 0)
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 2, M)
        out.append((m, eng.export_params(), eng.export_grads()))
        eng.close()
    for k in ("loss", "grad_norm", "mask_count"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])
    # the three-launch tail at B = 4096 against the bf16-emulating oracle: every minibatch's loss / norm, the update
    we = bc.emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, 2, M)
    c = bc.Checker()
    c.train(H, A, out[1][0], {}, None, we, params0=params, params=out[1][1])
    print(c.summary("data-parallel schedule B=4096 vs emulated oracle"))
    assert not c.failures, c.failures


@pytest.mark.parametrize("prec", ["bf16"])  # one precision: the 1-rank communicator init alone takes ~60 s
def test_rccl_path_with_one_rank_communicator(pkg, prec):
    """the data-parallel code path of aleppo_train (mask-count / bucketed gradient / metric all-reduces on the
    side stream, event choreography) executed with a 1-rank RCCL communicator: identical results to the
    no-communicator path (N>1 GPUs are only available to the round-end driver)"""
    H, A, N, M = 64, 4, 64, 2
    params = hf.fill_params(910, H, A)
    obs = hf.hf_bytes(911, (N, 4, 84, 84))
    actions = (hf.hf_u32(912, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(913, (N, A), -1, 1))
    adv, ret = hf.hf_range(914, (N,), -1, 1), hf.hf_range(915, (N,), -1, 1)
    masks = (hf.hf_unit(916, N) >= np.float32(0.2)).astype(np.uint8)
    out = []
    for comm in (False, True):
        eng = pkg.Engine(8, 8, A, H, precision=pkg.FP32 if prec == "fp32" else pkg.BF16, advantage_norm=False)
        if comm:
            eng.comm_init(pkg.Engine.comm_unique_id())
            eng._c(pkg.lib().aleppo_set_option(eng._ctx, 2, 1))
        eng.load_params(params)
        eng.set_batch(obs, actions, old_lp, adv, ret, masks)
        m = eng.train(2.5e-4, 2, M)
        out.append((m, eng.export_params()))
        eng.close()
    np.testing.assert_array_equal(out[0][0]["loss"], out[1][0]["loss"])
    np.testing.assert_array_equal(out[0][0]["grad_norm"], out[1][0]["grad_norm"])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_rccl_communicator_beside_torch_distributed_nccl(tmp_path):
    """bench.py's multi-GPU situation in one process: torch.distributed's NCCL (= RCCL) process group for the barriers /
    timing reductions AND the library's own RCCL communicator for the gradient all-reduce.  One rank (one GPU on this
    box), in a subprocess so that the process group does not leak into the other tests."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "coexist.py"
    script.write_text(f"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch, torch.distributed as dist
import hashfill as hf
from __graft_entry__ import load_package
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
pkg = load_package()
uid = [pkg.Engine.comm_unique_id()]
dist.broadcast_object_list(uid, src=0)
H, A, N, M = 64, 4, 64, 2
eng = pkg.Engine(8, 8, A, H, precision=pkg.BF16, advantage_norm=False)
eng.comm_init(uid[0])
eng._c(pkg.lib().aleppo_set_option(eng._ctx, pkg.OPT_FORCE_COMM, 1))
eng.load_params(hf.fill_params(910, H, A))
rng = np.random.default_rng(0)
eng.set_batch(rng.integers(0, 256, (N, 4, 84, 84), dtype=np.uint8), rng.integers(0, A, N),
              np.full((N, A), -np.log(A), np.float32), rng.standard_normal(N).astype(np.float32),
              rng.standard_normal(N).astype(np.float32), np.ones(N, np.uint8))
t = torch.ones(1, device="cuda")
dist.all_reduce(t); dist.barrier(); torch.cuda.synchronize()
m = eng.train(2.5e-4, 2, M)
dist.all_reduce(t); dist.barrier(); torch.cuda.synchronize()
assert np.isfinite(m["loss"]).all() and t.item() == 1.0
eng.close()
dist.destroy_process_group()
print("COEXIST_OK")
""")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "COEXIST_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_checkpoint_resume_is_bit_identical(pkg):
    H, A, N, M = 64, 4, 64, 2
    params = hf.fill_params(930, H, A)
    obs = hf.hf_bytes(931, (N, 4, 84, 84))
    batch = (obs, (hf.hf_u32(932, N) % np.uint32(A)).astype(np.int64), orc.log_softmax(hf.hf_range(933, (N, A), -1, 1)),
             hf.hf_range(934, (N,), -1, 1), hf.hf_range(935, (N,), -1, 1), np.ones(N, np.uint8))
    a = pkg.Engine(8, 8, A, H)
    a.load_params(params)
    a.set_batch(*batch)
    a.train(2.5e-4, 1, M)
    sd = a.state_dict()
    assert int(sd["step"]) == M and np.abs(sd["exp_avg_sq"]).sum() > 0
    a.train(2.0e-4, 1, M)
    want = a.export_params()
    a.close()
    b = pkg.Engine(8, 8, A, H)
    b.load_state_dict(sd)
    b.set_batch(*batch)
    b.train(2.0e-4, 1, M)
    np.testing.assert_array_equal(b.export_params(), want)
    b.close()


def test_buffer_not_full_and_bad_minibatch_errors(pkg):
    eng = pkg.Engine(4, 4, 4, 32)
    with pytest.raises(pkg.AleppoError, match="Buffer is not full"):
        eng.finish_rollout()
    eng.set_batch(np.zeros((16, 4, 84, 84), np.uint8), np.zeros(16, np.int64), np.zeros((16, 4), np.float32),
                  np.zeros(16), np.zeros(16), np.ones(16, np.uint8))
    with pytest.raises(pkg.AleppoError, match="divisible by num_mini_batches"):
        eng.train(1e-3, 1, 3)
    eng.close()


def test_builtin_rng_is_deterministic_and_roughly_uniform(pkg):
    E, A = 512, 4
    counts = np.zeros(A)
    seqs = []
    for rep in range(2):
        eng = pkg.Engine(E, 2, A, 32, seed=123)
        eng.load_params(np.zeros(eng.param_count, np.float32))  # all-zero net -> uniform policy
        a0 = eng.act().copy()
        eng.step(np.zeros((E, 84, 84), np.uint8), np.zeros(E), np.zeros(E), np.zeros(E), np.ones(E))
        a1 = eng.act().copy()
        seqs.append(np.concatenate([a0, a1]))
        eng.close()
    np.testing.assert_array_equal(seqs[0], seqs[1])
    for k in range(A):
        counts[k] = (seqs[0] == k).sum()
    assert counts.min() > 0.15 * 2 * E and (seqs[0][:E] != seqs[0][E:]).any()
