"""ALEPPO_OPT_MINIBATCH_SHUFFLE: opt-in per-epoch minibatch shuffling of aleppo_train.

CPU: a numpy mirror of the permutation aleppo.h specifies (aleppo_read_sample_order), the public constants, and the
trainer's `shuffle_minibatches` key against the host-only library stand-in.
GPU (-m gpu, everything through the C ABI): the device order equals the mirror (eager, resumed, graph-replayed), a
shuffled update equals a contiguous update on the host-permuted batch bit for bit on every schedule, and the CPU oracle
on the permuted batch."""
import functools
import os
import re

import numpy as np
import pytest

import hashfill as hf
import oracle_lib as orc
import update_harness as uh
from shared_fixtures import pkg, stub_trainer  # noqa: F401
from trainer_helpers import debug_cfg, events, header_const, run_stub
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


# ------------------------------------------------------------------ the permutation of aleppo.h, restated
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def sample_order_row(N, seed, rank, step0):
    w = max(2, int(N - 1).bit_length())  # ceil(log2 N), at least 2
    w += w & 1
    h = w // 2
    mask = np.uint32((1 << h) - 1)
    key = splitmix64(seed ^ splitmix64(((rank << 40) ^ step0) & U64))
    k = [np.uint32(splitmix64((key + r) & U64) & 0xFFFFFFFF) for r in range(4)]

    def P(x):
        L, R = x >> np.uint32(h), x & mask
        for r in range(4):
            L, R = R, L ^ (fmix32(R ^ k[r]) & mask)
        return (L << np.uint32(h)) | R

    y = P(np.arange(N, dtype=np.uint32))
    out = y >= N
    while out.any():
        y[out] = P(y[out])
        out = y >= N
    return y.astype(np.int32)


def sample_order(N, seed, rank, step, epochs, M):
    """rows of one aleppo_train call that starts at Adam step `step`"""
    return np.stack([sample_order_row(N, seed, rank, step + e * M) for e in range(epochs)])


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 1000, 16384, 2 ** 20 + 7])
def test_mirror_is_a_bijection(N):
    row = sample_order_row(N, 42, 0, 0)
    assert row.shape == (N,)
    np.testing.assert_array_equal(np.sort(row), np.arange(N))


def test_mirror_depends_on_step_seed_and_rank():
    N = 1000
    base = sample_order_row(N, 42, 0, 0)
    assert (base != np.arange(N)).sum() > N // 2
    for other in (sample_order_row(N, 42, 0, 4), sample_order_row(N, 43, 0, 0), sample_order_row(N, 42, 1, 0)):
        assert (other != base).sum() > N // 2
    np.testing.assert_array_equal(sample_order_row(N, 42, 0, 0), base)  # stateless


def test_header_constant_and_export():
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    assert header_const("ALEPPO_OPT_MINIBATCH_SHUFFLE") == pkg.OPT_MINIBATCH_SHUFFLE == 12
    assert "aleppo_read_sample_order" in pkg.EXPORTS
    assert re.search(r"int aleppo_read_sample_order\(aleppo_ctx \*ctx, int32_t \*dst, size_t count\);", hdr)


@pytest.mark.parametrize("shuffle", [True, False])
def test_trainer_key_reaches_the_hparams_record(stub_trainer, tmp_path, shuffle):
    r = run_stub(stub_trainer, tmp_path, debug_cfg(tmp_path, "shuffle_minibatches: true\n" if shuffle else ""))
    assert r.returncode == 0, r.stderr[-2000:]
    data = events(tmp_path)
    assert b"_hparams_/session_start_info" in data and b"cuda_graph" in data
    assert (b"shuffle_minibatches" in data) == shuffle


# ------------------------------------------------------------------ GPU
# (the first sample of each of this file's seeds is unmasked by its hash already: the harness pinning it changes nothing)
_hashed = functools.partial(uh.hashed_batch, mask_p=0.1)
METRICS = uh.PER_SAMPLE[:5]


@pytest.mark.gpu
def test_device_order_is_the_documented_one(pkg):
    E, T, A, H, epochs, M, seed = 8, 16, 4, 32, 4, 4, 1234
    N = E * T
    params = hf.fill_params(3100, H, A)
    batch = _hashed(3101, N, A)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=seed)
    eng.load_params(params)
    eng.set_batch(*batch)
    with pytest.raises(pkg.AleppoError):
        eng.sample_order(epochs)  # no update yet
    eng.train(2.5e-4, 1, M)
    np.testing.assert_array_equal(eng.sample_order(1), np.arange(N, dtype=np.int32)[None])  # contiguous: identity
    assert eng.get_option(pkg.OPT_MINIBATCH_SHUFFLE) == 0
    eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
    assert eng.get_option(pkg.OPT_MINIBATCH_SHUFFLE) == 1
    step = int(eng.state_dict()["step"])
    assert step == M
    eng.train(2.5e-4, epochs, M)
    o1 = eng.sample_order(epochs)
    for row in o1:
        np.testing.assert_array_equal(np.sort(row), np.arange(N))
    np.testing.assert_array_equal(o1, sample_order(N, seed, 0, step, epochs, M))
    sd = eng.state_dict()  # resume point
    eng.train(2.5e-4, epochs, M)  # continues from the new Adam step
    o2 = eng.sample_order(epochs)
    np.testing.assert_array_equal(o2, sample_order(N, seed, 0, step + epochs * M, epochs, M))
    assert (o2 != o1).any()
    p_after = eng.export_params()
    # graph capture / replay: every call still follows the Adam step
    eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    for call in range(3):  # eager (warm-up), capture + launch, replay
        eng.train(2.5e-4, epochs, M)
        s0 = step + (2 + call) * epochs * M
        np.testing.assert_array_equal(eng.sample_order(epochs), sample_order(N, seed, 0, s0, epochs, M))
    assert eng.get_option(pkg.OPT_UPDATE_GRAPH) >= 2
    eng.close()
    # a fresh context given the same seed, parameters and optimizer state replays the orders (and the update)
    eng2 = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=seed)
    eng2.load_state_dict(sd)
    eng2.set_batch(*batch)
    eng2.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
    eng2.train(2.5e-4, epochs, M)
    np.testing.assert_array_equal(eng2.sample_order(epochs), o2)
    np.testing.assert_array_equal(eng2.export_params(), p_after)
    eng2.close()


def _shuffled_vs_contiguous(pkg, E, T, A, H, epochs, M, prec, batch, options=(), comm=False, engine_kw=None,
                            params=None):
    """context A trains shuffled on `batch`; context B trains contiguously on batch[order[e]] one epoch at a time"""
    N = E * T
    B = N // M
    out = []
    for shuffled in (True, False):
        eng = uh.make_engine(pkg, E, T, A, H, prec, options, comm, **(engine_kw or {}))
        eng.load_params(params)
        if shuffled:
            eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
            eng.set_batch(*batch)
            m = eng.train(2.5e-4, epochs, M)
            order = eng.sample_order(epochs)
            per = {k: eng.read_train_metric(k, epochs, M, B) for k in METRICS}
            m_rows = m
        else:
            per = {k: np.zeros((epochs, M, B), np.float32) for k in METRICS}
            m_rows = {}
            for e in range(epochs):
                o = order[e]
                eng.set_batch(*[x[o] for x in batch])
                me = eng.train(2.5e-4, 1, M)
                for k in me:
                    m_rows.setdefault(k, []).append(me[k][0])
                for k in METRICS:
                    per[k][e] = eng.read_train_metric(k, 1, M, B)[0]
                np.testing.assert_array_equal(eng.sample_order(1)[0], np.arange(N))
            m_rows = {k: np.stack(v) for k, v in m_rows.items()}
        out.append((m_rows, per, eng.export_params(), eng.export_grads()))
        eng.close()
        if shuffled:
            assert (order != np.arange(N)[None]).any()
    (ma, pa, xa, ga), (mb, pb, xb, gb) = out
    for k in ("loss", "grad_norm", "clipped_loss", "value_loss", "entropy", "ratio", "mask_count"):
        np.testing.assert_array_equal(ma[k], mb[k], err_msg=k)
    for k in METRICS:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ga, gb)
    assert np.abs(xa - params).max() > 0
    return order


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fp32", "bf16_benched", "bf16_unfused", "bf16_comm"])
def test_shuffled_equals_contiguous_on_the_permuted_batch(pkg, case):
    if case == "fp32":
        E, T, A, H, epochs, M, prec, distinct = 8, 32, 6, 64, 2, 4, pkg.FP32, None
    else:  # BASELINE configs[1]'s update: 16384 samples, minibatches of 4096 (both fused kernels on the path)
        E, T, A, H, epochs, M, prec, distinct = 128, 128, 4, 512, 2, 4, pkg.BF16, 8
    options, comm = [], False
    if case == "bf16_unfused":
        options = [(pkg.OPT_FUSED_FWD, 0), (pkg.OPT_FUSED_BWD, 0)]
    if case == "bf16_comm":  # the data-parallel schedule on a 1-rank communicator
        options, comm = [(pkg.OPT_FORCE_COMM, 1)], True
    params = hf.fill_params(3200, H, A)
    batch = _hashed(3201, E * T, A, distinct=distinct)
    _shuffled_vs_contiguous(pkg, E, T, A, H, epochs, M, prec, batch, options, comm, params=params)


@pytest.mark.gpu
def test_shuffled_rollout_batch_with_fp16_planes_and_advantage_norm(pkg):
    """a rollout-produced batch (fp16 rollout planes, advantage normalisation): context B is fed context A's read-back
    planes, which fp16 represents exactly"""
    E, T, A, H, epochs, M = 8, 16, 4, 32, 3, 4
    N = E * T
    kw = dict(rollout_precision=pkg.ROLLOUT_FP16, advantage_norm=True)
    params = hf.fill_params(3300, H, A)
    a = pkg.Engine(E, T, A, H, precision=pkg.FP32, **kw)
    a.load_params(params)
    rng = np.random.default_rng(5)
    start = np.ones(E, np.uint8)
    rewards = np.zeros(E, np.float32)
    for t in range(T):
        a.act(rng.exponential(size=(E, A)).astype(np.float32))
        frames = hf.hf_bytes(3400 + t, (E, 84, 84))
        term = ((rng.random(E) < 0.15) & (start == 0)).astype(np.uint8)
        rewards = np.where(start == 1, rewards, rng.integers(-2, 3, E)).astype(np.float32)
        a.step(frames, rewards, term, np.zeros(E, np.uint8), start)
        start = term.copy()
    a.finish_rollout(rng.exponential(size=(E, A)).astype(np.float32))
    b = {k: a.read_batch(k) for k in ("observations", "actions", "log_probs", "advantages", "returns", "masks")}
    batch = (b["observations"].reshape(N, 4, 84, 84), b["actions"].ravel(), b["log_probs"].reshape(N, A),
             b["advantages"].ravel(), b["returns"].ravel(), b["masks"].ravel())
    assert (batch[5] == 0).any()  # some episode starts are masked out
    a.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
    m = a.train(2.5e-4, epochs, M)
    order = a.sample_order(epochs)
    per = {k: a.read_train_metric(k, epochs, M, N // M) for k in METRICS}
    xa, ga = a.export_params(), a.export_grads()
    a.close()
    bb = pkg.Engine(E, T, A, H, precision=pkg.FP32, **kw)
    bb.load_params(params)
    for e in range(epochs):
        bb.set_batch(*[x[order[e]] for x in batch])
        me = bb.train(2.5e-4, 1, M)
        for k in me:
            np.testing.assert_array_equal(me[k][0], m[k][e], err_msg=k)
        for k in METRICS:
            np.testing.assert_array_equal(bb.read_train_metric(k, 1, M, N // M)[0], per[k][e], err_msg=k)
    np.testing.assert_array_equal(bb.export_params(), xa)
    np.testing.assert_array_equal(bb.export_grads(), ga)
    bb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E,T,epochs,M", [(8, 32, 2, 2), (32, 128, 2, 1)])  # B = 128, B = 4096
def test_shuffled_update_vs_oracle_on_the_permuted_batch(pkg, E, T, epochs, M):
    A, H, seed = 6, 512, 99
    N = E * T
    params = hf.fill_params(3500, H, A)
    batch = _hashed(3501, N, A, distinct=8 if N >= 4096 else None)
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=seed)
    eng.load_params(params)
    eng.set_batch(*batch)
    eng.set_option(pkg.OPT_MINIBATCH_SHUFFLE, 1)
    m = eng.train(2.5e-4, epochs, M)
    order = eng.sample_order(epochs)
    np.testing.assert_array_equal(order, sample_order(N, seed, 0, 0, epochs, M))
    p, adam = params, None
    for e in range(epochs):
        w = orc.train(p, H, A, *[x[order[e]] for x in batch], 1, M, adam=adam)
        p, adam = w["params"], w["adam"]
        np.testing.assert_allclose(m["loss"][e], w["loss"][0], atol=1e-4)
    np.testing.assert_allclose(eng.export_params(), p, atol=1e-4)
    eng.close()
