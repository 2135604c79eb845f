"""The stored parameter sets (averaged, snapshot, anchor) and the sample sources behind the diagnostics, through the one
implementation each has (csrc/api_core.hip: param_set_* / upload_flat, source_check / source_open / source_walk).

GPU only.  Contexts of E = 8, T = 8 and max_minibatch = 24 at (H, A) = (32, 4) in fp32 and (96, 18) in bf16, hashed
parameters and a hashed batch of 64 samples through set_batch, so that the batch source walks in chunks of 24, 24, 16.
  1. a take from the live parameters, exported, is export_params bit for bit - for each of the three sets;
  2. an imported vector comes back bit for bit from the export, with the update count for the averaged set;
  3. (bf16) an imported snapshot's compute copy is cast: with the same vector loaded as the live parameters,
     policy_diff("snapshot", "live") over the batch sees no difference at all;
  4. activation_stats, feature_rank, policy_diff, recycle_dormant and saliency refuse a batch source without a batch
     (runtime error) and more observations than max_minibatch (invalid argument), and the context then acts like a twin
     that never made the calls.
What the calls compute is checked by each feature's own suite."""
import functools

import numpy as np
import pytest

import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401

E, T, MAX_MB, N_BATCH = 8, 8, 24, 64
SHAPES = {"fp32": (9100, 32, 4), "bf16": (9200, 96, 18)}  # precision: (parameter seed, H, A) - test_ema's small shapes
OTHER_SEED, BATCH_SEED, ACT_SEED = 9300, 9400, 9500
LR = 2.5e-4
PRECS = ["fp32", "bf16"]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _params(prec, other=False):
    seed, H, A = SHAPES[prec]
    p = hf.fill_params(OTHER_SEED if other else seed, H, A)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _batch(A):
    """what set_batch wants: N_BATCH hashed observations and the planes next to them"""
    s, n = BATCH_SEED, N_BATCH
    out = (hf.hf_bytes(s, (n, 4, 84, 84)), (hf.hf_u32(s + 2, n) % np.uint32(A)).astype(np.int64),
           orc.log_softmax(hf.hf_range(s + 3, (n, A), -1, 1)), hf.hf_range(s + 4, (n,), -1, 1),
           hf.hf_range(s + 5, (n,), -1, 1), (hf.hf_unit(s + 6, n) >= np.float32(0.1)).astype(np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


def _engine(pkg, prec, batch=True):
    _, H, A = SHAPES[prec]
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec == "fp32" else pkg.BF16, max_minibatch=MAX_MB)
    eng.load_params(_params(prec))
    if batch:
        eng.set_batch(*_batch(A))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_a_take_from_live_exports_the_live_parameters(pkg, prec):
    eng = _engine(pkg, prec)
    eng.train(LR, 1, 4)  # (the live parameters are no longer the vector that was loaded)
    live = eng.export_params()
    assert not _same(live, _params(prec))
    eng.ema_open()
    eng.snapshot_take("live")
    eng.anchor_take("live")
    averaged, updates = eng.ema_params()
    assert _same(averaged, live) and updates == 0
    assert _same(eng.snapshot_params(), live)
    assert _same(eng.anchor_params(), live)
    assert _same(eng.export_params(), live)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_an_import_exports_the_imported_vector(pkg, prec):
    eng = _engine(pkg, prec, batch=False)
    live, v = _params(prec), _params(prec, other=True)
    assert not _same(live, v)
    eng.ema_open()  # (aleppo_ema_import needs the open; the other two imports allocate their set themselves)
    eng.load_ema(v, 5)
    eng.load_snapshot(v)
    eng.load_anchor(v)
    averaged, updates = eng.ema_params()
    assert _same(averaged, v) and updates == 5
    assert _same(eng.snapshot_params(), v)
    assert _same(eng.anchor_params(), v)
    assert _same(eng.export_params(), live)
    eng.close()


@pytest.mark.gpu
def test_an_imported_snapshot_forwards_like_the_same_vector_loaded(pkg):
    prec = "bf16"
    eng = _engine(pkg, prec)
    v = _params(prec, other=True)
    eng.snapshot_take("live")  # (the snapshot's compute copy now holds the first vector: an import has to replace it)
    eng.load_snapshot(v)
    eng.load_params(v)
    got = eng.policy_diff("snapshot", "live", per_sample=True)
    st, rows = got["stats"], got["per_sample"]
    print({k: st[k] for k in ("rows", "nonfinite_rows", "churn", "mean_kl_ab", "mean_kl_ba", "mean_tv", "max_abs_dv")})
    assert st["rows"] == N_BATCH and st["nonfinite_rows"] == 0 and st["churn"] == 0
    assert rows.shape == (N_BATCH, pkg.PD_ROW)
    for name in ("kl_ab", "kl_ba", "tv", "dv"):
        assert (rows[:, pkg.PD_COLUMNS[name]] == 0).all(), name
    eng.close()


def _refusals(pkg, eng):
    """every diagnostic on a batch source without a batch, then on more observations than max_minibatch"""
    many = hf.hf_bytes(ACT_SEED + 3, (MAX_MB + 1, 4, 84, 84))
    calls = dict(activation_stats=eng.activation_stats, feature_rank=eng.feature_rank,
                 policy_diff=functools.partial(eng.policy_diff, "live", "live"), recycle_dormant=eng.recycle_dormant,
                 saliency=eng.saliency)
    for name, call in calls.items():
        with pytest.raises(pkg.AleppoError, match="no batch"):
            call(observations=None)
        with pytest.raises(pkg.AleppoInvalidArgument, match="n exceeds capacity"):
            call(observations=many)
    return len(calls)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_refused_sources_leave_the_acting_path_alone(pkg, prec):
    _, H, A = SHAPES[prec]
    noise = [hf.hf_range(ACT_SEED + k, (E, A), 0.05, 3) for k in range(2)]
    frames, zero = hf.hf_bytes(ACT_SEED + 2, (E, 84, 84)), np.zeros(E, np.uint8)
    seen = []
    for refused in (True, False):  # the context that makes the refused calls, then its twin that does not
        eng = _engine(pkg, prec, batch=False)
        first = eng.act(noise[0]).copy()
        eng.step(frames, np.zeros(E, np.float32), zero, zero, np.ones(E, np.uint8))  # (pre-computes slot 1's acting forward)
        if refused:
            assert _refusals(pkg, eng) == 5
        second = eng.act(noise[1]).copy()
        seen.append((first, second, eng.read_batch("logits")[:, :2], eng.read_batch("values")[:, :2], eng.export_params()))
        eng.close()
    for a, b in zip(*seen):
        assert _same(a, b)
    assert np.isfinite(seen[0][2]).all() and seen[0][2].any()
