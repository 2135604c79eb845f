"""aleppo_saliency / aleppo_saliency_perturbed on the device: the perturbed stacks byte for byte against the numpy
restatement (tests/saliency_ref.py, with the library's tables), the forward outputs of a chunked call against the oracles,
the scores against the engine's own outputs, the batch source, isolation of a training run, and the errors.
Shapes: fp32 (H, A) = (32, 4), bf16 (96, 18); contexts of E = 4, T = 8, max_minibatch = 32, so a forward chunk holds 32 pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
import saliency_ref as sr
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

SHAPES = {"fp32": (32, 4, 8100), "bf16": (96, 18, 8200)}  # H, A, parameter seed
E, T, MAXB = 4, 8, 32
COARSE = dict(stride=12, sigma_mask=2.0, sigma_blur=1.0)  # G = 7, P = 49
FINE = dict(stride=5, sigma_mask=5.0, sigma_blur=3.0)     # G = 17, P = 289


@functools.lru_cache(maxsize=None)
def _params(prec):
    H, A, seed = SHAPES[prec]
    p = hf.fill_params(seed, H, A)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _observations():
    """n = 3: random half-saturated; constant planes; one bright pixel in a corner of each plane (both reflections)"""
    rnd = sr.half_saturated(hf.hf_bytes(8300, (4, 84, 84)), hf.hf_unit(8301, 4 * 7056).reshape(4, 84, 84))
    const = np.stack([np.full((84, 84), v, np.uint8) for v in (0, 77, 200, 255)])
    corner = np.zeros((4, 84, 84), np.uint8)
    for k, (y, x) in enumerate(((0, 0), (0, 83), (83, 0), (83, 83))):
        corner[k, y, x] = 255
    obs = np.ascontiguousarray(np.stack([rnd, const, corner]))
    obs.setflags(write=False)
    return obs


def _engine(pkg, prec, **kw):
    H, A, _ = SHAPES[prec]
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec == "fp32" else pkg.BF16, max_minibatch=MAXB, **kw)
    eng.load_params(_params(prec))
    return eng


def _bits(a, dt=np.uint32):
    return np.ascontiguousarray(a).view(dt)


def _check_outputs(prec, outputs, stacks, tag):
    """outputs [m, A + 1] of the engine against the oracle's forward on uint8 stacks [m, 4, 84, 84]: fp32 at the project's
    1e-4 (1 + |ref|); bf16 against the bf16-emulating oracle by bf16_check's rule for logits and values"""
    H, A, _ = SHAPES[prec]
    outputs = np.asarray(outputs).reshape(-1, A + 1)
    stacks = np.ascontiguousarray(stacks).reshape(-1, 4, 84, 84)
    assert outputs.shape[0] == stacks.shape[0]
    if prec == "fp32":
        logits, values = orc.net_forward(_params(prec), H, A, stacks)
        ref = np.concatenate([logits, np.asarray(values).reshape(-1, 1)], axis=1).astype(np.float64)
        excess = np.abs(outputs - ref) / (1 + np.abs(ref))
        print(f"{tag} fp32: worst |d| / (1 + |ref|) = {excess.max():.3g} (bound 1e-4)")
        assert excess.max() <= 1e-4, (tag, float(excess.max()))
    else:
        ck = bc.Checker()
        ck.forward(outputs[:, :A], outputs[:, A], bc.emulated_forward(_params(prec), H, A, stacks), tag + " ")
        print(ck.summary(tag + " bf16:"))
        assert not ck.failures, ck.failures


# ------------------------------------------------------------------ 1. the perturbed stacks, byte for byte
@pytest.mark.gpu
@pytest.mark.parametrize("planes", [15, 1, 8])
def test_perturbed_stacks_byte_for_byte(pkg, planes):
    obs = _observations()
    eng = _engine(pkg, "fp32")
    g, w, R = pkg.saliency_tables(**COARSE)
    got = eng.saliency_perturbed(obs, planes=planes, **COARSE)  # all 49 positions: 147 pairs in five chunks
    ref = sr.perturbed(obs, g, w, R, COARSE["stride"], planes)
    assert got.shape == ref.shape == (3, 49, 4, 84, 84)
    assert np.array_equal(got, ref), int((got != ref).sum())
    g, w, R = pkg.saliency_tables(**FINE)
    for p in (0, 16, 272, 288, 144):  # the four corner points and the centre of the 17 x 17 grid
        one = eng.saliency_perturbed(obs, planes=planes, position_first=p, position_count=1, **FINE)
        ref = sr.perturbed(obs, g, w, R, FINE["stride"], planes, positions=[p])
        assert one.shape == ref.shape == (3, 1, 4, 84, 84)
        assert np.array_equal(one, ref), (p, int((one != ref).sum()))
        got = np.concatenate([got, one], axis=1)
    assert (got[1] == obs[1][None]).all()  # the constant observation comes back identical at every point
    off = [k for k in range(4) if not (planes >> k) & 1]
    assert (got[:, :, off] == obs[:, None][:, :, off]).all()  # a plane outside `planes` is untouched
    on = [k for k in range(4) if (planes >> k) & 1]
    assert all((got[0, q][on] != obs[0][on]).any() for q in range(got.shape[1]))  # (and the named ones are perturbed)
    eng.close()


# ------------------------------------------------------------------ 2. / 3. a chunked call: outputs and scores
@functools.lru_cache(maxsize=None)
def _chunked(prec):
    """n = 3 at stride 12: 147 pairs in five forward chunks of at most 32, boundaries inside a sample; called twice"""
    pkg = load_package()
    eng = _engine(pkg, prec)
    res = eng.saliency(_observations(), outputs=True, **COARSE)
    again = eng.saliency(_observations(), outputs=True, **COARSE)
    plain = eng.saliency(_observations(), **COARSE)
    eng.close()
    return res, again, plain


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_chunked_outputs_against_the_oracle(pkg, prec):
    H, A, _ = SHAPES[prec]
    res, again, plain = _chunked(prec)
    assert res["outputs"].shape == (3, 50, A + 1) and res["policy"].shape == res["value"].shape == (3, 7, 7)
    for k in res:  # two calls return identical bits; so does a call that does not ask for the outputs
        assert np.array_equal(_bits(res[k]), _bits(again[k])), k
    assert np.array_equal(_bits(res["policy"]), _bits(plain["policy"])) and np.array_equal(_bits(res["value"]), _bits(plain["value"]))
    assert "outputs" not in plain
    obs = _observations()
    g, w, R = pkg.saliency_tables(**COARSE)
    stacks = np.concatenate([obs[:, None], sr.perturbed(obs, g, w, R, COARSE["stride"])], axis=1)  # row 0: unperturbed
    _check_outputs(prec, res["outputs"], stacks, "chunked")
    assert np.isfinite(res["outputs"]).all()
    assert res["policy"][0].max() > 0 and res["value"][0].max() > 0  # the random observation's outputs move


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_scores_from_the_engines_own_outputs(pkg, prec):
    H, A, _ = SHAPES[prec]
    res = _chunked(prec)[0]
    s_pol, s_val = sr.scores(res["outputs"])
    for name, got, ref, terms in (("policy", res["policy"], s_pol, A), ("value", res["value"], s_val, 1)):
        got = np.asarray(got, np.float64).reshape(3, 49)
        err, bound = np.abs(got - ref), sr.score_bound(ref, terms)
        print(f"scores {prec} {name}: worst |S - S_ref| / bound = {(err / bound).max():.3g}, "
              f"exact zeros {int((ref == 0).sum())} of {ref.size}, constant observation max {got[1].max():.3g}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
        assert (got[ref == 0] == 0).all()  # where the outputs did not move the score is 0


# ------------------------------------------------------------------ 4. the batch source
def _rollout(eng, seed, probe=None):
    start = np.ones(E, np.uint8)
    acts = []
    for t in range(T):
        acts.append(eng.act().copy())
        te = ((hf.hf_unit(seed + 100 + t, E) < 0.1) & (start == 0)).astype(np.uint8)
        eng.step(hf.hf_bytes(seed + t, (E, 84, 84)), hf.hf_range(seed + 200 + t, (E,), -2, 2), te, np.zeros(E, np.uint8), start)
        if probe and t == T // 2:
            probe()
        start = te
    eng.finish_rollout()
    return acts


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_batch_source_reads_the_rollout_in_place(pkg, prec):
    """after finish_rollout, samples [T, 2T) are environment 1: the perturbed bytes equal the caller source's on read_batch's
    observations, the outputs meet the oracle's bounds, and the scores are the caller source's bit for bit"""
    H, A, _ = SHAPES[prec]
    eng = _engine(pkg, prec, seed=5)
    _rollout(eng, 8500)
    obs = eng.read_batch("observations").reshape(E * T, 4, 84, 84)
    env1 = np.ascontiguousarray(obs[T:2 * T])
    assert len({o.tobytes() for o in env1}) == T  # (all eight stacks differ: an order mistake would show)
    pb = eng.saliency_perturbed(first=T, n=T, **COARSE)
    pc = eng.saliency_perturbed(env1, **COARSE)
    assert pb.shape == (T, 49, 4, 84, 84) and np.array_equal(pb, pc)
    tail = eng.saliency_perturbed(first=E * T - 3, position_first=40, position_count=5, **COARSE)  # n: to the end of the batch
    assert np.array_equal(tail, eng.saliency_perturbed(np.ascontiguousarray(obs[-3:]), position_first=40, position_count=5, **COARSE))
    rb = eng.saliency(first=T, n=T, outputs=True, **COARSE)
    rc = eng.saliency(env1, outputs=True, **COARSE)
    for k in rb:
        assert np.array_equal(_bits(rb[k]), _bits(rc[k])), k
    g, w, R = pkg.saliency_tables(**COARSE)
    stacks = np.concatenate([env1[:, None], sr.perturbed(env1, g, w, R, COARSE["stride"])], axis=1)
    _check_outputs(prec, rb["outputs"], stacks, "batch source")
    eng.close()


# ------------------------------------------------------------------ 5. nothing else changes
def _twin(pkg, prec, graph, probes):
    H, A, _ = SHAPES[prec]
    eng = _engine(pkg, prec, seed=3)
    if graph:
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    seen, have_batch = [], []

    def probe():
        if not probes:
            return
        obs = _observations()[:2]
        a = eng.saliency(obs, **COARSE)
        b = eng.saliency(obs, **COARSE)
        seen.append(all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a))  # two consecutive calls: identical bits
        assert eng.saliency_perturbed(obs, position_first=24, position_count=2, **COARSE).shape == (2, 2, 4, 84, 84)
        if have_batch:  # the batch source, once a batch exists (in the middle of a rollout: the slots as they stand)
            assert eng.saliency(first=T - 1, n=2, outputs=True, **COARSE)["outputs"].shape == (2, 50, A + 1)
            assert eng.saliency_perturbed(first=3, n=1, position_count=1, **COARSE).shape == (1, 1, 4, 84, 84)
            seen.append(True)

    out = dict(acts=[], metrics=[], digests=[], replays=[])
    for r in range(2):
        out["acts"] += _rollout(eng, 8700 + 1000 * r, probe)
        have_batch.append(True)
        probe()
        m = eng.train(2.5e-4, 2, 2)
        probe()
        out["metrics"].append(np.stack([m[k] for k in sorted(m)]))
        out["digests"].append(eng.state_digest())
        out["replays"].append(eng.get_option(pkg.OPT_UPDATE_GRAPH))
    out["state"] = eng.state_dict()
    out["seen"] = seen
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec,graph", [("bf16", 0), ("fp32", 0), ("bf16", 1), ("fp32", 1)])
def test_calling_changes_nothing(pkg, prec, graph):
    """twins from one seed run rollout -> update -> rollout -> update; one calls saliency (both sources) and
    saliency_perturbed after a mid-rollout step, after finish_rollout and after train.  Sampled actions, update metrics, the
    state digest, parameters, both moments and the graph-launch count are bit-identical"""
    plain, mixed = _twin(pkg, prec, graph, False), _twin(pkg, prec, graph, True)
    assert len(mixed["seen"]) == 6 + 5 and all(mixed["seen"])
    np.testing.assert_array_equal(np.stack(plain["acts"]), np.stack(mixed["acts"]))
    for r in range(2):
        assert np.array_equal(_bits(plain["metrics"][r]), _bits(mixed["metrics"][r])), r
        assert plain["digests"][r] == mixed["digests"][r], r
    assert plain["replays"] == mixed["replays"] == ([0, 1] if graph else [0, 0])
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(_bits(plain["state"][k]), _bits(mixed["state"][k])), k
    assert plain["state"]["step"] == mixed["state"]["step"] == 8


# ------------------------------------------------------------------ 6. errors
def _raw(pkg, eng, obs, first, n, want_outputs=True, null=(), **kw):
    """the C entry point itself: (status, policy, value, outputs), the outputs pre-filled with -7"""
    k = dict(sr.DEFAULTS, **COARSE)
    k.update(kw)
    cfg = pkg.SaliencyConfig(k["stride"], k["planes"], k["sigma_mask"], k["sigma_blur"])
    m, G = max(int(n), 1), sr.grid(k["stride"]) if 1 <= k["stride"] <= 84 else 1
    pol, val = np.full((m, G, G), -7, np.float32), np.full((m, G, G), -7, np.float32)
    out = np.full((m, G * G + 1, eng.A + 1), -7, np.float32)
    ptr = lambda a, name: None if a is None or name in null else a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().aleppo_saliency(eng._ctx, ptr(obs, "obs"), C.c_int64(first), C.c_int64(n), C.byref(cfg),
                                   ptr(pol, "policy"), ptr(val, "value"), ptr(out if want_outputs else None, "outputs"))
    return rc, pol, val, out


def _raw_perturbed(pkg, eng, obs, first, n, p0, count, null_out=False, **kw):
    k = dict(sr.DEFAULTS, **COARSE)
    k.update(kw)
    cfg = pkg.SaliencyConfig(k["stride"], k["planes"], k["sigma_mask"], k["sigma_blur"])
    out = np.full((max(int(n), 1), max(int(count), 1), 4, 84, 84), 9, np.uint8)
    rc = pkg.lib().aleppo_saliency_perturbed(eng._ctx, None if obs is None else obs.ctypes.data_as(C.c_void_p),
                                             C.c_int64(first), C.c_int64(n), C.byref(cfg), C.c_int64(p0), C.c_int64(count),
                                             None if null_out else out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.gpu
def test_errors(pkg):
    """every invalid parameter, n above the capacity, first != 0 with observations, a range outside the batch, a null output:
    ALEPPO_ERR_INVALID_ARGUMENT; the batch source without a batch and any call while a step is armed: ALEPPO_ERR_RUNTIME; a
    failed call leaves the outputs untouched"""
    eng = _engine(pkg, "fp32")
    obs = np.ascontiguousarray(_observations())
    big = np.zeros((MAXB + 1, 4, 84, 84), np.uint8)
    untouched = lambda *arrays: all((a == (9 if a.dtype == np.uint8 else -7)).all() for a in arrays)
    bad_cfg = [dict(stride=1), dict(stride=85), dict(stride=-12), dict(sigma_mask=0.25), dict(sigma_mask=17.0),
               dict(sigma_mask=float("nan")), dict(sigma_blur=0.25), dict(sigma_blur=10.5), dict(sigma_blur=float("inf")),
               dict(planes=0), dict(planes=16), dict(planes=-1)]
    for kw in bad_cfg:
        rc, *arrays = _raw(pkg, eng, obs, 0, 3, **kw)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(*arrays), kw
        rc, out = _raw_perturbed(pkg, eng, obs, 0, 3, 0, 1, **kw)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), kw
    for o, first, n in ((obs, 0, 0), (obs, 0, -1), (big, 0, MAXB + 1), (obs, 1, 2)):
        rc, *arrays = _raw(pkg, eng, o, first, n)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(*arrays), (first, n)
        rc, out = _raw_perturbed(pkg, eng, o, first, n, 0, 1)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), (first, n)
    for null in ("policy", "value"):
        rc, *arrays = _raw(pkg, eng, obs, 0, 3, null=(null,))
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(*arrays), null
    assert _raw_perturbed(pkg, eng, obs, 0, 3, 0, 1, null_out=True)[0] == pkg.ERR_INVALID_ARGUMENT
    for p0, count in ((-1, 1), (49, 1), (0, 0), (0, 50), (48, 2), (10, -1)):  # P = 49
        rc, out = _raw_perturbed(pkg, eng, obs, 0, 3, p0, count)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), (p0, count)
    # the batch source without a batch
    rc, *arrays = _raw(pkg, eng, None, 0, 2)
    assert rc == pkg.ERR_RUNTIME and untouched(*arrays)
    rc, out = _raw_perturbed(pkg, eng, None, 0, 2, 0, 1)
    assert rc == pkg.ERR_RUNTIME and untouched(out)
    with pytest.raises(pkg.AleppoError, match="no batch"):
        eng.saliency(first=0, n=2)
    with pytest.raises(pkg.AleppoInvalidArgument, match="capacity"):
        eng.saliency(big)
    with pytest.raises(pkg.AleppoInvalidArgument, match="stride"):
        eng.saliency(obs, stride=1)
    # ... and with one: a range outside it
    _rollout(eng, 8900)
    for first, n in ((-1, 2), (0, 0), (0, E * T + 1), (E * T, 1), (E * T - 1, 2), (5, -3)):
        rc, *arrays = _raw(pkg, eng, None, first, n)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(*arrays), (first, n)
        rc, out = _raw_perturbed(pkg, eng, None, first, n, 0, 1)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), (first, n)
    rc, pol, val, out = _raw(pkg, eng, None, E * T - 1, 1)
    assert rc == pkg.OK and (pol != -7).all() and (val != -7).all() and (out != -7).all()
    assert _raw(pkg, eng, obs, 0, 3, want_outputs=False)[0] == pkg.OK
    # while a step is armed
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(8950, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    rc, *arrays = _raw(pkg, eng, obs, 0, 3)
    assert rc == pkg.ERR_RUNTIME and untouched(*arrays)
    rc, out = _raw_perturbed(pkg, eng, obs, 0, 3, 0, 1)
    assert rc == pkg.ERR_RUNTIME and untouched(out)
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    assert _raw(pkg, eng, obs, 0, 3)[0] == pkg.OK
    eng.synchronize()
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()


# ------------------------------------------------------------------ the trainer writes the video
@pytest.mark.gpu
def test_trainer_writes_a_saliency_video(tmp_path):
    """trainer/train on the debug configuration (8 environments x T = 32, fp32) with record_saliency: true at stride 12: one
    C444 y4m per rollout with T frames, the game's frames as luma, U and V constant over each grid cell, never below 128 and
    255 at the file's maximum"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    from __graft_entry__ import build
    build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer")])
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read().replace("num_rollouts: 10", "num_rollouts: 2")
    cfg = tmp_path / "debug.yaml"
    cfg.write_text(txt + "record_saliency: true\nsaliency_stride: 12\nsaliency_sigma_mask: 4\nsaliency_sigma_blur: 2\n")
    os.makedirs(tmp_path / "tb")
    r = subprocess.run([os.path.join(ROOT, "trainer", "train"), "breakout.bin", str(tmp_path / "tb" / "run.log"),
                        str(tmp_path / "video"), "g", str(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "video")) == ["saliency_1.y4m", "saliency_2.y4m"]
    header = b"YUV4MPEG2 W84 H84 F15:1 Ip A1:1 C444 XALEPPO_Y=channel0_newest\n"
    cells = sr.upsample(np.arange(49).reshape(7, 7), 12)
    for name in ("saliency_1.y4m", "saliency_2.y4m"):
        blob = open(tmp_path / "video" / name, "rb").read()
        assert blob.startswith(header) and len(blob) == len(header) + 32 * (6 + 3 * 7056)
        yuv = np.frombuffer(blob, np.uint8, offset=len(header)).reshape(32, 6 + 3 * 7056)[:, 6:].reshape(32, 3, 84, 84)
        assert yuv[:, 0].any(axis=(1, 2)).all() and len({f.tobytes() for f in yuv[:, 0]}) > 1  # frames of the game, not one
        for plane in (1, 2):
            assert yuv[:, plane].min() >= 128 and yuv[:, plane].max() == 255  # a non-zero maximum, scaled to 255
            for c in range(49):  # one value per grid cell
                cell = yuv[:, plane][:, cells == c]
                assert (cell == cell[:, :1]).all(), (name, plane, c)
