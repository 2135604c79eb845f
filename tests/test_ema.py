"""aleppo_ema_open / _update / _read / _export / _import and ALEPPO_OPT_EVAL_PARAMS: the exponentially averaged parameters.

CPU (not marked gpu): the numpy restatement (tests/ema_ref.py) - the rule is three fp32 roundings, the planted fused and
interpolated forms differ from it, decay = 0 returns p; the header's constants and prototypes against the Python mirror; a
NULL context is refused before any device work.
GPU: the averaged set against the restatement bit for bit and the statistics at their rounding bounds; the learner is
bit-identical with and without the average; the evaluation lanes under ALEPPO_OPT_EVAL_PARAMS = 1 act exactly like a
fresh engine loaded with the averaged parameters; import / load_params / re-open / run_state; failed calls change nothing."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import ema_ref as er
import hashfill as hf
import oracle_lib as orc
from conftest import ROOT
import trainer_helpers
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

SHAPES = {"h32": (9100, 32, 4), "h96": (9200, 96, 18)}  # name: (parameter seed, H, A) - the recycle tests' two shapes
N_BATCH, BATCH_SEED = 64, 9400
DECAYS = (0.5, 0.999, 0.0, 0.9)
LR = 2.5e-4


def _bits(a, dt=np.uint32):
    return np.ascontiguousarray(a).view(dt)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a, np.uint8), _bits(b, np.uint8))


# ------------------------------------------------------------------ CPU: the restatement
def test_the_rule_is_three_roundings_and_the_planted_forms_differ():
    n = 1 << 16
    e, p = hf.hf_range(9901, (n,), -1, 1), hf.hf_range(9902, (n,), -1, 1)
    for decay in (0.5, 0.9, 0.999, 0.1, 2.0 / 11.0):
        d, w = er.scalars(decay)
        assert d == np.float32(decay) and w == np.float32(1.0 - decay)
        want = er.update(e, p, decay)
        assert want.dtype == np.float32
        # element by element on Python scalars: each operation rounded to binary32
        for i in range(0, n, 4099):
            a = np.float32(np.float64(d) * np.float64(e[i]))  # (a 48-bit product is exact in float64: one rounding)
            b = np.float32(np.float64(w) * np.float64(p[i]))
            assert want[i] == np.float32(np.float64(a) + np.float64(b))
        fma, lerp = er.update_fma(e, p, decay), er.update_lerp(e, p, decay)
        n_fma, n_lerp = int((_bits(fma) != _bits(want)).sum()), int((_bits(lerp) != _bits(want)).sum())
        print(f"decay {decay}: fused differs on {n_fma}, interpolated on {n_lerp} of {n}")
        if decay != 0.5:  # (d = w = 0.5: both products are exact, and the planted forms may agree with the rule)
            assert n_fma > 0 and n_lerp > 0
        assert np.abs(fma.astype(np.float64) - want).max() < 1e-6 and np.abs(lerp.astype(np.float64) - want).max() < 1e-6


def test_decay_zero_returns_the_parameters_and_pads_stay_zero():
    n = 4096
    e, p = hf.hf_range(9903, (n,), -3, 3), hf.hf_range(9904, (n,), -3, 3)
    assert er.scalars(0.0) == (np.float32(0), np.float32(1))
    assert _same(er.update(e, p, 0.0), p)
    z = np.zeros(64, np.float32)
    for decay in DECAYS:
        out = er.update(z, z, decay)
        assert not out.any() and not np.signbit(out).any()
    assert [er.valid(x) for x in (0.0, 0.5, 0.999999, 1.0, -0.1, float("nan"), float("inf"), -0.0)] == \
        [True, True, True, False, False, False, False, True]


def test_statistics_restatement_known_answer():
    e, p = np.array([3, 0, 0, 4], np.float32), np.array([0, 0, 0, 0], np.float32)
    assert er.stats(e, p, 2, 0.5) == dict(updates=2.0, decay=0.5, norm=5.0, param_norm=0.0, distance=5.0, relative_distance=0.0)
    s = er.stats(e, 2 * e, 1, 0.999)
    assert s["param_norm"] == 10.0 and s["distance"] == 5.0 and s["relative_distance"] == 0.5
    assert s["decay"] == float(np.float32(0.999)) != 0.999
    assert er.stats(e, e, 0, None)["decay"] == 0.0
    assert er.padded_count(32, 4) % 64 == 0 and er.padded_count(32, 4) > 32 * 3136
    assert [er.warmup_decay(0.9, n) for n in range(4)] == [0.1, 2 / 11, 3 / 12, 4 / 13] and er.warmup_decay(0.9, 1000) == 0.9


def test_header_constants_and_prototypes_match_the_python_mirror():
    pkg = load_package()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)

    const = functools.partial(trainer_helpers.header_const, stripped=True)

    assert const("ALEPPO_EMA_STATS_COUNT") == pkg.EMA_STATS_COUNT == len(er.STATS) == 6
    for name, i in pkg.EMA_STATS.items():
        assert const("ALEPPO_EMA_" + name.upper()) == i == er.STATS.index(name)
    assert const("ALEPPO_OPT_EVAL_PARAMS") == pkg.OPT_EVAL_PARAMS == 25
    assert const("ALEPPO_K_EMA") == pkg.KERNEL_CLASSES["ema"] == 26 and const("ALEPPO_K_COUNT") == 27
    names = ("aleppo_ema_open", "aleppo_ema_update", "aleppo_ema_read", "aleppo_ema_export", "aleppo_ema_import")
    for name in names:
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    for name in ("ema_open", "ema_update", "ema_stats", "ema_params", "load_ema", "eval_use_averaged"):
        assert hasattr(pkg.Engine, name)
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int aleppo_ema_open(aleppo_ctx *ctx);", "int aleppo_ema_update(aleppo_ctx *ctx, double decay);",
                  "int aleppo_ema_read(aleppo_ctx *ctx, double out[ALEPPO_EMA_STATS_COUNT]);",
                  "int aleppo_ema_export(aleppo_ctx *ctx, float *flat, size_t count, int64_t *updates);",
                  "int aleppo_ema_import(aleppo_ctx *ctx, const float *flat, size_t count, int64_t updates);"):
        assert proto in flat, proto
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


def test_a_null_context_is_refused_before_any_device_work():
    pkg = load_package()
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    INV = pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_ema_open(None) == INV
    assert lib.aleppo_ema_update(None, C.c_double(0.5)) == INV
    out = np.full(6, -7.0)
    assert lib.aleppo_ema_read(None, ptr(out)) == INV and (out == -7).all()
    flat, updates = np.full(16, -7, np.float32), C.c_int64(-7)
    assert lib.aleppo_ema_export(None, ptr(flat), C.c_size_t(16), C.byref(updates)) == INV
    assert (flat == -7).all() and updates.value == -7
    assert lib.aleppo_ema_import(None, ptr(flat), C.c_size_t(16), C.c_int64(0)) == INV
    assert lib.aleppo_set_option(None, C.c_int(pkg.OPT_EVAL_PARAMS), C.c_int(1)) == INV


# ------------------------------------------------------------------ GPU
def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


@functools.lru_cache(maxsize=None)
def _params(shape):
    seed, H, A = SHAPES[shape]
    p = hf.fill_params(seed, H, A)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _obs(seed, shape):
    a = hf.hf_bytes(seed, shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _batch(A):
    """what aleppo_set_batch wants: N_BATCH hashed observations and the planes next to them"""
    s, n = BATCH_SEED, N_BATCH
    return (_obs(s, (n, 4, 84, 84)), (hf.hf_u32(s + 2, n) % np.uint32(A)).astype(np.int64),
            orc.log_softmax(hf.hf_range(s + 3, (n, A), -1, 1)), hf.hf_range(s + 4, (n,), -1, 1),
            hf.hf_range(s + 5, (n,), -1, 1), (hf.hf_unit(s + 6, n) >= np.float32(0.1)).astype(np.uint8))


def _engine(pkg, shape, prec, graph=False, generic=False, params=None, batch=True, **kw):
    """E = 8, T = 8, the case's hashed parameters (or `params`) and the hashed batch of 64 samples"""
    _, H, A = SHAPES[shape]
    eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec), max_minibatch=64, **kw)
    eng.load_params(_params(shape) if params is None else params)
    if graph:
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    if generic:
        eng.set_option(pkg.OPT_GENERIC_CONV, 1)
    if batch:
        eng.set_batch(*_batch(A))
    return eng


def _train(eng):
    return eng.train(LR, 1, 2)  # 1 epoch x 2 minibatches


def _check_stats(got, want, n, what):
    rb, qb = er.stat_bounds(n)
    for k in er.STATS:
        print(f"  {what} {k}: device {got[k]!r} restatement {want[k]!r}")
    assert got["updates"] == want["updates"] and got["decay"] == want["decay"], what
    for k in ("norm", "param_norm", "distance"):
        assert abs(got[k] - want[k]) <= rb * want[k], (what, k)
    assert abs(got["relative_distance"] - want["relative_distance"]) <= qb * want["relative_distance"], what


def _arithmetic_run(pkg, shape, prec):
    """open, then four train + update rounds: [(exported parameters, averaged parameters, updates, statistics)] per stage"""
    eng = _engine(pkg, shape, prec)
    eng.ema_open()
    out = [(eng.export_params(),) + eng.ema_params() + (eng.ema_stats(),)]
    for decay in DECAYS:
        _train(eng)
        eng.ema_update(decay)
        out.append((eng.export_params(),) + eng.ema_params() + (eng.ema_stats(),))
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["h32", "h96"])
def test_average_and_statistics_against_the_restatement(pkg, shape, prec):
    _, H, A = SHAPES[shape]
    n = er.padded_count(H, A)
    run = _arithmetic_run(pkg, shape, prec)
    p0, e0, u0, s0 = run[0]
    assert _same(p0, _params(shape)) and _same(e0, p0) and u0 == 0
    _check_stats(s0, er.stats(p0, p0, 0, None), n, "open")
    assert s0["norm"] == s0["param_norm"] > 0 and s0["distance"] == 0 and s0["relative_distance"] == 0 and s0["decay"] == 0
    e_prev = e0
    for k, decay in enumerate(DECAYS):
        p, e, u, s = run[k + 1]
        want = er.update(e_prev, p, decay)
        wrong = int((_bits(e) != _bits(want)).sum())
        print(f"{shape} {prec} update {k + 1} decay {decay}: {wrong} of {e.size} elements differ from the restatement; "
              f"fused form differs on {int((_bits(er.update_fma(e_prev, p, decay)) != _bits(want)).sum())}")
        assert u == k + 1 and wrong == 0
        assert not _same(p, run[k][0])  # (the update moved the parameters: the average has something to follow)
        if decay == 0.0:
            assert _same(e, p)
        else:
            assert not _same(e, p)
        _check_stats(s, er.stats(e, p, k + 1, decay), n, f"update {k + 1}")
        assert s["decay"] == float(np.float32(decay))
        e_prev = e
    again = _arithmetic_run(pkg, shape, prec)  # a second identical run: the same bits, statistics included
    for a, b in zip(run, again):
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2] == b[2]
        assert _same(np.array([a[3][k] for k in er.STATS]), np.array([b[3][k] for k in er.STATS]))


def _learner(eng, metrics):
    sd = eng.state_dict()
    return dict(params=sd["params"], exp_avg=sd["exp_avg"], exp_avg_sq=sd["exp_avg_sq"], step=np.int64(sd["step"]),
                grads=eng.export_grads(), metrics=np.stack([np.stack([m[k] for k in sorted(m)]) for m in metrics]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,prec,graph", [("h32", "fp32", 0), ("h96", "fp32", 0), ("h32", "bf16", 0), ("h96", "bf16", 0),
                                              ("h32", "bf16", 1), ("h96", "bf16", 1)])
def test_the_learner_is_untouched(pkg, shape, prec, graph):
    runs = []
    for averaged in (False, True):
        eng = _engine(pkg, shape, prec, graph=graph)
        metrics = []
        if averaged:
            eng.ema_open()
        for k in range(4):
            metrics.append(_train(eng))
            if averaged:
                eng.ema_update(DECAYS[k])
        out = _learner(eng, metrics)
        out["digest"] = eng.state_digest()
        out["replays"] = eng.get_option(pkg.OPT_UPDATE_GRAPH)
        if averaged:
            assert eng.ema_stats()["updates"] == 4 and eng.ema_stats()["distance"] > 0
        eng.close()
        runs.append(out)
    plain, avg = runs
    for k in ("params", "exp_avg", "exp_avg_sq", "step", "grads", "metrics"):
        assert _same(plain[k], avg[k]), k
    assert plain["digest"] == avg["digest"] and plain["step"] == 8
    print(f"{shape} {prec} graph={graph}: graph launches {plain['replays']} / {avg['replays']}")
    assert plain["replays"] == avg["replays"] and (plain["replays"] >= 1) == bool(graph)


LANE_FRAMES = 9600


def _lane_acts(eng, L, A, push=True):
    """two pushes of hashed frames (push), then the greedy and the sample rule with given noise: what eval_read returns"""
    if push:
        eng.eval_push_frames(_obs(LANE_FRAMES, (L, 84, 84)), np.ones(L, np.uint8))
        eng.eval_push_frames(_obs(LANE_FRAMES + 1, (L, 84, 84)), np.zeros(L, np.uint8))
    out = {}
    for rule, kw in (("greedy", {}), ("sample", dict(temperature=0.7, noise=hf.hf_range(LANE_FRAMES + 2, (L, A), 0.05, 3)))):
        acts = eng.eval_act(rule, **kw).copy()
        out[rule] = (eng.eval_read("logits"), eng.eval_read("values"), eng.eval_read("actions"), acts)
    return out


def _same_acts(a, b):
    return all(_same(x, y) for rule in a for x, y in zip(a[rule], b[rule]))


def _env_run(eng, steps=8):
    eng.eval_set_counter(0)
    eng.eval_env_open(seed_base=77, run_steps=steps)
    eng.eval_env_run("sample", temperature=1.0, steps=steps)
    planes = [eng.eval_env_read(k) for k in ("episode_returns", "episode_lengths", "game_returns", "game_lengths", "frames")]
    return planes + [eng.eval_env_state(), eng.eval_read("logits"), eng.eval_read("values"), eng.eval_read("actions"),
                     eng.eval_read("observations")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,prec,generic,L", [("h32", "fp32", 0, 3), ("h96", "fp32", 0, 3), ("h32", "bf16", 0, 3),
                                                  ("h96", "bf16", 0, 5), ("h96", "bf16", 1, 3)])
def test_the_lanes_act_on_the_average(pkg, shape, prec, generic, L):
    """A: three train + update rounds, lanes on the average.  B: a fresh engine loaded with A's averaged parameters, live
    lanes.  C: a fresh engine loaded with A's live parameters."""
    _, H, A_ = SHAPES[shape]
    a = _engine(pkg, shape, prec, generic=generic)
    a.ema_open()
    for k in range(3):
        _train(a)
        a.ema_update(0.9)
    avg, updates = a.ema_params()
    live = a.export_params()
    assert updates == 3 and not _same(avg, live)
    b = _engine(pkg, shape, prec, generic=generic, params=avg, batch=False)
    c = _engine(pkg, shape, prec, generic=generic, params=live, batch=False)
    for e in (a, b, c):
        e.eval_open(L)
    assert a.get_option(pkg.OPT_EVAL_PARAMS) == 0
    a_live = _lane_acts(a, L, A_)
    a.eval_use_averaged(True)
    assert a.get_option(pkg.OPT_EVAL_PARAMS) == 1
    a_avg = _lane_acts(a, L, A_, push=False)  # (acting does not move the stacks)
    a.eval_use_averaged(False)
    a_back = _lane_acts(a, L, A_, push=False)
    b_acts, c_acts = _lane_acts(b, L, A_), _lane_acts(c, L, A_)
    assert _same_acts(a_avg, b_acts) and _same_acts(a_live, c_acts) and _same_acts(a_back, c_acts)
    assert not _same(a_avg["greedy"][0], a_live["greedy"][0])  # (the two sets give different logits)
    # the rollout's acting keeps the live parameters: one step of hashed frames, then act with the option on, off, and on C
    E = 8
    noise = hf.hf_range(LANE_FRAMES + 3, (E, A_), 0.05, 3)
    frames, start, zero = _obs(LANE_FRAMES + 4, (E, 84, 84)), np.ones(E, np.uint8), np.zeros(E, np.uint8)
    for e in (a, c):
        e.act(noise)
        e.step(frames, np.zeros(E, np.float32), zero, zero, start)
    a.eval_use_averaged(True)
    act_on = a.act(noise).copy()
    a.eval_use_averaged(False)
    act_off = a.act(noise).copy()
    assert np.array_equal(act_on, act_off) and np.array_equal(act_on, c.act(noise))
    # device-resident evaluation environments: 8 steps of the sample rule with the built-in generator
    a.eval_use_averaged(True)
    ra, rb = _env_run(a), _env_run(b)
    assert all(_same(x, y) for x, y in zip(ra, rb))
    assert not all(_same(x, y) for x, y in zip(ra, _env_run(c)))  # (C acts on other weights: its run differs)
    # the learner never noticed
    assert _same(a.export_params(), live)
    for e in (a, b, c):
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_import_load_reopen_and_run_state(pkg, prec):
    shape, L = "h96", 3
    _, H, A_ = SHAPES[shape]
    n = er.padded_count(H, A_)
    a = _engine(pkg, shape, prec)
    a.ema_open()
    _train(a)
    a.ema_update(0.9)
    live = a.export_params()
    flat = hf.fill_params(9300, H, A_)
    a.load_ema(flat, 7)
    got, updates = a.ema_params()
    assert _same(got, flat) and updates == 7 and _same(a.export_params(), live)
    _check_stats(a.ema_stats(), er.stats(flat, live, 7, None), n, "import")
    a.eval_open(L)
    a.eval_use_averaged(True)
    b = _engine(pkg, shape, prec, params=flat, batch=False)
    b.eval_open(L)
    assert _same_acts(_lane_acts(a, L, A_), _lane_acts(b, L, A_))  # the import rebuilt the compute copy
    b.close()
    # run_state carries the average; a fresh engine that loads it holds the same average, count and lanes' weights
    _train(a)
    a.ema_update(0.5)
    rs = a.run_state()
    assert set(rs["ema"]) == {"params", "updates"} and int(rs["ema"]["updates"]) == 8
    c = _engine(pkg, shape, prec, batch=False)
    assert "ema" not in c.run_state()
    c.load_run_state(rs)
    assert _same(c.ema_params()[0], a.ema_params()[0]) and c.ema_params()[1] == 8
    assert _same(c.export_params(), a.export_params()) and c.state_digest() == a.state_digest()
    c.eval_open(L)
    c.eval_use_averaged(True)
    assert _same_acts(_lane_acts(a, L, A_, push=False), _lane_acts(c, L, A_))
    c.close()
    # a second open restarts the average at the live parameters; load_params re-initialises it at the loaded ones
    a.ema_open()
    p = a.export_params()
    assert _same(a.ema_params()[0], p) and a.ema_params()[1] == 0
    _check_stats(a.ema_stats(), er.stats(p, p, 0, None), n, "re-open")
    _train(a)
    a.ema_update(0.9)
    assert a.ema_params()[1] == 1 and not _same(a.ema_params()[0], a.export_params())
    a.load_params(flat)
    assert _same(a.ema_params()[0], flat) and a.ema_params()[1] == 0 and a.ema_stats()["distance"] == 0
    assert a.get_option(pkg.OPT_EVAL_PARAMS) == 1  # (the option stays; the lanes now act on the re-initialised average)
    a.close()


def _raw(pkg, eng):
    """one failed call of every kind but the armed step: [(what, status)], every output buffer checked for writes"""
    lib, ctx = pkg.lib(), eng._ctx
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    INV = pkg.ERR_INVALID_ARGUMENT
    n = eng.param_count
    out = []
    for what, decay in (("nan", float("nan")), ("-0.1", -0.1), ("1.0", 1.0), ("inf", float("inf")), ("-inf", float("-inf")),
                        ("2", 2.0)):
        out.append(("update decay " + what, lib.aleppo_ema_update(ctx, C.c_double(decay)) == INV))
    out.append(("read null", lib.aleppo_ema_read(ctx, None) == INV))
    flat, upd = np.full(n + 1, -7, np.float32), C.c_int64(-7)
    for what, args in (("null flat", (None, C.c_size_t(n), C.byref(upd))), ("count - 1", (ptr(flat), C.c_size_t(n - 1), C.byref(upd))),
                       ("count + 1", (ptr(flat), C.c_size_t(n + 1), C.byref(upd))), ("null updates", (ptr(flat), C.c_size_t(n), None))):
        out.append(("export " + what, lib.aleppo_ema_export(ctx, *args) == INV and (flat == -7).all() and upd.value == -7))
    src = np.ones(n + 1, np.float32)
    for what, args in (("null flat", (None, C.c_size_t(n), C.c_int64(1))), ("count - 1", (ptr(src), C.c_size_t(n - 1), C.c_int64(1))),
                       ("count + 1", (ptr(src), C.c_size_t(n + 1), C.c_int64(1))), ("updates -1", (ptr(src), C.c_size_t(n), C.c_int64(-1)))):
        out.append(("import " + what, lib.aleppo_ema_import(ctx, *args) == INV))
    for v in (2, -1):
        out.append((f"option = {v}", lib.aleppo_set_option(ctx, C.c_int(pkg.OPT_EVAL_PARAMS), C.c_int(v)) == INV))
    return out


def _every_entry_point(pkg, eng, status):
    lib, ctx = pkg.lib(), eng._ctx
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    n = eng.param_count
    st, flat, upd = np.full(6, -7.0), np.full(n, -7, np.float32), C.c_int64(-7)
    rcs = dict(update=lib.aleppo_ema_update(ctx, C.c_double(0.5)), read=lib.aleppo_ema_read(ctx, ptr(st)),
               export=lib.aleppo_ema_export(ctx, ptr(flat), C.c_size_t(n), C.byref(upd)),
               imp=lib.aleppo_ema_import(ctx, ptr(np.ones(n, np.float32)), C.c_size_t(n), C.c_int64(1)))
    assert all(rc == status for rc in rcs.values()), rcs
    assert (st == -7).all() and (flat == -7).all() and upd.value == -7
    return rcs


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_failed_calls_change_nothing(pkg, prec):
    shape = "h32"
    E = 8
    eng = _engine(pkg, shape, prec)
    _train(eng)
    digest = eng.state_digest()
    # before aleppo_ema_open: everything is ALEPPO_ERR_RUNTIME, the option included, and nothing is opened by trying
    _every_entry_point(pkg, eng, pkg.ERR_RUNTIME)
    assert pkg.lib().aleppo_set_option(eng._ctx, C.c_int(pkg.OPT_EVAL_PARAMS), C.c_int(1)) == pkg.ERR_RUNTIME
    assert eng.get_option(pkg.OPT_EVAL_PARAMS) == 0
    with pytest.raises(pkg.AleppoError, match="aleppo_ema_open"):
        eng.ema_stats()
    with pytest.raises(pkg.AleppoError, match="aleppo_ema_open"):
        eng.eval_use_averaged(True)
    assert "ema" not in eng.run_state() and eng.state_digest() == digest
    eng.ema_open()
    _train(eng)
    eng.ema_update(0.9)
    digest = eng.state_digest()
    held, stats, live = eng.ema_params(), eng.ema_stats(), eng.export_params()
    failed = _raw(pkg, eng)
    assert len(failed) == 17 and all(ok for _, ok in failed), [f for f in failed if not f[1]]
    for decay in (float("nan"), -0.1, 1.0, float("inf")):
        with pytest.raises(pkg.AleppoInvalidArgument, match="decay"):
            eng.ema_update(decay)
    with pytest.raises(pkg.AleppoInvalidArgument, match="count"):
        eng.load_ema(np.zeros(5, np.float32))

    def unchanged():
        e, u = eng.ema_params()
        return (_same(e, held[0]) and u == held[1] and eng.ema_stats() == stats and eng.state_digest() == digest and
                _same(eng.export_params(), live) and eng.get_option(pkg.OPT_EVAL_PARAMS) == 0)

    assert unchanged()
    # while a step is armed every entry point is refused like the others
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(9680, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    _every_entry_point(pkg, eng, pkg.ERR_RUNTIME)
    assert pkg.lib().aleppo_ema_open(eng._ctx) == pkg.ERR_RUNTIME
    assert pkg.lib().aleppo_set_option(eng._ctx, C.c_int(pkg.OPT_EVAL_PARAMS), C.c_int(1)) == pkg.ERR_RUNTIME
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    eng.synchronize()
    e, u = eng.ema_params()
    assert _same(e, held[0]) and u == held[1] and eng.ema_stats() == stats and _same(eng.export_params(), live)
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
