"""aleppo_snapshot_* and aleppo_policy_diff: two parameter sets compared on the device (policy churn).

CPU (not marked gpu): the header's constants and prototypes against the Python mirror, the null-context refusals, the
reference's known answers (tests/policy_diff_ref.py), the planted errors the bound has to reject, the float64 reference
against its np.longdouble restatement at a quarter of the bound, and the margins of the GPU fixtures on the oracle's
forward in all three oracle modes (a comparison that moves no greedy action would let a test pass on a degenerate case).
GPU: `outputs` are the bits of aleppo_forward on engines that hold each set and within the forward bounds of the oracle;
stats, per-sample columns and transitions against the reference on the engine's own outputs and fc exports; identical
sets; the three sets; determinism and isolation of a training run; non-finite rows; a recycle; the errors.

Where the margins apply: churn strictly between 0.1 and 0.6 and two off-diagonal transition cells need more than one row
and more than one action, so the fixtures with n = 1 or A = 1 (which the rows of the issue include) are held to what they
can show instead - a policy that moved (tv > 0.01) at n = 1, features and a value that moved at A = 1."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
import policy_diff_ref as pdr
import trainer_helpers
from conftest import ROOT
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

# name: (parameter seed, H, A, n, observation seed, perturbation size, max_minibatch)
CASES = {"h32a4n1": (9900, 32, 4, 1, 9950, 0.5, 64), "h32a1": (9905, 32, 1, 37, 9951, 0.5, 64),
         "h96a18": (9910, 96, 18, 37, 9952, 0.5, 64), "h512a4": (9920, 512, 4, 37, 9953, 0.5, 64),
         "n260": (9930, 32, 4, 260, 9954, 0.85, 64)}
MODES = dict(fp32={}, bf16=dict(emulate_bf16=True), floor=dict(emulate_bf16=True, sums="float32"))
I, COL = pdr.IDX, pdr.COL
ZERO_STATS = ("churn", "mean_kl_ab", "max_kl_ab", "mean_kl_ba", "mean_tv", "max_tv", "mean_abs_dv", "max_abs_dv", "rms_dv",
              "feature_rel_change")


@functools.lru_cache(maxsize=None)
def _obs(seed, n):
    """hashed bytes, each plane of each sample cut to a hashed window: so that the samples' greedy actions differ"""
    a = hf.hf_bytes(seed, (n, 4, 84, 84))
    r = (hf.hf_u32(seed + 1, n * 16) % np.uint32(84)).reshape(n, 4, 4)
    yy, xx = np.arange(84)[:, None], np.arange(84)[None, :]
    for i in range(n):
        for c in range(4):
            (y0, y1), (x0, x1) = sorted(r[i, c, :2]), sorted(r[i, c, 2:])
            a[i, c] *= ((yy >= y0) & (yy <= y1) & (xx >= x0) & (xx <= x1)).astype(np.uint8)
    a.setflags(write=False)
    return a


def _perturbed(p, seed, H, A, eps):
    """p plus a hashed perturbation: every tensor moved by up to eps times the bound it was filled within"""
    fan_in = [256, 0, 512, 0, 576, 0, 3136, 0, H, 0, H, 0]
    out, at = [], 0
    for k, shp in enumerate(hf.param_shapes(H, A)):
        n = int(np.prod(shp))
        b = np.float32(0.05) if k % 2 else np.sqrt(np.float32(6.0) / np.float32(fan_in[k])).astype(np.float32)
        out.append(p[at:at + n] + np.float32(eps) * b * hf.hf_range(seed + k, (n,), -1, 1))
        at += n
    return np.concatenate(out).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sets(case):
    seed, H, A, _, _, eps, _ = CASES[case]
    a = hf.fill_params(seed, H, A)
    b = _perturbed(a, seed + 40, H, A, eps)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _oracle(case, mode):
    """the oracle's (logits_a, values_a, h_a, logits_b, values_b, h_b) of a case"""
    _, H, A, n, oseed, _, _ = CASES[case]
    out = []
    for p in _sets(case):
        l, v, acts = orc.net_forward(p, H, A, _obs(oseed, n), want_acts=True, **MODES[mode])
        out += [l, v, np.ascontiguousarray(np.asarray(acts, np.float32)[:, -H:])]
    for x in out:
        x.setflags(write=False)
    return tuple(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _off_diagonal_cells(t):
    return int((t - np.diag(np.diag(t)) > 0).sum())


def _margins(case, ref):
    """what keeps a fixture from being a degenerate comparison (see the module docstring); a list of complaints"""
    _, H, A, n, _, _, _ = CASES[case]
    st, bad = ref["stats"], []
    if n > 1 and A > 1:
        if not 0.1 < st[I["churn"]] < 0.6:
            bad.append(f"churn {st[I['churn']]}")
        if _off_diagonal_cells(ref["transitions"]) < 2:
            bad.append("fewer than two off-diagonal transition cells")
    elif A > 1:
        if not st[I["max_tv"]] > 0.01:
            bad.append(f"tv {st[I['max_tv']]}")
    if not (st[I["mean_abs_dv"]] > 1e-3 and st[I["feature_rel_change"]] > 0.05 and st[I["mean_feature_cos"]] < 0.99):
        bad.append("value or features did not move")
    return bad


# ------------------------------------------------------------------ CPU: constants and prototypes
def test_header_constants_and_prototypes_match_the_python_mirror():
    pkg = load_package()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)
    const = functools.partial(trainer_helpers.header_const, stripped=True)
    assert const("ALEPPO_PD_COUNT") == pkg.PD_COUNT == len(pdr.STATS) == len(pkg.PD_STATS) == 16
    assert const("ALEPPO_PD_ROW") == pkg.PD_ROW == len(pdr.COLUMNS) == len(pkg.PD_COLUMNS) == 8
    for i, name in enumerate(pdr.STATS):
        assert const("ALEPPO_PD_" + name.upper()) == pkg.PD_STATS[name] == i
    for i, name in enumerate(pdr.COLUMNS):
        assert pkg.PD_COLUMNS[name] == i
    assert (const("ALEPPO_SET_LIVE"), const("ALEPPO_SET_AVERAGED"), const("ALEPPO_SET_SNAPSHOT")) == (0, 1, 2)
    assert (pkg.SET_LIVE, pkg.SET_AVERAGED, pkg.SET_SNAPSHOT) == (0, 1, 2)
    assert pkg.SETS == dict(live=0, averaged=1, snapshot=2)
    for f in ("aleppo_snapshot_take", "aleppo_snapshot_export", "aleppo_snapshot_import", "aleppo_policy_diff"):
        assert f in pkg.EXPORTS
    for m in ("snapshot_take", "snapshot_params", "load_snapshot", "policy_diff"):
        assert hasattr(pkg.Engine, m)
    flat = re.sub(r"\s+", " ", hdr)
    assert "int aleppo_snapshot_take(aleppo_ctx *ctx, int source_set);" in flat
    assert "int aleppo_snapshot_export(aleppo_ctx *ctx, float *flat, size_t count);" in flat
    assert "int aleppo_snapshot_import(aleppo_ctx *ctx, const float *flat, size_t count);" in flat
    assert ("int aleppo_policy_diff(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, int set_a, int set_b, "
            "double *stats, size_t stat_count, double *per_sample, size_t per_sample_count, int64_t *transitions, "
            "size_t transition_count, float *outputs, size_t output_count);") in flat
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


def test_a_null_context_is_refused_before_any_device_work():
    pkg = load_package()
    lib = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    obs = np.zeros((1, 4, 84, 84), np.uint8)
    stats, flat = np.full(16, -7.0), np.full(8, -7.0, np.float32)
    assert lib.aleppo_policy_diff(None, p(obs), C.c_int64(1), 0, 0, p(stats), C.c_size_t(16), None, C.c_size_t(0), None,
                                  C.c_size_t(0), None, C.c_size_t(0)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_snapshot_take(None, 0) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_snapshot_export(None, p(flat), C.c_size_t(8)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_snapshot_import(None, p(flat), C.c_size_t(8)) == pkg.ERR_INVALID_ARGUMENT
    assert (stats == -7).all() and (flat == -7).all()


# ------------------------------------------------------------------ CPU: the reference's known answers
def _synthetic(seed, n, H, A):
    return (hf.hf_range(seed, (n, A), -2, 2), hf.hf_range(seed + 1, (n,), -1, 1), hf.hf_range(seed + 2, (n, H), -1, 1))


def test_reference_known_answers():
    n, H, A = 23, 32, 5
    la, va, ha = _synthetic(9960, n, H, A)
    # identical sets: zeros, cos 1, a diagonal transition matrix
    r = pdr.reference(la, va, ha, la, va, ha)
    st = r["stats"]
    assert st[I["rows"]] == n and st[I["nonfinite_rows"]] == 0
    assert all(st[I[k]] == 0 for k in ZERO_STATS)
    assert np.abs(r["per_sample"][:, COL["cos"]] - 1).max() <= 4 * 2.0 ** -53
    assert (r["per_sample"][:, [COL[k] for k in ("kl_ab", "kl_ba", "tv", "dv", "dh2")]] == 0).all()
    assert _off_diagonal_cells(r["transitions"]) == 0 and r["transitions"].sum() == n
    assert st[I["mean_entropy_a"]] == st[I["mean_entropy_b"]] > 0
    # a permuted head (logits rolled by one action): every greedy action moves, KL is the closed form
    lb = np.roll(la, 1, axis=1)
    r = pdr.reference(la, va, ha, lb, va, ha)
    lp = np.log(np.exp(la.astype(np.float64) - la.astype(np.float64).max(1, keepdims=True)))
    lp -= np.log(np.exp(lp).sum(1, keepdims=True))
    kl = (np.exp(lp) * (lp - np.roll(lp, 1, axis=1))).sum(1)
    assert r["stats"][I["churn"]] == 1 and np.trace(r["transitions"]) == 0
    np.testing.assert_allclose(r["per_sample"][:, COL["kl_ab"]], kl, rtol=0, atol=1e-14)
    np.testing.assert_allclose(r["stats"][I["mean_kl_ab"]], kl.mean(), rtol=0, atol=1e-14)
    assert (r["per_sample"][:, COL["g_b"]] == (r["per_sample"][:, COL["g_a"]] + 1) % A).all()
    assert r["stats"][I["mean_abs_dv"]] == 0 and r["stats"][I["feature_rel_change"]] == 0
    # two actions, p_a = (1/2, 1/2), p_b = (1/4, 3/4): the closed forms; the tie of set a takes the lowest index
    l2a = np.zeros((1, 2), np.float32)
    l2b = np.log(np.array([[1.0, 3.0]])).astype(np.float32)
    h1 = np.array([[3.0, 4.0]], np.float32)
    r = pdr.reference(l2a, [1.0], h1, l2b, [-0.5], 2 * h1)
    pb = np.exp(l2b.astype(np.float64)) / np.exp(l2b.astype(np.float64)).sum()
    row = r["per_sample"][0]
    np.testing.assert_allclose(row[COL["kl_ab"]], (0.5 * (np.log(0.5) - np.log(pb))).sum(), atol=1e-15)
    np.testing.assert_allclose(row[COL["kl_ba"]], (pb * (np.log(pb) - np.log(0.5))).sum(), atol=1e-15)
    np.testing.assert_allclose(row[COL["tv"]], 0.5 * np.abs(pb - 0.5).sum(), atol=1e-15)
    assert row[COL["dv"]] == -1.5 and row[COL["cos"]] == 1 and row[COL["dh2"]] == 25
    assert row[COL["g_a"]] == 0 and row[COL["g_b"]] == 1 and r["transitions"].tolist() == [[0, 1], [0, 0]]
    np.testing.assert_allclose(r["stats"][I["mean_entropy_a"]], np.log(2.0), atol=1e-15)
    assert r["stats"][I["feature_rel_change"]] == 1 and r["stats"][I["rms_dv"]] == 1.5
    # a tie between actions 1 and 3 takes 1
    lt = np.array([[0.0, 2.0, -1.0, 2.0]], np.float32)
    assert pdr.reference(lt, [0], h1, lt[:, ::-1], [0], h1)["per_sample"][0, COL["g_a"]:].tolist() == [1, 0]
    # a zero feature row: cos is 1 by definition
    assert pdr.reference(l2a, [0], 0 * h1, l2a, [0], h1)["per_sample"][0, COL["cos"]] == 1
    # a NaN row is counted and left out of everything else
    hb = ha.copy()
    hb[4, 7] = np.nan
    lb = la.copy()
    lb[9, 2] = np.inf
    r, clean = pdr.reference(la, va, ha, lb, va, hb), pdr.reference(np.delete(la, (4, 9), 0), np.delete(va, (4, 9)),
                                                                   np.delete(ha, (4, 9), 0), np.delete(lb, (4, 9), 0),
                                                                   np.delete(va, (4, 9)), np.delete(hb, (4, 9), 0))
    assert r["stats"][I["rows"]] == n - 2 and r["stats"][I["nonfinite_rows"]] == 2
    assert np.array_equal(r["stats"][2:], clean["stats"][2:]) and np.isfinite(r["stats"]).all()
    assert np.isnan(r["per_sample"][[4, 9]]).all() and np.isfinite(np.delete(r["per_sample"], (4, 9), 0)).all()
    assert np.array_equal(r["transitions"], clean["transitions"])
    none = pdr.reference(la[:2], va[:2], ha[:2] * np.nan, la[:2], va[:2], ha[:2])
    assert none["stats"].tolist() == [0, 2] + [0] * 14 and np.isnan(none["per_sample"]).all()
    # A = 1: one action, no policy to move; value and features still do
    l1 = hf.hf_range(9970, (n, 1), -2, 2)
    r = pdr.reference(l1, va, ha, -l1, va + 1, -ha)
    assert all(r["stats"][I[k]] == 0 for k in ("churn", "mean_kl_ab", "max_kl_ab", "mean_kl_ba", "mean_tv", "max_tv",
                                                "mean_entropy_a", "mean_entropy_b"))
    assert r["transitions"].tolist() == [[n]] and r["stats"][I["min_feature_cos"]] == pytest.approx(-1, abs=1e-15)
    np.testing.assert_allclose(r["stats"][[I["mean_abs_dv"], I["rms_dv"], I["feature_rel_change"]]], [1, 1, 2], rtol=1e-7)


# ------------------------------------------------------------------ CPU: planted errors, the longdouble restatement
def _planted_fixture():
    """the oracle's fp32 forward of the H = 96 case with a tie planted in row 3 of both sets and a NaN in row 5 of h_b"""
    la, va, ha, lb, vb, hb = (x.copy() for x in _oracle("h96a18", "fp32"))
    la[3, 11] = la[3].max()
    la[3, 2] = la[3, 11]
    lb[3, 16] = lb[3].max()
    lb[3, 0] = lb[3, 16]
    hb[5, 40] = np.nan
    return la, va, ha, lb, vb, hb


@pytest.mark.parametrize("plant", pdr.PLANTS)
def test_planted_errors_are_rejected(plant):
    fx = _planted_fixture()
    ref = pdr.reference(*fx)
    assert ref["stats"][I["nonfinite_rows"]] == 1 and pdr.check(ref["stats"], ref["per_sample"], ref["transitions"], ref) == ([], 0.0)
    wrong = pdr.reference(*fx, plant=plant)
    bad, worst = pdr.check(wrong["stats"], wrong["per_sample"], wrong["transitions"], ref)
    print(plant, bad, worst)
    if plant == "tie_high":  # integers: exact, so any difference is one
        assert "g_a: differs" in bad and "g_b: differs" in bad and "transitions differ" in bad
    elif plant == "count_nonfinite":
        assert any(b.startswith("rows:") for b in bad) and any(b.startswith("nonfinite_rows:") for b in bad)
        assert any("NaN pattern" in b for b in bad)
    else:
        assert bad and worst >= 1e6, (bad, worst)
        col = dict(kl_swap="kl_ab", tv_whole="tv", dv_sign="dv", drop_last="dh2")[plant]
        assert any(b.startswith(col + ":") for b in bad)


@pytest.mark.parametrize("case", list(CASES))
def test_float64_reference_against_its_longdouble_restatement(case):
    """what float64 itself loses on the GPU fixtures stays within a quarter of the bound"""
    fx = _oracle(case, "fp32")
    r64, rld = pdr.reference(*fx), pdr.reference(*fx, dtype=np.longdouble)
    bad, worst = pdr.check(r64["stats"], r64["per_sample"], r64["transitions"], rld)
    print(case, "float64 against longdouble: worst", worst, "of the bound")
    assert not bad and worst <= 0.25, (bad, worst)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_fixtures_are_no_degenerate_comparison(case, mode):
    ref = pdr.reference(*_oracle(case, mode))
    print(case, mode, "churn", ref["stats"][I["churn"]], "off-diagonal cells", _off_diagonal_cells(ref["transitions"]),
          "max tv", ref["stats"][I["max_tv"]], "feature change", ref["stats"][I["feature_rel_change"]])
    assert ref["stats"][I["nonfinite_rows"]] == 0
    assert not _margins(case, ref), _margins(case, ref)


# ------------------------------------------------------------------ GPU
def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


def _engine(pkg, case, prec, params, E=8, T=8):
    _, H, A, _, _, _, mm = CASES[case]
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec), max_minibatch=mm)
    eng.load_params(params)
    return eng


def _forward_all(eng, obs, chunk=64):
    """(logits, values, fc) of aleppo_forward / aleppo_forward_activations in chunks of at most `chunk` samples"""
    parts = []
    for i in range(0, obs.shape[0], chunk):
        l, v = eng.forward(obs[i:i + chunk])
        parts.append((l, v, eng.forward_activations(obs[i:i + chunk], layers=("fc",))["fc"]))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _split(outputs, A):
    return outputs[0][:, :A], outputs[0][:, A], outputs[1][:, :A], outputs[1][:, A]


def _stats_array(d):
    return np.array([d["stats"][k] for k in pdr.STATS])


def _check_call(tag, got, h_a, h_b, A):
    la, va, lb, vb = _split(got["outputs"], A)
    ref = pdr.reference(la, va, h_a, lb, vb, h_b)
    bad, worst = pdr.check(_stats_array(got), got["per_sample"], got["transitions"], ref)
    print(f"{tag}: worst {worst:.3g} of the bound; churn {got['stats']['churn']:.3g}")
    assert not bad, (tag, bad)
    return ref, worst


@functools.lru_cache(maxsize=None)
def _batch_planes(seed, n, A):
    return ((hf.hf_u32(seed + 2, n) % np.uint32(A)).astype(np.int64), orc.log_softmax(hf.hf_range(seed + 3, (n, A), -1, 1)),
            hf.hf_range(seed + 4, (n,), -1, 1), hf.hf_range(seed + 5, (n,), -1, 1),
            (hf.hf_unit(seed + 6, n) >= np.float32(0.1)).astype(np.uint8))


_RUNS = {}


def _run(pkg, case, prec):
    """one case on the GPU, shared by the tests that read it: set a in the snapshot and set b live on one engine (the
    snapshot is taken BEFORE set b is loaded: aleppo_load_params must leave it alone), a second engine whose live
    parameters are set a for the references.  n260 goes through the batch source: 260 samples in chunks of 64, 64, 64, 64, 4."""
    if (case, prec) in _RUNS:
        return _RUNS[case, prec]
    _, H, A, n, oseed, _, _ = CASES[case]
    pa, pb = _sets(case)
    obs = _obs(oseed, n)
    T = 33 if case == "n260" else 8
    main, ea = _engine(pkg, case, prec, pa, T=T), _engine(pkg, case, prec, pa, T=T)
    main.snapshot_take("live")
    main.load_params(pb)
    if case == "n260":
        main.set_batch(obs, *_batch_planes(9980, n, A))
        src = None
    else:
        src = obs
    got = main.policy_diff("snapshot", "live", src, per_sample=True, transitions=True, outputs=True)
    again = main.policy_diff("snapshot", "live", src, per_sample=True, transitions=True, outputs=True)
    plain = main.policy_diff("snapshot", "live", src)
    out = dict(got=got, again=again, plain=plain, fwd_a=_forward_all(ea, obs), fwd_b=_forward_all(main, obs),
               snapshot=main.snapshot_params())
    main.close()
    ea.close()
    _RUNS[case, prec] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_outputs_are_the_same_forward(pkg, prec, case):
    """the ParamView forward is THE forward: set a's block (read from the snapshot) equals aleppo_forward on an engine whose
    live parameters are set a, bit for bit, and set b's the engine's own; both are within the forward bounds of the oracle"""
    _, H, A, n, oseed, _, _ = CASES[case]
    run = _run(pkg, case, prec)
    out = run["got"]["outputs"]
    assert out.shape == (2, n, A + 1)
    la, va, lb, vb = _split(out, A)
    for tag, (l, v), (fl, fv, _) in (("a", (la, va), run["fwd_a"]), ("b", (lb, vb), run["fwd_b"])):
        assert np.array_equal(_bits(l), _bits(fl)) and np.array_equal(_bits(v), _bits(fv)), tag
    assert np.array_equal(_bits(run["snapshot"]), _bits(_sets(case)[0]))  # load_params(set b) left the snapshot alone
    assert not np.array_equal(la, lb)
    for p, l, v in zip(_sets(case), (la, lb), (va, vb)):
        if prec == "fp32":
            wl, wv = orc.net_forward(p, H, A, _obs(oseed, n))
            np.testing.assert_allclose(l, wl, atol=1e-4, rtol=0)
            np.testing.assert_allclose(v, wv, atol=1e-4, rtol=0)
        else:
            c = bc.Checker()
            c.forward(l, v, bc.emulated_forward(p, H, A, _obs(oseed, n)))
            assert not c.failures, c.failures


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_stats_rows_and_transitions_against_the_reference(pkg, prec, case):
    """Measured on an MI355X: see DESIGN.md 4n for the worst value / bound of every row."""
    _, H, A, n, _, _, _ = CASES[case]
    run = _run(pkg, case, prec)
    got = run["got"]
    assert got["per_sample"].shape == (n, 8) and got["transitions"].shape == (A, A) and got["transitions"].dtype == np.int64
    ref, _ = _check_call(f"policy_diff {prec} {case}", got, run["fwd_a"][2], run["fwd_b"][2], A)
    assert got["stats"]["rows"] == n and got["stats"]["nonfinite_rows"] == 0 and got["transitions"].sum() == n
    assert not _margins(case, ref), _margins(case, ref)
    # two calls return the same bits; the optional outputs are optional
    for k in ("per_sample", "transitions", "outputs"):
        assert np.array_equal(_bits(got[k]), _bits(run["again"][k])), k
        assert run["plain"][k] is None
    assert np.array_equal(_bits(_stats_array(got)), _bits(_stats_array(run["again"])))
    assert np.array_equal(_bits(_stats_array(got)), _bits(_stats_array(run["plain"])))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["h96a18", "n260"])
def test_identical_sets(pkg, prec, case):
    _, H, A, n, oseed, _, _ = CASES[case]
    obs = _obs(oseed, n)[:64]
    eng = _engine(pkg, case, prec, _sets(case)[1])
    for a, b in (("live", "live"), ("snapshot", "live"), ("snapshot", "snapshot"), ("live", "snapshot")):
        if (a, b) == ("snapshot", "live"):
            eng.snapshot_take("live")
        got = eng.policy_diff(a, b, obs, per_sample=True, transitions=True, outputs=True)
        st, ps = got["stats"], got["per_sample"]
        assert st["rows"] == obs.shape[0] and st["nonfinite_rows"] == 0
        assert all(st[k] == 0 for k in ZERO_STATS), (a, b, st)
        assert (ps[:, [COL[k] for k in ("kl_ab", "kl_ba", "tv", "dv", "dh2")]] == 0).all()
        assert np.abs(ps[:, COL["cos"]] - 1).max() <= 4 * 2.0 ** -53
        assert abs(st["min_feature_cos"] - 1) <= 4 * 2.0 ** -53
        assert abs(st["mean_feature_cos"] - 1) <= (4 + obs.shape[0]) * 2.0 ** -53  # (a sum of n terms: n more roundings)
        assert _off_diagonal_cells(got["transitions"]) == 0 and got["transitions"].sum() == obs.shape[0]
        assert (ps[:, COL["g_a"]] == ps[:, COL["g_b"]]).all() and st["mean_entropy_a"] == st["mean_entropy_b"] > 0
        assert np.array_equal(_bits(got["outputs"][0]), _bits(got["outputs"][1]))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_three_sets(pkg, prec):
    """averaged = 0.5 a + 0.5 b (imported a, one update at decay 0.5 towards the live b); its snapshot against live equals
    the reference on ema_params() and the live export; load_snapshot / snapshot_params move bits"""
    case = "h96a18"
    _, H, A, n, oseed, _, _ = CASES[case]
    pa, pb = _sets(case)
    obs = _obs(oseed, n)
    eng = _engine(pkg, case, prec, pb)
    eng.ema_open()
    eng.load_ema(pa)
    eng.ema_update(0.5)
    avg, _ = eng.ema_params()
    assert not np.array_equal(avg, pa) and not np.array_equal(avg, pb)
    direct = eng.policy_diff("averaged", "live", obs, per_sample=True, transitions=True, outputs=True)
    eng.snapshot_take("averaged")
    assert np.array_equal(_bits(eng.snapshot_params()), _bits(avg))
    got = eng.policy_diff("snapshot", "live", obs, per_sample=True, transitions=True, outputs=True)
    for k in ("per_sample", "transitions", "outputs"):
        assert np.array_equal(_bits(got[k]), _bits(direct[k])), k
    assert np.array_equal(_bits(_stats_array(got)), _bits(_stats_array(direct)))
    assert np.array_equal(_bits(eng.export_params()), _bits(pb))
    # later EMA calls leave the snapshot alone
    eng.ema_update(0.25)
    eng.ema_open()
    assert np.array_equal(_bits(eng.snapshot_params()), _bits(avg))
    e_avg = _engine(pkg, case, prec, avg)
    fa, fb = _forward_all(e_avg, obs), _forward_all(eng, obs)
    la, va, lb, vb = _split(got["outputs"], A)
    assert np.array_equal(_bits(la), _bits(fa[0])) and np.array_equal(_bits(va), _bits(fa[1]))
    assert np.array_equal(_bits(lb), _bits(fb[0])) and np.array_equal(_bits(vb), _bits(fb[1]))
    ref, _ = _check_call(f"averaged against live {prec}", got, fa[2], fb[2], A)
    assert ref["stats"][I["max_tv"]] > 0.01
    # a checkpoint from disk: import, export, compare
    eng.load_snapshot(pa)
    assert np.array_equal(_bits(eng.snapshot_params()), _bits(pa))
    e_a = _engine(pkg, case, prec, pa)
    got = eng.policy_diff("live", "snapshot", obs, outputs=True)
    fa = _forward_all(e_a, obs)
    assert np.array_equal(_bits(got["outputs"][1][:, :A]), _bits(fa[0])) and np.array_equal(_bits(got["outputs"][1][:, A]), _bits(fa[1]))
    for e in (eng, e_avg, e_a):
        e.close()


def _rollout(eng, seed, E, T):
    start = np.ones(E, np.uint8)
    acts = []
    for t in range(T):
        acts.append(eng.act().copy())
        te = ((hf.hf_unit(seed + 100 + t, E) < 0.1) & (start == 0)).astype(np.uint8)
        eng.step(hf.hf_bytes(seed + t, (E, 84, 84)), hf.hf_range(seed + 200 + t, (E,), -2, 2), te, np.zeros(E, np.uint8), start)
        start = te
    eng.finish_rollout()
    return acts


def _twin(pkg, prec, probes):
    E, T, H, A = 8, 8, 64, 6
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec), seed=3)
    eng.load_params(hf.fill_params(9600, H, A))
    eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    out = dict(acts=[], metrics=[], digests=[], replays=[], states=[], seen=[])
    for r in range(2):
        out["acts"] += _rollout(eng, 9700 + 1000 * r, E, T)
        if probes:
            eng.snapshot_take("live")
            out["seen"].append(eng.policy_diff("snapshot", "live")["stats"])  # identical sets, the batch source
        m = eng.train(2.5e-4, 2, 2)
        if probes:
            out["seen"].append(eng.policy_diff("snapshot", "live", transitions=True)["stats"])
            out["seen"].append(eng.policy_diff("live", "snapshot", _obs(9950, 5))["stats"])
        out["metrics"].append(np.stack([m[k] for k in sorted(m)]))
        out["digests"].append(eng.state_digest())
        out["replays"].append(eng.get_option(pkg.OPT_UPDATE_GRAPH))
        sd = eng.state_dict()
        out["states"].append(np.concatenate([sd["params"], sd["exp_avg"], sd["exp_avg_sq"], [np.float32(sd["step"])]]))
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_calling_changes_nothing(pkg, prec):
    """twins from one seed run rollout -> captured update twice; one takes a snapshot before each update and compares after
    it.  Sampled actions (the second rollout's too), update metrics, state digests, parameters, moments and the graph-launch
    count are bit-identical; the update itself shows in the comparison"""
    plain, mixed = _twin(pkg, prec, False), _twin(pkg, prec, True)
    np.testing.assert_array_equal(np.stack(plain["acts"]), np.stack(mixed["acts"]))
    for r in range(2):
        assert np.array_equal(np.ascontiguousarray(plain["metrics"][r]).view(np.uint32),
                              np.ascontiguousarray(mixed["metrics"][r]).view(np.uint32)), r
        assert plain["digests"][r] == mixed["digests"][r], r
        assert np.array_equal(_bits(plain["states"][r]), _bits(mixed["states"][r])), r
    assert plain["replays"] == mixed["replays"] == [0, 1]
    before, after, back = mixed["seen"][0], mixed["seen"][1], mixed["seen"][2]
    assert before["rows"] == after["rows"] == 64 and back["rows"] == 5
    assert before["max_tv"] == 0 and before["feature_rel_change"] == 0
    assert after["max_tv"] > 0 and after["feature_rel_change"] > 0 and after["mean_kl_ab"] > 0 and after["rms_dv"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nonfinite_rows_are_counted_and_left_out(pkg, prec):
    case = "h32a4n1"
    _, H, A, _, _, _, _ = CASES[case]
    n = 37
    obs = _obs(9951, n)
    pa = _sets(case)[0]
    pb = pa.copy()
    pb[orc.param_offsets(H, A)[7] + 5] = np.nan  # one fc bias of set b: column 5 of every row of h_b
    eng = _engine(pkg, case, prec, pa)
    eng.load_snapshot(pb)
    got = eng.policy_diff("live", "snapshot", obs, per_sample=True, transitions=True, outputs=True)
    assert got["stats"]["nonfinite_rows"] == n and got["stats"]["rows"] == 0
    assert all(v == 0 for k, v in got["stats"].items() if k != "nonfinite_rows")
    assert np.isnan(got["per_sample"]).all() and not got["transitions"].any()
    assert np.isfinite(got["outputs"][0]).all() and np.isnan(got["outputs"][1]).all()
    ok = eng.policy_diff("live", "live", obs)["stats"]  # set a alone is finite
    assert ok["rows"] == n and ok["nonfinite_rows"] == 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_after_a_recycle(pkg, prec):
    """recycle_units with a snapshot taken before: how far the outputs moved equals the reference on the two exports (ReDo
    zeroes the outgoing weights; no threshold on the size is asserted)"""
    case = "h96a18"
    _, H, A, n, oseed, _, _ = CASES[case]
    obs = _obs(oseed, n)
    eng = _engine(pkg, case, prec, _sets(case)[0])
    eng.snapshot_take("live")
    mask = (hf.hf_unit(9990, 160 + H) < np.float32(0.2)).astype(np.uint8)
    counts = eng.recycle_units(mask, key=77)
    assert counts["total"] == mask.sum() > 8
    before, after = eng.snapshot_params(), eng.export_params()
    assert np.array_equal(_bits(before), _bits(_sets(case)[0])) and not np.array_equal(before, after)
    got = eng.policy_diff("snapshot", "live", obs, per_sample=True, transitions=True, outputs=True)
    e_before = _engine(pkg, case, prec, before)
    fa, fb = _forward_all(e_before, obs), _forward_all(eng, obs)
    la, va, lb, vb = _split(got["outputs"], A)
    assert np.array_equal(_bits(la), _bits(fa[0])) and np.array_equal(_bits(lb), _bits(fb[0]))
    ref, _ = _check_call(f"after a recycle {prec}", got, fa[2], fb[2], A)
    for k in ("max_tv", "max_abs_dv"):
        assert abs(got["stats"][k] - ref["stats"][I[k]]) <= pdr.bound(ref["lmax"], ref["stats"][I[k]]), k
    print(f"after a recycle {prec}: max tv {got['stats']['max_tv']:.3g}, max |dv| {got['stats']['max_abs_dv']:.3g}, "
          f"feature change {got['stats']['feature_rel_change']:.3g}")
    eng.close()
    e_before.close()


def _raw_diff(pkg, eng, obs, n, a=0, b=0, rows=None, stat_count=16, per_count=None, trans_count=None, out_count=None,
              null_stats=False):
    """the C entry point itself: (status, outputs), the outputs pre-filled with -7 so that "nothing is written" shows"""
    A = eng.A
    rows = n if rows is None else rows
    out = [np.full(16, -7.0), np.full(rows * 8, -7.0), np.full(A * A, -7, np.int64), np.full(2 * rows * (A + 1), -7.0, np.float32)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().aleppo_policy_diff(
        eng._ctx, None if obs is None else p(obs), C.c_int64(n), C.c_int(a), C.c_int(b), None if null_stats else p(out[0]),
        C.c_size_t(stat_count), p(out[1]), C.c_size_t(out[1].size if per_count is None else per_count), p(out[2]),
        C.c_size_t(out[2].size if trans_count is None else trans_count), p(out[3]),
        C.c_size_t(out[3].size if out_count is None else out_count))
    return rc, out


@pytest.mark.gpu
def test_errors(pkg):
    E, T, H, A = 8, 8, 32, 4
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    pa = _sets("h32a4n1")[0]
    eng.load_params(pa)
    obs = np.ascontiguousarray(_obs(9951, 37))
    lib, ctx = pkg.lib(), eng._ctx
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    untouched = lambda out: all((o == -7).all() for o in out)
    LIVE, AVG, SNAP = pkg.SET_LIVE, pkg.SET_AVERAGED, pkg.SET_SNAPSHOT
    flat = np.full(eng.param_count, -7.0, np.float32)
    # sets that do not exist yet: RUNTIME; nothing is written
    assert lib.aleppo_snapshot_export(ctx, p(flat), C.c_size_t(flat.size)) == pkg.ERR_RUNTIME and (flat == -7).all()
    assert lib.aleppo_snapshot_take(ctx, AVG) == pkg.ERR_RUNTIME
    assert lib.aleppo_snapshot_export(ctx, p(flat), C.c_size_t(flat.size)) == pkg.ERR_RUNTIME  # the failed take made none
    for a, b in ((SNAP, LIVE), (LIVE, SNAP), (AVG, LIVE), (LIVE, AVG)):
        rc, out = _raw_diff(pkg, eng, obs, 37, a, b)
        assert rc == pkg.ERR_RUNTIME and untouched(out), (a, b)
    # the snapshot as a take's source, unknown sets: INVALID_ARGUMENT
    for s in (SNAP, 3, -1):
        assert lib.aleppo_snapshot_take(ctx, s) == pkg.ERR_INVALID_ARGUMENT, s
    for a, b in ((3, LIVE), (LIVE, -1), (7, 7)):
        rc, out = _raw_diff(pkg, eng, obs, 37, a, b)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), (a, b)
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.policy_diff("frozen", "live", obs)
    # counts and pointers
    for kw in (dict(null_stats=True), dict(stat_count=15), dict(stat_count=17), dict(per_count=37 * 8 - 1), dict(per_count=0),
               dict(trans_count=A), dict(trans_count=A * A + 1), dict(out_count=37 * (A + 1)), dict(out_count=0)):
        rc, out = _raw_diff(pkg, eng, obs, 37, **kw)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), kw
    for o, n in ((obs, 0), (obs, -1), (obs, 65), (None, 1), (None, 37)):  # maxB = E * T = 64
        rc, out = _raw_diff(pkg, eng, o, n, rows=37)
        assert rc == pkg.ERR_INVALID_ARGUMENT and untouched(out), n
    rc, out = _raw_diff(pkg, eng, None, 0, rows=E * T)
    assert rc == pkg.ERR_RUNTIME and untouched(out)  # no batch yet
    for bad_flat, cnt in ((None, flat.size), (p(flat), flat.size - 1), (p(flat), 0)):
        assert lib.aleppo_snapshot_import(ctx, bad_flat, C.c_size_t(cnt)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_snapshot_export(ctx, p(flat), C.c_size_t(flat.size)) == pkg.ERR_RUNTIME  # still none
    eng.snapshot_take("live")
    assert lib.aleppo_snapshot_export(ctx, None, C.c_size_t(flat.size)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_snapshot_export(ctx, p(flat), C.c_size_t(flat.size + 1)) == pkg.ERR_INVALID_ARGUMENT and (flat == -7).all()
    rc2, out2 = _raw_diff(pkg, eng, obs, 37, SNAP, LIVE)
    assert rc2 == pkg.OK and out2[0][0] == 37 and out2[2].sum() == 37
    assert eng.policy_diff("snapshot", "live", obs)["stats"] == dict(zip(pdr.STATS, out2[0]))
    # while a step is armed: every call is refused, nothing changes
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(9180, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    rc, out = _raw_diff(pkg, eng, obs, 37, SNAP, LIVE)
    assert rc == pkg.ERR_RUNTIME and untouched(out)
    assert lib.aleppo_snapshot_take(ctx, LIVE) == pkg.ERR_RUNTIME
    assert lib.aleppo_snapshot_import(ctx, p(pa.copy()), C.c_size_t(pa.size)) == pkg.ERR_RUNTIME
    assert lib.aleppo_snapshot_export(ctx, p(flat), C.c_size_t(flat.size)) == pkg.ERR_RUNTIME and (flat == -7).all()
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    rc, out3 = _raw_diff(pkg, eng, obs, 37, SNAP, LIVE)
    assert rc == pkg.OK and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out2, out3))
    eng.synchronize()
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
