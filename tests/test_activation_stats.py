"""aleppo_forward_activations / aleppo_activation_stats: the hidden activations and their per-unit statistics.

CPU (not marked gpu): the header's constants and prototypes against the Python mirror, the null-context refusal, the
reference's known answers and what its checker rejects (tests/activation_stats_ref.py), the fixture (one dead and one
dormant unit by design) on the bf16-emulating oracle, the export bound against the plain fp32 oracle, and the trainer's
log_activation_stats keys on the host-only stand-in (tests/stub/aleppo_stub_activation_stats.cc).
GPU: the export against the oracles on every forward route, the statistics against the float64 reference built from the
engine's own export, both sample sources and the chunked batch, isolation of a training run, and the errors."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import activation_stats_ref as asr
import adam_ref as ar
import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
import trainer_helpers
from conftest import ROOT
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

TAU = 0.025
# name: (parameter seed, H, A, n, observation seed)
CASES = {"h32": (9100, 32, 4, 37, 9150), "h96": (9200, 96, 6, 37, 9250), "n260": (9300, 32, 4, 260, 9350),
         "n1": (9100, 32, 4, 1, 9160)}


@functools.lru_cache(maxsize=None)
def _obs(seed, n):
    a = hf.hf_bytes(seed, (n, 4, 84, 84))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _params(case, modified=False):
    seed, H, A, _, _ = CASES[case]
    p = hf.fill_params(seed, H, A)
    if modified:
        p = asr.modified_params(p, H, A)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _oracle_acts(case, mode, modified=False):
    """the oracle's hidden activations of a case as the export's dict; mode: "fp32", "bf16" (the emulation, double sums) or
    "floor" (the emulation with sequential fp32 sums).  Computed once and shared."""
    _, H, A, n, oseed = CASES[case]
    kw = dict(fp32={}, bf16=dict(emulate_bf16=True), floor=dict(emulate_bf16=True, sums="float32"))[mode]
    acts = orc.net_forward(_params(case, modified), H, A, _obs(oseed, n), want_acts=True, **kw)[2]
    out = asr.from_oracle_acts(acts, H)
    for a in out.values():
        a.setflags(write=False)
    return out


def _export_errors(got, ref):
    """{layer: (relative L2 of the layer, bf16_check.channel_rel per unit)} of an export against a reference export"""
    return {l: (bc.rel(got[l], ref[l]), bc.channel_rel(asr.unit_rows(got[l]), asr.unit_rows(ref[l]), ref[l].shape[1]))
            for l in asr.LAYERS}


def _export_bounds(case, modified=False):
    """bf16_check's rule per layer: max(base, FLOOR_FACTOR x the floor run's own measurement against the emulation)"""
    floor = _export_errors(_oracle_acts(case, "floor", modified), _oracle_acts(case, "bf16", modified))
    return {l: (max(bc.BOUNDS["out_rel"], bc.FLOOR_FACTOR * floor[l][0]),
                max(bc.BOUNDS["channel"], bc.FLOOR_FACTOR * floor[l][1])) for l in asr.LAYERS}, floor


# ------------------------------------------------------------------ CPU: constants and prototypes
def test_header_constants_and_prototypes_match_the_python_mirror():
    pkg = load_package()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)

    const = functools.partial(trainer_helpers.header_const, stripped=True)

    assert const("ALEPPO_ACT_UNIT_COLS") == pkg.ACT_UNIT_COLS == len(asr.UNIT_STATS) == 5
    assert const("ALEPPO_ACT_LAYER_ROWS") == len(pkg.ACT_LAYER_ROWS) == len(asr.ROWS) == 5
    assert const("ALEPPO_ACT_LAYER_COLS") == pkg.ACT_LAYER_COLS == len(asr.LAYER_STATS) == 8
    for i, name in enumerate(asr.UNIT_STATS):
        assert const("ALEPPO_ACT_" + name.upper()) == pkg.ACT_UNIT_STATS[name] == i
    for i, name in enumerate(asr.LAYER_STATS):
        assert const("ALEPPO_ACT_L_" + name.upper()) == pkg.ACT_LAYER_STATS[name] == i
    assert len(pkg.ACT_UNIT_STATS) == 5 and len(pkg.ACT_LAYER_STATS) == 8
    assert tuple(pkg.ACT_LAYERS) == asr.LAYERS and tuple(pkg.ACT_LAYER_ROWS) == asr.ROWS
    for name in ("aleppo_forward_activations", "aleppo_activation_stats"):
        assert name in pkg.EXPORTS
    assert hasattr(pkg.Engine, "forward_activations") and hasattr(pkg.Engine, "activation_stats")
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int aleppo_forward_activations(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, float *conv1, "
            "float *conv2, float *conv3, float *fc);") in flat
    assert ("int aleppo_activation_stats(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, double tau, "
            "double *units, size_t unit_count, double *layers, size_t layer_count);") in flat
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


def test_a_null_context_is_refused_before_any_device_work():
    pkg = load_package()
    lib = pkg.lib()
    obs = np.zeros((1, 4, 84, 84), np.uint8)
    units, layers = np.full((192, 5), -7.0), np.full((5, 8), -7.0)
    rc = lib.aleppo_activation_stats(None, obs.ctypes.data_as(C.c_void_p), C.c_int64(1), C.c_double(TAU),
                                     units.ctypes.data_as(C.c_void_p), C.c_size_t(units.size),
                                     layers.ctypes.data_as(C.c_void_p), C.c_size_t(layers.size))
    assert rc == pkg.ERR_INVALID_ARGUMENT and (units == -7).all() and (layers == -7).all()
    fc = np.full((1, 32), -7.0, np.float32)
    rc = lib.aleppo_forward_activations(None, obs.ctypes.data_as(C.c_void_p), C.c_int64(1), None, None, None,
                                        fc.ctypes.data_as(C.c_void_p))
    assert rc == pkg.ERR_INVALID_ARGUMENT and (fc == -7).all()


# ------------------------------------------------------------------ CPU: the reference's known answers
def _hand_made(n=3, H=32):
    acts = dict(conv1=hf.hf_range(9001, (n, 32, 20, 20), 0, 2), conv2=hf.hf_range(9002, (n, 64, 9, 9), 0, 1),
                conv3=hf.hf_range(9003, (n, 64, 7, 7), 0, 3), fc=hf.hf_range(9004, (n, H), -1, 1))
    for i, k in enumerate(("conv1", "conv2", "conv3")):  # a ReLU layer: about half of the elements are zero
        gate = hf.hf_unit(9010 + i, acts[k].size).reshape(acts[k].shape) < 0.5
        acts[k] = np.where(gate, np.float32(0), acts[k]).astype(np.float32)
    return acts


def test_reference_known_answers():
    pkg = load_package()
    assert {n: i for i, n in enumerate(asr.UNIT_STATS)} == pkg.ACT_UNIT_STATS
    assert {n: i for i, n in enumerate(asr.LAYER_STATS)} == pkg.ACT_LAYER_STATS
    n, H = 3, 32
    acts = _hand_made(n, H)
    acts["conv2"][:, 9] = 0                         # a zero channel
    acts["conv3"][1, 4, 2, 3] = np.nan              # one NaN, one Inf: each counted once and left out
    acts["conv3"][2, 4, 0, 0] = np.inf
    acts["fc"][:, 6] = [0.5, -0.25, 0.0]            # P / K and S / K by hand
    ref = asr.reference(acts, TAU)
    units, layers = ref["units"], ref["layers"]
    first = asr.first_units(H)
    assert units.shape == (160 + H, 5) and layers.shape == (5, 8)
    z = units[first[1] + 9]
    assert (z == 0).all()  # dead: mean, fraction, maximum and score 0
    assert layers[1, asr.L_DEAD] == 1 and layers[1, asr.L_DORMANT] >= 1 and layers[0, asr.L_DEAD] == 0
    u = units[first[2] + 4]
    assert u[asr.NONFINITE] == 2 and layers[2, asr.L_NONFINITE] == 2 == layers[4, asr.L_NONFINITE]
    rows = asr.unit_rows(acts["conv3"])[4].astype(np.float64)
    fin = rows[np.isfinite(rows)]
    assert fin.size == n * 49 - 2
    np.testing.assert_allclose(u[asr.MEAN_ABS], np.abs(fin).sum() / (n * 49), rtol=1e-14)  # K keeps the left-out positions
    assert u[asr.MAX_ABS] == np.abs(fin).max() and u[asr.POSITIVE_FRACTION] == (fin > 0).sum() / (n * 49)
    assert np.isfinite(units).all() and np.isfinite(layers).all()
    f = units[first[3] + 6]
    assert f[asr.MEAN_ABS] == 0.25 and f[asr.POSITIVE_FRACTION] == 1 / 3 and f[asr.MAX_ABS] == 0.5  # exact
    # scores: mean 1 over a layer; the layer rows and the total row add up
    for l in range(4):
        sc = units[first[l]:first[l + 1], asr.SCORE]
        np.testing.assert_allclose(sc.mean(), 1.0, rtol=1e-13)
        assert layers[l, asr.L_UNITS] == first[l + 1] - first[l]
        assert layers[l, asr.L_ELEMENTS] == layers[l, asr.L_UNITS] * n * asr.PIX[asr.LAYERS[l]]
        assert layers[l, asr.L_MAX_ABS] == units[first[l]:first[l + 1], asr.MAX_ABS].max()
        np.testing.assert_allclose(layers[l, asr.L_MEAN_ABS], units[first[l]:first[l + 1], asr.MEAN_ABS].mean(), rtol=1e-13)
    for col in (asr.L_UNITS, asr.L_ELEMENTS, asr.L_DEAD, asr.L_DORMANT, asr.L_NONFINITE):
        assert layers[4, col] == layers[:4, col].sum()
    assert layers[4, asr.L_UNITS] == 160 + H and layers[4, asr.L_MAX_ABS] == layers[:4, asr.L_MAX_ABS].max()
    np.testing.assert_allclose(layers[4, asr.L_MEAN_ABS],
                               (layers[:4, asr.L_MEAN_ABS] * layers[:4, asr.L_ELEMENTS]).sum() / layers[4, asr.L_ELEMENTS],
                               rtol=1e-13)
    np.testing.assert_allclose(layers[4, asr.L_POSITIVE_FRACTION],
                               (layers[:4, asr.L_POSITIVE_FRACTION] * layers[:4, asr.L_ELEMENTS]).sum() /
                               layers[4, asr.L_ELEMENTS], rtol=1e-13)
    # tau = 0: exactly the units whose every finite element is zero
    assert asr.reference(acts, 0.0)["layers"][1, asr.L_DORMANT] == 1
    # an all-zero layer: the layer mean is 0, every score is 0, every unit dead and dormant
    zero = dict(acts, conv1=np.zeros_like(acts["conv1"]))
    rz = asr.reference(zero, TAU)
    assert (rz["units"][:32] == 0).all() and rz["layers"][0, asr.L_DEAD] == 32 == rz["layers"][0, asr.L_DORMANT]


def test_the_checker_rejects_what_it_has_to():
    acts = _hand_made()
    ref = asr.reference(acts, TAU)
    units, layers = ref["units"], ref["layers"]
    assert not asr.check(units, layers, ref)
    # the derived bounds: 2 K 2^-53 on a unit's mean, (4 K + 2 units) 2^-53 on its score, equal everywhere else
    assert ref["unit_rtol"][0, asr.MEAN_ABS] == 2 * 3 * 400 * 2.0 ** -53
    assert ref["unit_rtol"][40, asr.SCORE] == (4 * 3 * 81 + 2 * 64) * 2.0 ** -53
    assert not ref["unit_rtol"][:, [asr.POSITIVE_FRACTION, asr.MAX_ABS, asr.NONFINITE]].any()
    assert np.count_nonzero(ref["layer_rtol"]) == 5  # MEAN_ABS of the five rows
    d = units.copy()
    d[50, asr.NONFINITE] += 1  # a count off by one
    assert [f[:2] for f in asr.check(d, layers, ref)] == [("conv2[18]", "nonfinite")]
    d = units.copy()
    d[170, asr.POSITIVE_FRACTION] += 1 / 3  # one sample more
    assert [f[:2] for f in asr.check(d, layers, ref)] == [("fc[10]", "positive_fraction")]
    d = units.copy()
    d[7, asr.MEAN_ABS] *= 1 + 1e-9
    assert [f[:2] for f in asr.check(d, layers, ref)] == [("conv1[7]", "mean_abs")]
    d = units.copy()
    d[[100, 101]] = d[[101, 100]]  # two channels swapped
    bad = asr.check(d, layers, ref)
    assert {f[0] for f in bad} == {"conv3[4]", "conv3[5]"} and len(bad) >= 6
    d = layers.copy()
    d[2, asr.L_DEAD] += 1
    assert [f[:2] for f in asr.check(units, d, ref)] == [("conv3", "dead")]
    d = layers.copy()
    d[4, asr.L_MEAN_ABS] *= 1 + 1e-9
    assert [f[:2] for f in asr.check(units, d, ref)] == [("total", "mean_abs")]
    d = layers.copy()
    d[3, asr.L_DORMANT] += 1
    assert [f[:2] for f in asr.check(units, d, ref)] == [("fc", "dormant")]
    # a summation order changes a mean by far less than the bound: float64 pairwise sums pass
    d = units.copy()
    d[:32, asr.MEAN_ABS] = np.abs(asr.unit_rows(acts["conv1"]).astype(np.float64)).sum(axis=1) / (3 * 400)
    assert not asr.check(d, layers, ref)


# ------------------------------------------------------------------ CPU: the fixture on the emulating oracle
@pytest.mark.parametrize("case", ["h32", "h96", "n260"])
def test_fixture_has_one_dead_and_one_dormant_unit_by_design(case):
    _, H, A, n, _ = CASES[case]
    for mode in ("bf16", "fp32"):
        ref = asr.reference(_oracle_acts(case, mode, True), TAU)
        assert not asr.fixture_facts(ref["units"], ref["layers"], H), (mode, asr.fixture_facts(ref["units"], ref["layers"], H))
        fc = ref["units"][160:, asr.SCORE]
        print(f"{case} {mode}: fc[3] score {fc[3]:.3g}, the others {np.delete(fc, 3).min():.3g} .. {np.delete(fc, 3).max():.3g}; "
              f"dead {ref['layers'][:4, asr.L_DEAD]}, dormant {ref['layers'][:4, asr.L_DORMANT]}")
    assert (_oracle_acts(case, "bf16", True)["conv2"][:, 5] == 0).all()
    assert not asr.check(ref["units"], ref["layers"], ref)


@pytest.mark.parametrize("case", ["h32", "h96", "n260"])
def test_the_export_bound_rejects_the_fp32_oracle_on_every_layer(case):
    """bf16_check's rule, max(base, 4 x floor), applied per layer to the export: the floor run (the emulation with fp32
    sums) is far inside it, the plain fp32 oracle outside it on every layer - a bf16 engine has to round where the
    emulation rounds to pass"""
    bounds, floor = _export_bounds(case)
    plain = _export_errors(_oracle_acts(case, "fp32"), _oracle_acts(case, "bf16"))
    for l in asr.LAYERS:
        print(f"{case} {l}: floor {floor[l][0]:.3g} / {floor[l][1]:.3g}, fp32 oracle {plain[l][0]:.3g} / {plain[l][1]:.3g}, "
              f"bounds {bounds[l][0]:.3g} / {bounds[l][1]:.3g}")
        assert floor[l][0] <= bounds[l][0] / bc.FLOOR_FACTOR and floor[l][1] <= bounds[l][1] / bc.FLOOR_FACTOR
        assert plain[l][0] > bounds[l][0], l


# ------------------------------------------------------------------ CPU: the trainer's keys on the stand-in
TAGS = [f"activation_stats/{l}/{s}".encode() for l in asr.ROWS
        for s in ("dormant_fraction", "dead_fraction", "positive_fraction", "mean_abs")] + [b"activation_stats/nonfinite"]


def _scalar_bits(blob):
    """{tag: [binary32 bit pattern, ...]} of every simple_value scalar of an event file, in file order"""
    out = {}
    for m in re.finditer(rb"\x0a([\x01-\x40])([A-Za-z_/.0-9]+)\x15", blob):
        if m.group(1)[0] == len(m.group(2)):
            out.setdefault(m.group(2), []).append(struct.unpack("<I", blob[m.end():m.end() + 4])[0])
    return out


def _run_trainer(binary, d, extra, rollouts=4):
    os.makedirs(d / "tb")
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def astats_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_astats_stub"])
    return os.path.join(ROOT, "trainer", "train_astats_stub")


def _calls(r):
    m = re.search(r"stub: aleppo_activation_stats calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    return int(m.group(1))


def test_trainer_keys_with_the_stub_library(astats_trainer, tmp_path):
    runs = (("absent", "", 0, 0), ("false", "log_activation_stats: false\n", 0, 0),
            ("true", "log_activation_stats: true\n", 4, 0),
            ("every2", "log_activation_stats: true\nactivation_stats_interval: 2\ndormant_tau: 0.1\n", 2, 1 / 32))
    tags, blobs = {}, {}
    for name, extra, calls, _ in runs:
        (tmp_path / name).mkdir()
        r = _run_trainer(astats_trainer, tmp_path / name, extra)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        assert _calls(r) == calls, name  # the key off: the stand-in is never called
        blobs[name] = trainer_helpers.events(tmp_path / name / "tb")
        tags[name] = _scalar_bits(blobs[name])
    assert set(tags["absent"]) == set(tags["false"]) and b"mean_loss" in tags["absent"]
    assert not set(TAGS) & set(tags["absent"]) and len(TAGS) == 21
    f = lambda bits: struct.unpack("<f", struct.pack("<I", bits))[0]
    for name, _, calls, conv1_dormant in runs[2:]:
        assert set(tags[name]) == set(tags["absent"]) | set(TAGS)  # nothing else appears or goes
        for tag in TAGS:
            assert len(tags[name][tag]) == calls and len(tags[name][b"mean_loss"]) == 4, tag
        for tag in tags["absent"]:  # (the stand-in is deterministic: the rest of the event file does not move)
            assert tags["absent"][tag] == tags[name][tag], tag
        # the stand-in's scores are 2 (i + 1) / (C + 1): 0 of conv1's 32 are <= 0.025, 1 is <= 0.1; its DEAD is the row index
        assert [f(b) for b in tags[name][b"activation_stats/conv1/dormant_fraction"]] == [np.float32(conv1_dormant)] * calls
        assert f(tags[name][b"activation_stats/conv3/dead_fraction"][0]) == np.float32(2 / 64)
        assert f(tags[name][b"activation_stats/fc/positive_fraction"][0]) == 0.5
        assert f(tags[name][b"activation_stats/conv2/mean_abs"][0]) == np.float32(0.5)
        assert [f(b) for b in tags[name][b"activation_stats/nonfinite"]] == [0.0] * calls
        assert b"log_activation_stats" in blobs[name]  # the hparams flag of the config dump, only when set
    assert b"log_activation_stats" not in blobs["absent"] and b"log_activation_stats" not in blobs["false"]


@pytest.mark.parametrize("extra,message", [
    ("log_activation_stats: true\ndormant_tau: -0.1\n", "dormant_tau must be finite and non-negative"),
    ("log_activation_stats: true\ndormant_tau: sometimes\n", "bad value for dormant_tau"),
    ("log_activation_stats: true\ndormant_tau: nan\n", "dormant_tau"),
    ("log_activation_stats: true\nactivation_stats_interval: 0\n", "activation_stats_interval must be positive"),
    ("dormant_tau: 0.1\n", "dormant_tau needs log_activation_stats: true"),
])
def test_trainer_refuses_bad_keys(astats_trainer, tmp_path, extra, message):
    r = _run_trainer(astats_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _calls(r) == 0


def test_library_without_the_symbol_refuses_the_key(tmp_path_factory, tmp_path):
    plain = trainer_helpers.build_stub_trainer(tmp_path_factory)  # (the stand-in without aleppo_activation_stats)
    r = _run_trainer(plain, tmp_path, "log_activation_stats: true\n", 2)
    assert r.returncode == 1 and "aleppo_activation_stats is missing" in r.stderr and "Rollout" not in r.stdout, r.stderr
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0


# ------------------------------------------------------------------ GPU
def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


def _engine(pkg, case, prec, modified=False, params=None):
    _, H, A, n, _ = CASES[case]
    eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec), max_minibatch=max(n, 64))
    eng.load_params(_params(case, modified) if params is None else params)
    return eng


def _bits(a, dt=np.uint32):
    return np.ascontiguousarray(a).view(dt)


def _same_export(a, b):
    return all(np.array_equal(_bits(a[l]), _bits(b[l])) for l in a)


def _raw_call(pkg, eng, obs, n, tau=TAU, H=None, unit_count=None, layer_count=40, null_units=False, null_layers=False):
    """the C entry point itself: (status, units, layers), the outputs pre-filled with -7 so that "nothing is written" shows"""
    H = eng.H if H is None else H
    units, layers = np.full((160 + H, 5), -7.0), np.full((5, 8), -7.0)
    rc = pkg.lib().aleppo_activation_stats(
        eng._ctx, None if obs is None else obs.ctypes.data_as(C.c_void_p), C.c_int64(n), C.c_double(tau),
        None if null_units else units.ctypes.data_as(C.c_void_p), C.c_size_t(units.size if unit_count is None else unit_count),
        None if null_layers else layers.ctypes.data_as(C.c_void_p), C.c_size_t(layer_count))
    return rc, units, layers


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["h32", "h96"])
def test_export_fp32_against_the_oracle(pkg, case):
    """every layer within |d| <= 1e-4 (1 + |ref|) of oracle_lib.net_forward(want_acts=True): this pins the channel order and
    the NHWC -> NCHW conversion; a subset of layers exports the same bits"""
    _, H, A, n, oseed = CASES[case]
    eng = _engine(pkg, case, "fp32")
    got = eng.forward_activations(_obs(oseed, n))
    ref = _oracle_acts(case, "fp32")
    for l in asr.LAYERS:
        assert got[l].shape == ref[l].shape and got[l].dtype == np.float32
        excess = np.abs(got[l].astype(np.float64) - ref[l]) / (1 + np.abs(ref[l]))
        print(f"export fp32 {case} {l}: max |d| / (1 + |ref|) = {excess.max():.3g}")
        assert excess.max() <= 1e-4, l
    for l in ("conv1", "conv2", "conv3"):
        assert got[l].min() >= 0  # after the ReLU
    assert got["fc"].min() < 0 < got["fc"].max()  # no ReLU: signed
    part = eng.forward_activations(_obs(oseed, n), layers=("conv2", "fc"))
    assert set(part) == {"conv2", "fc"} and _same_export(part, {l: got[l] for l in part})
    logits, values = eng.forward(_obs(oseed, n))  # the export leaves aleppo_forward's answer where it was
    np.testing.assert_allclose(logits, orc.net_forward(_params(case), H, A, _obs(oseed, n))[0], atol=1e-4)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["h32", "h96", "n260", "n1"])
def test_export_bf16_against_the_emulation_on_every_route(pkg, case):
    """the default route (fused forward), three launches (OPT_FUSED_FWD = 0) and the generic convolutions
    (OPT_GENERIC_CONV = 1) against the bf16-emulating oracle by bf16_check's rule; fused forward and three launches export
    identical bits (the identity the project claims), and the conv activations are bf16 values"""
    _, H, A, n, oseed = CASES[case]
    obs = _obs(oseed, n)
    ref = _oracle_acts(case, "bf16")
    bounds, _ = _export_bounds(case)
    eng = _engine(pkg, case, "bf16")
    routes = {}
    for name, opt, val in (("fused", None, None), ("three launches", pkg.OPT_FUSED_FWD, 0),
                           ("generic", pkg.OPT_GENERIC_CONV, 1)):
        if opt is not None:
            eng.set_option(opt, val)
        got = routes[name] = eng.forward_activations(obs)
        err = _export_errors(got, ref)
        print(f"export bf16 {case} {name}:", {l: "%.3g/%.3g %.3g/%.3g" % (err[l][0], bounds[l][0], err[l][1], bounds[l][1])
                                             for l in asr.LAYERS})
        for l in asr.LAYERS:
            assert err[l][0] <= bounds[l][0] and err[l][1] <= bounds[l][1], (name, l, err[l], bounds[l])
        for l in ("conv1", "conv2", "conv3"):
            assert not (_bits(got[l]) & 0xFFFF).any() and got[l].min() >= 0, l  # bf16 values widened exactly
    assert _same_export(routes["fused"], routes["three launches"])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["h32", "h96", "n260", "n1"])
def test_statistics_against_the_engines_own_export(pkg, prec, case):
    """activation_stats(obs) against the float64 reference on forward_activations(obs) of the modified fixture, at the
    derived bounds; the fixture's three facts hold on the device"""
    _, H, A, n, oseed = CASES[case]
    obs = _obs(oseed, n)
    eng = _engine(pkg, case, prec, modified=True)
    ref = asr.reference(eng.forward_activations(obs), TAU)
    units, layers = eng.activation_stats(obs, tau=TAU, raw=True)
    print(f"activation stats {prec} {case}: worst |device - reference| / bound",
          {k: "%.3g" % v for k, v in asr.worst(units, layers, ref).items()}, "dead", layers[:, asr.L_DEAD], "dormant",
          layers[:, asr.L_DORMANT])
    assert not asr.check(units, layers, ref), asr.check(units, layers, ref)[:6]
    assert layers[4, asr.L_ELEMENTS] == n * (12800 + 5184 + 3136 + H) and not layers[:, asr.L_NONFINITE].any()
    if n > 1:
        assert not asr.fixture_facts(units, layers, H), asr.fixture_facts(units, layers, H)
    else:
        assert (units[32 + 5] == 0).all()  # conv2 channel 5 is dead on any sample
    # the dictionary form, and tau reaches the kernel: at tau = 0 dormant is dead, at a large tau every unit
    d = eng.activation_stats(obs, tau=0.0)
    assert set(d) == {"units", "layers"} and set(d["units"]) == set(asr.LAYERS) and set(d["layers"]) == set(asr.ROWS)
    assert d["units"]["fc"]["score"].shape == (H,) and set(d["layers"]["total"]) == set(pkg.ACT_LAYER_STATS)
    assert np.array_equal(d["units"]["conv2"]["mean_abs"], units[32:96, asr.MEAN_ABS])
    for l in asr.ROWS:
        assert d["layers"][l]["dormant"] == d["layers"][l]["dead"]
    assert eng.activation_stats(obs, tau=1e9)["layers"]["total"]["dormant"] == 160 + H
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_infinite_bias_is_counted_and_left_out(pkg, prec):
    """+Inf in conv3.b[7]: unit (conv3, 7) has NONFINITE == n * 49 and zero mean and maximum, and every number still equals
    the reference on the export (fc, downstream of it, is non-finite too)"""
    case = "h32"
    _, H, A, n, oseed = CASES[case]
    params = np.array(_params(case, True))
    params[int(ar.param_offsets(H, A)[5]) + 7] = np.inf
    eng = _engine(pkg, case, prec, params=params)
    acts = eng.forward_activations(_obs(oseed, n))
    assert np.isposinf(acts["conv3"][:, 7]).all()
    ref = asr.reference(acts, TAU)
    units, layers = eng.activation_stats(_obs(oseed, n), tau=TAU, raw=True)
    assert not asr.check(units, layers, ref), asr.check(units, layers, ref)[:6]
    u = units[96 + 7]
    assert u[asr.NONFINITE] == n * 49 and u[asr.MEAN_ABS] == 0 and u[asr.MAX_ABS] == 0 and u[asr.SCORE] == 0
    assert layers[2, asr.L_NONFINITE] == n * 49 and layers[3, asr.L_NONFINITE] > 0
    assert layers[4, asr.L_NONFINITE] == layers[:4, asr.L_NONFINITE].sum() and np.isfinite(units).all()
    eng.close()


@functools.lru_cache(maxsize=None)
def _batch_planes(seed, n, A):
    """the planes aleppo_set_batch wants next to the observations: (actions, old log-probs, advantages, returns, masks)"""
    return ((hf.hf_u32(seed + 2, n) % np.uint32(A)).astype(np.int64), orc.log_softmax(hf.hf_range(seed + 3, (n, A), -1, 1)),
            hf.hf_range(seed + 4, (n,), -1, 1), hf.hf_range(seed + 5, (n,), -1, 1),
            (hf.hf_unit(seed + 6, n) >= np.float32(0.1)).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sources_and_chunking(pkg, prec):
    """E = 8, T = 65, max_minibatch = 260: a caller batch of 260 samples is one forward chunk, and the batch source equals
    the caller source bit for bit; one of 520 is two chunks, against the reference on the two exports concatenated (masked
    samples included); two calls in a row are bit-identical"""
    H, A = 32, 4
    eng = pkg.Engine(8, 65, A, H, precision=_prec(pkg, prec), max_minibatch=260)
    eng.load_params(_params("n260", True))
    with pytest.raises(pkg.AleppoError, match="no batch"):
        eng.activation_stats()
    o1, o2 = _obs(9350, 260), _obs(9360, 260)
    eng.set_batch(o1, *_batch_planes(9400, 260, A))
    bu, bl = eng.activation_stats(tau=TAU, raw=True)
    cu, cl = eng.activation_stats(o1, tau=TAU, raw=True)
    assert np.array_equal(_bits(bu, np.uint64), _bits(cu, np.uint64)) and np.array_equal(_bits(bl, np.uint64), _bits(cl, np.uint64))
    both = np.concatenate([o1, o2])
    eng.set_batch(both, *_batch_planes(9410, 520, A))
    units, layers = eng.activation_stats(tau=TAU, raw=True)
    again = eng.activation_stats(tau=TAU, raw=True)
    assert np.array_equal(_bits(units, np.uint64), _bits(again[0], np.uint64))
    assert np.array_equal(_bits(layers, np.uint64), _bits(again[1], np.uint64))
    ref = asr.reference(asr.concat([eng.forward_activations(o1), eng.forward_activations(o2)]), TAU)
    print(f"chunked batch {prec}: worst / bound", {k: "%.3g" % v for k, v in asr.worst(units, layers, ref).items()})
    assert not asr.check(units, layers, ref), asr.check(units, layers, ref)[:6]
    assert layers[0, asr.L_ELEMENTS] == 32 * 520 * 400 and not asr.fixture_facts(units, layers, H)
    with pytest.raises(pkg.AleppoInvalidArgument, match="capacity"):
        eng.activation_stats(both)  # the caller source takes one forward chunk at the most
    eng.close()


def _rollout(eng, seed, E, T, probe=None):
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
def test_a_rollout_batch_is_read_in_place(pkg, prec):
    """E = 4, T = 8 through the rollout protocol: the batch source against the caller source on read_batch("observations")
    (32 samples: one chunk, so bit for bit) and against the reference on their export"""
    E, T, A, H = 4, 8, 4, 32
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec), seed=5)
    eng.load_params(_params("h32", True))
    _rollout(eng, 9500, E, T)
    obs = eng.read_batch("observations").reshape(E * T, 4, 84, 84)
    # (every environment starts from the empty stack; all later stacks differ: an order mistake would show)
    assert len({o.tobytes() for o in obs}) == E * (T - 1) + 1 and not obs[::T].any()
    bu, bl = eng.activation_stats(tau=TAU, raw=True)
    cu, cl = eng.activation_stats(obs, tau=TAU, raw=True)
    assert np.array_equal(_bits(bu, np.uint64), _bits(cu, np.uint64)) and np.array_equal(_bits(bl, np.uint64), _bits(cl, np.uint64))
    ref = asr.reference(eng.forward_activations(obs), TAU)
    assert not asr.check(bu, bl, ref), asr.check(bu, bl, ref)[:6]
    eng.close()


def _twin(pkg, prec, graph, probes):
    E, T, A, H = 8, 8, 6, 64
    eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec), seed=3)
    eng.load_params(hf.fill_params(9600, H, A))
    if graph:
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    seen, have_batch = [], []

    def probe():
        if not probes:
            return
        obs = _obs(9650, 5)
        assert eng.forward_activations(obs)["fc"].shape == (5, H)
        seen.append(eng.activation_stats(obs, raw=True)[1][4, asr.L_ELEMENTS])
        if have_batch:  # the batch source, once a batch exists (in the middle of a rollout: the previous rollout's)
            seen.append(eng.activation_stats(raw=True)[1][4, asr.L_ELEMENTS])

    out = dict(acts=[], metrics=[], digests=[], replays=[])
    for r in range(2):
        out["acts"] += _rollout(eng, 9700 + 1000 * r, E, T, probe)
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
    """twins from the same seed run rollout -> update -> rollout -> update; one calls both entry points after a mid-rollout
    step (the next aleppo_act recomputes what the step had pre-computed), after finish_rollout and after train.  Sampled
    actions, update metrics, the state digest, parameters, both moments and the graph-launch count are bit-identical"""
    plain, mixed = _twin(pkg, prec, graph, False), _twin(pkg, prec, graph, True)
    assert len(mixed["seen"]) >= 8 and set(mixed["seen"]) == {5 * (21120 + 64), 64 * (21120 + 64)}
    np.testing.assert_array_equal(np.stack(plain["acts"]), np.stack(mixed["acts"]))
    for r in range(2):
        assert np.array_equal(_bits(plain["metrics"][r]), _bits(mixed["metrics"][r])), r
        assert plain["digests"][r] == mixed["digests"][r], r
    assert plain["replays"] == mixed["replays"] == ([0, 1] if graph else [0, 0])
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(_bits(plain["state"][k]), _bits(mixed["state"][k])), k
    assert plain["state"]["step"] == mixed["state"]["step"] == 8


@pytest.mark.gpu
def test_errors(pkg):
    """tau negative or not finite, a null output, wrong counts, n out of range, null observations with n != 0:
    ALEPPO_ERR_INVALID_ARGUMENT; the batch source without a batch and any call while a step is armed: ALEPPO_ERR_RUNTIME;
    a failed call writes nothing, and after the release both calls succeed"""
    E, T, H, A = 8, 8, 32, 4
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32)
    eng.load_params(_params("h32"))
    obs = np.ascontiguousarray(_obs(9150, 37))
    bad = [dict(tau=-1e-9), dict(tau=float("nan")), dict(tau=float("inf")), dict(null_units=True), dict(null_layers=True),
           dict(unit_count=(160 + H) * 5 - 1), dict(unit_count=160 + H), dict(layer_count=39), dict(layer_count=45)]
    for kw in bad:
        rc, units, layers = _raw_call(pkg, eng, obs, 37, **kw)
        assert rc == pkg.ERR_INVALID_ARGUMENT and (units == -7).all() and (layers == -7).all(), kw
    for o, n in ((obs, 0), (obs, -1), (obs, 65), (None, 1), (None, 37)):  # maxB = E * T = 64
        rc, units, layers = _raw_call(pkg, eng, o, n)
        assert rc == pkg.ERR_INVALID_ARGUMENT and (units == -7).all() and (layers == -7).all(), n
    rc, units, layers = _raw_call(pkg, eng, None, 0)
    assert rc == pkg.ERR_RUNTIME and (units == -7).all() and (layers == -7).all()  # no batch yet
    assert _raw_call(pkg, eng, obs, 37)[0] == pkg.OK and _raw_call(pkg, eng, obs, 37, tau=0.0)[0] == pkg.OK
    with pytest.raises(pkg.AleppoInvalidArgument, match="tau"):
        eng.activation_stats(obs, tau=-1)
    with pytest.raises(pkg.AleppoInvalidArgument, match="layers"):
        eng.forward_activations(obs, layers=("conv4",))
    with pytest.raises(pkg.AleppoInvalidArgument, match="layers"):
        eng.forward_activations(obs, layers=())
    with pytest.raises(pkg.AleppoInvalidArgument, match="capacity"):
        eng.forward_activations(_obs(9170, 65))
    lib = pkg.lib()
    fc = np.full((37, H), -7.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.aleppo_forward_activations(eng._ctx, ptr(obs), C.c_int64(37), None, None, None, None) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_forward_activations(eng._ctx, None, C.c_int64(37), None, None, None, ptr(fc)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_forward_activations(eng._ctx, ptr(obs), C.c_int64(0), None, None, None, ptr(fc)) == pkg.ERR_INVALID_ARGUMENT
    assert (fc == -7).all()
    # while a step is armed
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(9180, (E * 7056,)), np.ones(E, np.uint8)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    rc, units, layers = _raw_call(pkg, eng, obs, 37)
    assert rc == pkg.ERR_RUNTIME and (units == -7).all() and (layers == -7).all()
    assert lib.aleppo_forward_activations(eng._ctx, ptr(obs), C.c_int64(37), None, None, None, ptr(fc)) == pkg.ERR_RUNTIME
    assert (fc == -7).all()
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    ref = asr.reference(eng.forward_activations(obs), TAU)
    rc, units, layers = _raw_call(pkg, eng, obs, 37)
    assert rc == pkg.OK and not asr.check(units, layers, ref)
    eng.synchronize()
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
