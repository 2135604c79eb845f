"""aleppo_recycle_units / aleppo_recycle_dormant: ReDo's re-initialisation and reset of masked units, on the device.

CPU (not marked gpu): the header's constants and prototypes against the Python mirror, the null-context refusal, hand-written
known answers of the numpy reference (tests/recycle_ref.py), the distribution of the re-initialised values, and the
fixture (conv2[5] dead, fc[3] dormant) through the oracle: the recycled conv2[5] fires again, and recycling a dead unit
leaves every output alone.
GPU: the state after a recycle against the reference bit for bit, the derived copies against a twin that was given the
reference's state, recycle_dormant against a twin that forms the mask on the host, isolation, the errors."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import activation_stats_ref as asr
import adam_ref as ar
import hashfill as hf
import oracle_lib as orc
import recycle_ref as rr
from conftest import ROOT
import trainer_helpers
from shared_fixtures import pkg  # noqa: F401
from __graft_entry__ import load_package

TAU = 0.025
KEY = 12345  # the key of the fixture's recycle, on the CPU and on the GPU
SHAPES = {"h32": (9100, 32, 4), "h96": (9200, 96, 18)}  # name: (parameter seed, H, A)
N_OBS, OBS_SEED = 37, 9150
N_BATCH, BATCH_SEED = 64, 9400


@functools.lru_cache(maxsize=None)
def _obs(seed, n):
    a = hf.hf_bytes(seed, (n, 4, 84, 84))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _params(shape, modified=False):
    seed, H, A = SHAPES[shape]
    p = hf.fill_params(seed, H, A)
    if modified:
        p = asr.modified_params(p, H, A)
    p.setflags(write=False)
    return p


def _unit_mask(H, **units):
    """a mask with the named units set: _unit_mask(32, conv2=[5], fc=[3])"""
    m = np.zeros(160 + H, np.uint8)
    first = rr.first_units(H)
    for layer, idx in units.items():
        m[np.asarray(idx) + first[rr.LAYERS.index(layer)]] = 1
    return m


def _bits(a, dt=np.uint32):
    return np.ascontiguousarray(a).view(dt)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a, np.uint8), _bits(b, np.uint8))


# ------------------------------------------------------------------ CPU: constants and prototypes
def test_header_constants_and_prototypes_match_the_python_mirror():
    pkg = load_package()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)

    const = functools.partial(trainer_helpers.header_const, stripped=True)

    assert const("ALEPPO_RECYCLE_COUNTS") == pkg.RECYCLE_COUNTS == len(rr.ROWS) == 5
    for name in ("conv1", "conv2", "conv3", "fc"):
        assert const("ALEPPO_RECYCLE_" + name.upper()) == pkg.RECYCLE_LAYERS[name] == rr.LAYER_BITS[name]
    assert const("ALEPPO_RECYCLE_ALL") == pkg.RECYCLE_ALL == pkg.RECYCLE_LAYERS["all"] == 15
    assert (pkg.RECYCLE_CONV1, pkg.RECYCLE_CONV2, pkg.RECYCLE_CONV3, pkg.RECYCLE_FC) == (1, 2, 4, 8)
    assert const("ALEPPO_RECYCLE_KEEP_MOMENTS") == pkg.RECYCLE_KEEP_MOMENTS == 1
    assert const("ALEPPO_K_RECYCLE") == pkg.KERNEL_CLASSES["recycle"] == 22
    for name in ("aleppo_recycle_units", "aleppo_recycle_dormant"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert hasattr(pkg.Engine, "recycle_units") and hasattr(pkg.Engine, "recycle_dormant")
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int aleppo_recycle_units(aleppo_ctx *ctx, const uint8_t *mask, size_t unit_count, uint64_t key, int flags, "
            "int64_t counts[ALEPPO_RECYCLE_COUNTS]);") in flat
    assert ("int aleppo_recycle_dormant(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, double tau, int layers, "
            "uint64_t key, int flags, uint8_t *mask_out, size_t unit_count, int64_t counts[ALEPPO_RECYCLE_COUNTS]);") in flat
    assert re.search(r"(?m)^#define ALEPPO_ABI_VERSION 2$", hdr) and pkg.ABI_VERSION == 2


def test_a_null_context_is_refused_before_any_device_work():
    pkg = load_package()
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    mask, counts = np.full(192, 7, np.uint8), np.full(5, -7, np.int64)
    rc = lib.aleppo_recycle_units(None, ptr(np.zeros(192, np.uint8)), C.c_size_t(192), C.c_uint64(1), C.c_int(0), ptr(counts))
    assert rc == pkg.ERR_INVALID_ARGUMENT and (counts == -7).all()
    obs = np.zeros((1, 4, 84, 84), np.uint8)
    rc = lib.aleppo_recycle_dormant(None, ptr(obs), C.c_int64(1), C.c_double(TAU), C.c_int(15), C.c_uint64(1), C.c_int(0),
                                    ptr(mask), C.c_size_t(192), ptr(counts))
    assert rc == pkg.ERR_INVALID_ARGUMENT and (counts == -7).all() and (mask == 7).all()


# ------------------------------------------------------------------ CPU: the reference's known answers
@pytest.fixture(scope="module")
def mirror():
    """the reference speaks the package's language: the layer bits, the rows of the counts, the flag"""
    pkg = load_package()
    assert {l: pkg.RECYCLE_LAYERS[l] for l in rr.LAYERS} == rr.LAYER_BITS and pkg.RECYCLE_LAYERS["all"] == sum(rr.LAYER_BITS.values())
    assert tuple(pkg.ACT_LAYER_ROWS) == rr.ROWS and pkg.RECYCLE_COUNTS == len(rr.ROWS) and pkg.RECYCLE_KEEP_MOMENTS == 1
    return pkg


def _hand_state(H=32, A=4):
    n = int(ar.param_offsets(H, A)[-1])
    return hf.hf_range(8801, (n,), -1, 1), hf.hf_range(8802, (n,), -1, 1), hf.hf_range(8803, (n,), 0.5, 1)


def _expected_value(key, i, fan_in):
    """the header's formula on Python integers"""
    r = rr.splitmix64(rr.splitmix64(int(key)) ^ int(i))
    k = (r >> 40) - 8388608
    return np.float32(np.sqrt(6.0 / fan_in)) * (np.float32(k) * np.float32(2.0 ** -23))


def test_known_answer_a_single_conv2_unit(mirror):
    H, A = 32, 4
    offs = [int(o) for o in ar.param_offsets(H, A)]
    p0, m0, v0 = _hand_state()
    assert (p0 != 0).all() and (m0 != 0).all() and (v0 != 0).all()
    mask = _unit_mask(H, conv2=[7])
    assert rr.counts(mask, H) == dict(conv1=0, conv2=1, conv3=0, fc=0, total=1)
    p, m, v = rr.apply(p0, m0, v0, mask, 11, H, A)
    changed = np.zeros(p.size, bool)
    row = slice(offs[2] + 7 * 512, offs[2] + 8 * 512)  # conv2.w[7]: re-initialised
    changed[row] = True
    for i in (row.start, row.start + 100, row.stop - 1):
        assert p[i] == _expected_value(11, i, 512) and abs(p[i]) <= np.float32(np.sqrt(6 / 512))
    assert len(np.unique(p[row])) > 500
    changed[offs[3] + 7] = True  # conv2.b[7]: zero
    assert p[offs[3] + 7] == 0
    w3 = np.arange(offs[4], offs[5]).reshape(64, 64, 3, 3)[:, 7]  # conv3.w[:, 7]: zero
    changed[w3.reshape(-1)] = True
    assert (p[w3] == 0).all() and w3.size == 576
    assert np.array_equal(p != p0, changed) and _same(p[~changed], p0[~changed])
    assert (m[changed] == 0).all() and (v[changed] == 0).all() and not np.signbit(m[changed]).any()
    assert _same(m[~changed], m0[~changed]) and _same(v[~changed], v0[~changed])
    assert changed.sum() == 512 + 1 + 576
    pk, mk, vk = rr.apply(p0, m0, v0, mask, 11, H, A, keep_moments=True)
    assert _same(pk, p) and _same(mk, m0) and _same(vk, v0)
    # an all-zero mask changes nothing; an fc unit zeroes its column of both heads and leaves the head biases
    pz, mz, vz = rr.apply(p0, m0, v0, np.zeros(160 + H, np.uint8), 11, H, A)
    assert _same(pz, p0) and _same(mz, m0) and _same(vz, v0)
    pf = rr.apply(p0, m0, v0, _unit_mask(H, fc=[3]), 11, H, A)[0]
    aw = np.arange(offs[8], offs[9]).reshape(A, H)
    assert (pf[aw[:, 3]] == 0).all() and pf[offs[10] + 3] == 0 and pf[offs[7] + 3] == 0
    assert _same(pf[offs[9]:offs[10]], p0[offs[9]:offs[10]]) and pf[offs[11]] == p0[offs[11]]
    fcw = np.arange(offs[6], offs[7]).reshape(H, 3136)
    assert all(pf[i] == _expected_value(11, i, 3136) for i in fcw[3, ::500])
    assert (pf != p0).sum() == 3136 + 1 + A + 1


def test_known_answer_zero_wins_over_a_conv1_conv2_pair(mirror):
    H, A = 32, 4
    offs = [int(o) for o in ar.param_offsets(H, A)]
    p0, m0, v0 = _hand_state()
    p, m, v = rr.apply(p0, m0, v0, _unit_mask(H, conv1=[2], conv2=[7]), 12, H, A)
    w1 = np.arange(offs[0], offs[1]).reshape(32, 256)
    assert all(p[i] == _expected_value(12, i, 256) for i in w1[2]) and p[offs[1] + 2] == 0
    w2 = np.arange(offs[2], offs[3]).reshape(64, 32, 16)
    assert (p[w2[:, 2]] == 0).all()  # the outgoing weights of conv1[2] - also those inside the re-initialised conv2.w[7]
    assert (p[w2[7, 2]] == 0).all() and (m[w2[7, 2]] == 0).all() and (v[w2[7, 2]] == 0).all()
    rest = np.delete(w2[7], 2, axis=0).reshape(-1)
    assert all(p[i] == _expected_value(12, i, 512) for i in rest) and (p[rest] != 0).all()
    w3 = np.arange(offs[4], offs[5]).reshape(64, 64, 9)
    assert (p[w3[:, 7]] == 0).all()
    assert (p != p0).sum() == 256 + 1 + 64 * 16 + (512 - 16) + 1 + 576
    sel = p != p0
    assert (m[sel] == 0).all() and _same(m[~sel], m0[~sel]) and _same(v[~sel], v0[~sel])


# ------------------------------------------------------------------ CPU: the re-initialised values
def test_reinitialised_values_are_he_uniform(mirror):
    """every value in [-a_l, a_l); over all of fc.w (all of fc masked, nothing of conv3) the mean is 0 and the variance
    a_l^2 / 3 = 2 / fan_in within 5 standard errors: for n values uniform on [-a, a) the mean has standard error
    a / sqrt(3 n) and the sample variance sqrt((E x^4 - (E x^2)^2) / n) = a^2 sqrt(4 / 45) / sqrt(n)"""
    H, A = 96, 18
    offs = [int(o) for o in ar.param_offsets(H, A)]
    n_all = offs[-1]
    zeros = np.zeros(n_all, np.float32)
    first = rr.first_units(H)
    for l, (layer, k) in enumerate(zip(rr.LAYERS, (0, 2, 4, 6))):  # each layer alone, so that zero-wins removes nothing
        m = _unit_mask(H, **{layer: np.arange(first[l + 1] - first[l])})
        w = rr.apply(zeros, zeros, zeros, m, KEY, H, A)[0][offs[k]:offs[k + 1]].astype(np.float64)
        a, n = float(rr.bound(layer)), w.size
        assert -a <= w.min() and w.max() < a, layer
        assert rr.bound(layer) == np.float32(np.sqrt(6.0 / rr.FAN_IN[layer]))
        if layer == "fc":
            assert n == H * 3136
            mean_se, var_se = a / np.sqrt(3 * n), a * a * np.sqrt(4 / 45) / np.sqrt(n)
            print(f"fc.w: mean {w.mean():.3g} (5 se {5 * mean_se:.3g}), variance {w.var():.6g} against {a * a / 3:.6g} "
                  f"(5 se {5 * var_se:.3g}), 2 / fan_in {2 / 3136:.6g}")
            assert abs(w.mean()) <= 5 * mean_se and abs(w.var() - a * a / 3) <= 5 * var_se
            assert abs(a * a / 3 - 2 / 3136) <= 1e-6 * (2 / 3136)  # (a_l is rounded to float32)
    fc = _unit_mask(H, fc=np.arange(H))
    a1 = rr.apply(zeros, zeros, zeros, fc, 1, H, A)[0]
    a2 = rr.apply(zeros, zeros, zeros, fc, 2, H, A)[0]
    again = rr.apply(zeros, zeros, zeros, fc, 1, H, A)[0]
    assert _same(a1, again) and (a1[offs[6]:offs[7]] != a2[offs[6]:offs[7]]).mean() > 0.999


# ------------------------------------------------------------------ CPU: the fixture through the oracle
@functools.lru_cache(maxsize=None)
def _fixture_recycled(shape, which):
    """the modified fixture after the reference recycles conv2[5] and fc[3] ("both") or conv2[5] alone ("dead")"""
    _, H, A = SHAPES[shape]
    p0 = _params(shape, True)
    z = np.zeros_like(p0)
    units = dict(conv2=[5], fc=[3]) if which == "both" else dict(conv2=[5])
    p = rr.apply(p0, z, z, _unit_mask(H, **units), KEY, H, A)[0]
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("shape", ["h32", "h96"])
def test_the_fixtures_dead_unit_fires_again_after_the_recycle(mirror, shape):
    _, H, A = SHAPES[shape]
    obs = _obs(OBS_SEED, N_OBS)
    before = asr.from_oracle_acts(orc.net_forward(_params(shape, True), H, A, obs, want_acts=True)[2], H)
    after = asr.from_oracle_acts(orc.net_forward(_fixture_recycled(shape, "both"), H, A, obs, want_acts=True)[2], H)
    assert before["conv2"][:, 5].max() == 0 and after["conv2"][:, 5].max() > 0
    ref = asr.reference(after, TAU)
    print(f"{shape}: conv2[5] max {after['conv2'][:, 5].max():.3g} score {ref['units'][32 + 5, asr.SCORE]:.3g}, "
          f"fc[3] score {ref['units'][160 + 3, asr.SCORE]:.3g}")
    assert ref["units"][32 + 5, asr.MAX_ABS] > 0 and ref["units"][160 + 3, asr.SCORE] > TAU


@pytest.mark.parametrize("shape", ["h32", "h96"])
def test_recycling_a_dead_unit_leaves_every_output_alone(mirror, shape):
    """a dead unit contributed exactly zero, and its successor's outgoing weights are now zero: equal logits and values"""
    _, H, A = SHAPES[shape]
    obs = _obs(OBS_SEED, N_OBS)
    l0, v0 = orc.net_forward(_params(shape, True), H, A, obs)
    l1, v1 = orc.net_forward(_fixture_recycled(shape, "dead"), H, A, obs)
    assert np.array_equal(l0, l1) and np.array_equal(v0, v1)
    assert not _same(_params(shape, True), _fixture_recycled(shape, "dead"))


# ------------------------------------------------------------------ GPU
def _prec(pkg, prec):
    return pkg.FP32 if prec == "fp32" else pkg.BF16


@functools.lru_cache(maxsize=None)
def _batch(A):
    """what aleppo_set_batch wants: N_BATCH observations and the planes next to them"""
    s, n = BATCH_SEED, N_BATCH
    return (_obs(s, n), (hf.hf_u32(s + 2, n) % np.uint32(A)).astype(np.int64), orc.log_softmax(hf.hf_range(s + 3, (n, A), -1, 1)),
            hf.hf_range(s + 4, (n,), -1, 1), hf.hf_range(s + 5, (n,), -1, 1),
            (hf.hf_unit(s + 6, n) >= np.float32(0.1)).astype(np.uint8))


def _engine(pkg, shape, prec, modified=False, graph=False, lr=2.5e-4, train=True, **kw):
    """E = 8, T = 8, the case's hashed parameters, then one train on the hashed batch so that the moments are non-zero"""
    _, H, A = SHAPES[shape]
    eng = pkg.Engine(8, 8, A, H, precision=_prec(pkg, prec), max_minibatch=64, **kw)
    eng.load_params(_params(shape, modified))
    if graph:
        eng.set_option(pkg.OPT_UPDATE_GRAPH, 1)
    if train:
        eng.set_batch(*_batch(A))
        eng.train(lr, 1, 2)
    return eng


def _state(eng):
    sd = eng.state_dict()
    return sd["params"], sd["exp_avg"], sd["exp_avg_sq"], int(sd["step"])


def _masks(H):
    ones = np.ones(160 + H, np.uint8)
    return [("zeros", np.zeros(160 + H, np.uint8)),
            ("one per layer", _unit_mask(H, conv1=[31], conv2=[0], conv3=[63], fc=[H - 1])),
            ("adjacent layers", _unit_mask(H, conv1=[3, 4], conv2=[3, 40], conv3=[40, 41], fc=[0, 5, H - 2])),
            ("keyed random", rr.keyed_mask(8900 + H, H)),
            ("ones", ones)]


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["h32", "h96"])
def test_state_after_a_recycle_is_the_reference_bit_for_bit(pkg, shape, prec, keep):
    _, H, A = SHAPES[shape]
    eng = _engine(pkg, shape, prec)
    grads = eng.export_grads()
    for k, (name, mask) in enumerate(_masks(H)):
        p0, m0, v0, step0 = _state(eng)
        assert m0.any() and v0.any() and step0 == 2
        digest0 = eng.state_digest()
        counts = eng.recycle_units(mask, key=KEY + k, keep_moments=keep)
        p1, m1, v1, step1 = _state(eng)
        rp, rm, rv = rr.apply(p0, m0, v0, mask, KEY + k, H, A, keep_moments=keep)
        print(f"{shape} {prec} keep={keep} {name}: {counts}, {int((_bits(p1) != _bits(p0)).sum())} parameters changed")
        assert counts == rr.counts(mask, H), name
        assert _same(p1, rp) and _same(m1, rm) and _same(v1, rv) and step1 == step0, name
        assert _same(eng.export_grads(), grads), name
        if name == "zeros":
            assert eng.state_digest() == digest0
        elif not keep:
            assert not _same(p1, p0) and not _same(m1, m0)
        else:
            assert _same(m1, m0) and _same(v1, v0)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,prec,graph", [("h32", "fp32", 0), ("h32", "bf16", 0), ("h96", "fp32", 0), ("h96", "bf16", 0),
                                              ("h96", "bf16", 1), ("h32", "fp32", 1)])
def test_derived_copies_follow_the_recycle(pkg, shape, prec, graph):
    """a twin is GIVEN the reference's state (load_params + import_optimizer rebuild every copy from scratch); the recycled
    engine must forward and train to the same bits - the only check of the bf16 copy and of W2d / W3d / WfcT"""
    _, H, A = SHAPES[shape]
    mask = rr.keyed_mask(8950 + H, H)
    assert all(c > 0 for c in rr.counts(mask, H).values())
    eng, twin = _engine(pkg, shape, prec, graph=graph), _engine(pkg, shape, prec, graph=graph)
    p0, m0, v0, step0 = _state(twin)
    assert all(_same(a, b) for a, b in zip(_state(eng)[:3], (p0, m0, v0)))
    eng.recycle_units(mask, key=KEY)
    rp, rm, rv = rr.apply(p0, m0, v0, mask, KEY, H, A)
    twin.load_state_dict(dict(params=rp, exp_avg=rm, exp_avg_sq=rv, step=step0))
    obs = _obs(OBS_SEED, N_OBS)
    (l1, v1), (l2, v2) = eng.forward(obs), twin.forward(obs)
    assert _same(l1, l2) and _same(v1, v2)
    assert not _same(l1, _engine_forward_before(pkg, shape, prec, obs))
    ma, mb = eng.train(2.5e-4, 1, 2), twin.train(2.5e-4, 1, 2)
    for k in ("loss", "grad_norm"):
        assert _same(ma[k], mb[k]), k
    assert _same(eng.export_grads(), twin.export_grads())
    for a, b, what in zip(_state(eng), _state(twin), ("params", "exp_avg", "exp_avg_sq", "step")):
        assert (a == b) if what == "step" else _same(a, b), what
    assert eng.state_digest() == twin.state_digest()
    if graph:
        print("graph replays:", eng.get_option(pkg.OPT_UPDATE_GRAPH), twin.get_option(pkg.OPT_UPDATE_GRAPH))
        assert eng.get_option(pkg.OPT_UPDATE_GRAPH) >= 1  # the capture of the first train was replayed after the recycle
    eng.close()
    twin.close()


_forward_before = {}


def _engine_forward_before(pkg, shape, prec, obs):
    """the logits of the trained, not recycled engine (computed once per case): the recycle has to move them"""
    if (shape, prec) not in _forward_before:
        e = _engine(pkg, shape, prec)
        _forward_before[(shape, prec)] = e.forward(obs)[0]
        e.close()
    return _forward_before[(shape, prec)]


@pytest.mark.gpu
@pytest.mark.parametrize("layers", ["all", "fc"])
@pytest.mark.parametrize("source", ["caller", "batch"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_recycle_dormant_on_the_fixture(pkg, prec, source, layers):
    """mask_out is the mask a twin forms on the host from activation_stats' SCORE <= tau and the layer bits; the state is
    the twin's after recycle_units(that mask); conv2[5] is alive afterwards.  (lr = 1e-12: the train only makes the moments
    non-zero, the fixture's dead and dormant units stay what they are.)"""
    shape = "h32"
    _, H, A = SHAPES[shape]
    eng, twin = (_engine(pkg, shape, prec, modified=True, lr=1e-12) for _ in range(2))
    obs = None if source == "batch" else _obs(OBS_SEED, N_OBS)  # batch: the N = 64 samples of set_batch
    units, table = twin.activation_stats(obs, tau=TAU, raw=True)
    assert not asr.fixture_facts(units, table, H)
    bits = pkg.RECYCLE_LAYERS[layers]
    first = rr.first_units(H)
    want = (units[:, asr.SCORE] <= TAU).astype(np.uint8)
    for l in range(4):
        if not bits >> l & 1:
            want[first[l]:first[l + 1]] = 0
    mask, counts = eng.recycle_dormant(obs, tau=TAU, layers=layers, key=KEY)
    print(f"{prec} {source} {layers}: {counts}")
    assert mask.dtype == np.uint8 and np.array_equal(mask, want) and counts == rr.counts(want, H)
    assert mask[160 + 3] == 1 and mask[32 + 5] == (1 if layers == "all" else 0)
    assert twin.recycle_units(want, key=KEY) == counts
    for a, b, what in zip(_state(eng), _state(twin), ("params", "exp_avg", "exp_avg_sq", "step")):
        assert (a == b) if what == "step" else _same(a, b), what
    assert eng.state_digest() == twin.state_digest()
    after = eng.activation_stats(obs, tau=TAU, raw=True)[0]
    assert after[160 + 3, asr.SCORE] > TAU
    assert (after[32 + 5, asr.MAX_ABS] > 0) == (layers == "all")
    eng.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_recycling_a_dead_unit_alone_leaves_forward_equal(pkg, prec):
    shape = "h32"
    _, H, A = SHAPES[shape]
    eng = _engine(pkg, shape, prec, modified=True, train=False)
    obs = _obs(OBS_SEED, N_OBS)
    l0, v0 = eng.forward(obs)
    p0 = eng.export_params()
    assert eng.recycle_units(_unit_mask(H, conv2=[5]), key=KEY)["total"] == 1
    l1, v1 = eng.forward(obs)
    assert not _same(eng.export_params(), p0)
    assert np.array_equal(l0, l1) and np.array_equal(v0, v1)
    eng.close()


def _raw_units(pkg, eng, mask, unit_count=None, key=KEY, flags=0, null_mask=False, null_counts=False):
    counts = np.full(5, -7, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().aleppo_recycle_units(eng._ctx, None if null_mask else ptr(mask),
                                        C.c_size_t(mask.size if unit_count is None else unit_count), C.c_uint64(key),
                                        C.c_int(flags), None if null_counts else ptr(counts))
    return rc, counts


def _raw_dormant(pkg, eng, obs, n, tau=TAU, layers=15, key=KEY, flags=0, unit_count=None, null_counts=False, null_mask=False):
    mask, counts = np.full(160 + eng.H, 7, np.uint8), np.full(5, -7, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().aleppo_recycle_dormant(eng._ctx, None if obs is None else ptr(obs), C.c_int64(n), C.c_double(tau),
                                          C.c_int(layers), C.c_uint64(key), C.c_int(flags), None if null_mask else ptr(mask),
                                          C.c_size_t(mask.size if unit_count is None else unit_count),
                                          None if null_counts else ptr(counts))
    return rc, mask, counts


def _failed_calls(pkg, eng, obs, have_batch):
    """one failed call of every kind the header lists (but the armed step): [(what, status, nothing was written)]"""
    H = eng.H
    ones, two = np.ones(160 + H, np.uint8), np.ones(160 + H, np.uint8)
    two[160 + H - 1] = 2
    out = []
    INV = pkg.ERR_INVALID_ARGUMENT
    for what, kw in (("null mask", dict(null_mask=True)), ("null counts", dict(null_counts=True)),
                     ("unit_count - 1", dict(unit_count=159 + H)), ("unit_count * 5", dict(unit_count=5 * (160 + H))),
                     ("unknown flag", dict(flags=2)), ("unknown flags", dict(flags=-1))):
        rc, counts = _raw_units(pkg, eng, ones, **kw)
        out.append(("units: " + what, rc == INV, (counts == -7).all()))
    rc, counts = _raw_units(pkg, eng, two)
    out.append(("units: a mask byte of 2", rc == INV, (counts == -7).all()))
    for what, kw in (("null counts", dict(null_counts=True)), ("unit_count", dict(unit_count=159 + H)),
                     ("unknown flag", dict(flags=4)), ("layers 0", dict(layers=0)), ("layers 16", dict(layers=16)),
                     ("layers -1", dict(layers=-1)), ("tau < 0", dict(tau=-1e-9)), ("tau nan", dict(tau=float("nan"))),
                     ("tau inf", dict(tau=float("inf")))):
        rc, mask, counts = _raw_dormant(pkg, eng, obs, obs.shape[0], **kw)
        out.append(("dormant: " + what, rc == INV, (counts == -7).all() and (mask == 7).all()))
    for o, n in ((obs, 0), (obs, -1), (obs, 65), (None, 1)):  # what aleppo_activation_stats refuses (maxB = 64)
        rc, mask, counts = _raw_dormant(pkg, eng, o, n)
        out.append((f"dormant: n = {n}", rc == INV, (counts == -7).all() and (mask == 7).all()))
    if not have_batch:
        rc, mask, counts = _raw_dormant(pkg, eng, None, 0)
        out.append(("dormant: no batch", rc == pkg.ERR_RUNTIME, (counts == -7).all() and (mask == 7).all()))
    return out


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


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_failed_calls_change_nothing(pkg, prec):
    """two engines run the same rollout and update; one makes a failed call of each kind before the rollout, between the
    rollout and the update and after it: equal actions, update metrics, digests and state"""
    E, T, A, H = 8, 8, 4, 32
    obs = np.ascontiguousarray(_obs(OBS_SEED, N_OBS))
    runs = []
    for failing in (False, True):
        eng = pkg.Engine(E, T, A, H, precision=_prec(pkg, prec), seed=3)
        eng.load_params(_params("h32"))
        out = dict(failed=[])
        if failing:
            out["failed"] += _failed_calls(pkg, eng, obs, False)
        out["acts"] = np.stack(_rollout(eng, 9700, E, T))
        if failing:
            out["failed"] += _failed_calls(pkg, eng, obs, True)
        m = eng.train(2.5e-4, 2, 2)
        if failing:
            out["failed"] += _failed_calls(pkg, eng, obs, True)
        out["metrics"] = np.stack([m[k] for k in sorted(m)])
        out["digest"] = eng.state_digest()
        out["state"] = _state(eng)
        eng.close()
        runs.append(out)
    plain, mixed = runs
    assert len(mixed["failed"]) == 3 * 20 + 1
    assert all(status and untouched for _, status, untouched in mixed["failed"]), [f for f in mixed["failed"] if not (f[1] and f[2])]
    assert np.array_equal(plain["acts"], mixed["acts"]) and _same(plain["metrics"], mixed["metrics"])
    assert plain["digest"] == mixed["digest"]
    assert all(_same(a, b) for a, b in zip(plain["state"][:3], mixed["state"][:3])) and plain["state"][3] == mixed["state"][3]


@pytest.mark.gpu
def test_errors_and_what_follows_a_recycle(pkg):
    """every refusal of the header with nothing written and the state where it was; an armed step; world_size > 1 refuses
    recycle_dormant and allows recycle_units; tensor_stats("step") is refused after a recycle until the next train"""
    shape = "h32"
    _, H, A = SHAPES[shape]
    E = 8
    eng = _engine(pkg, shape, "fp32")
    obs = np.ascontiguousarray(_obs(OBS_SEED, N_OBS))
    digest = eng.state_digest()
    failed = _failed_calls(pkg, eng, obs, True)
    assert len(failed) == 20 and all(s and u for _, s, u in failed), [f for f in failed if not (f[1] and f[2])]
    with pytest.raises(pkg.AleppoInvalidArgument, match="unit_count"):
        eng.recycle_units(np.zeros(160 + H + 1, np.uint8))
    with pytest.raises(pkg.AleppoInvalidArgument, match="0 or 1"):
        eng.recycle_units(np.full(160 + H, 3, np.uint8))
    with pytest.raises(pkg.AleppoInvalidArgument, match="layers"):
        eng.recycle_dormant(obs, layers=("conv4",))
    with pytest.raises(pkg.AleppoInvalidArgument, match="layers"):
        eng.recycle_dormant(obs, layers=())
    with pytest.raises(pkg.AleppoInvalidArgument, match="tau"):
        eng.recycle_dormant(obs, tau=-1)
    # tensor_stats: the step section describes the last optimizer step - not after a recycle, again after a train
    assert eng.state_digest() == digest
    assert eng.tensor_stats("step")["total"]["update_norm"] > 0
    rc, mask, counts = _raw_dormant(pkg, eng, obs, N_OBS, null_mask=True)  # mask_out may be NULL
    assert rc == pkg.OK and counts[4] == counts[:4].sum() >= 0
    with pytest.raises(pkg.AleppoError):
        eng.tensor_stats("step")
    assert eng.tensor_stats("params")["total"]["param_norm"] > 0
    eng.set_batch(*_batch(A))
    eng.train(2.5e-4, 1, 2)
    assert eng.tensor_stats("step")["total"]["update_norm"] > 0
    eng.recycle_units(np.zeros(160 + H, np.uint8))  # an all-zero mask is a recycle too
    with pytest.raises(pkg.AleppoError):
        eng.tensor_stats("step")
    # while a step is armed
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    frames, start = hf.hf_bytes(9180, (E * 7056,)), np.ones(E, np.uint8)
    held = _state(eng)
    eng.act()
    eng.arm_step(fbuf, sbuf)
    rc, counts = _raw_units(pkg, eng, np.ones(160 + H, np.uint8))
    assert rc == pkg.ERR_RUNTIME and (counts == -7).all()
    rc, mask, counts = _raw_dormant(pkg, eng, obs, N_OBS)
    assert rc == pkg.ERR_RUNTIME and (counts == -7).all() and (mask == 7).all()
    C.memmove(fbuf, frames.ctypes.data, E * 7056)
    C.memmove(sbuf, start.ctypes.data, E)
    eng.release_step(np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8))
    eng.synchronize()
    assert all(_same(x, y) for x, y in zip(_state(eng)[:3], held[:3]))
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
    # world_size 2 (no communicator is needed to get this far): the scores would be this rank's alone
    dp = _engine(pkg, shape, "fp32", train=False, world_size=2, rank=0)
    p0 = dp.export_params()
    rc, mask, counts = _raw_dormant(pkg, dp, obs, N_OBS)
    assert rc == pkg.ERR_RUNTIME and (counts == -7).all() and (mask == 7).all() and _same(dp.export_params(), p0)
    one = _unit_mask(H, conv3=[9])
    assert dp.recycle_units(one, key=KEY)["total"] == 1
    z = np.zeros_like(p0)
    assert _same(dp.export_params(), rr.apply(p0, z, z, one, KEY, H, A)[0])
    dp.close()
