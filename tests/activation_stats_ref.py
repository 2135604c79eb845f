"""aleppo_activation_stats, restated: the float64 reference built from exported activations, and the bounds a device answer
has to meet.  A plain helper module (no fixtures), shared by the CPU and GPU tests of tests/test_activation_stats.py.

The reference works on what aleppo_forward_activations exports (or what oracle_lib.net_forward(want_acts=True) saves):
{"conv1": [n,32,20,20], "conv2": [n,64,9,9], "conv3": [n,64,7,7], "fc": [n,H]} float32.  Unit i of a layer has K = n * PIX
positions; over its finite elements S = sum |a|, P = #{a > 0}, X = max |a|; a non-finite element is counted (NONFINITE) and
left out of everything else.  Rows and columns: include/aleppo.h.

Bounds, derived (u53 = 2^-53):
    any order of adding K non-negative doubles is within (K - 1) u53 S of the exact sum; the reference's own sums are
    exact sums rounded once (math.fsum), and one division follows on either side, so
    MEAN_ABS (unit)      relative 2 K u53
    SCORE                that plus the same term for the layer mean, whose `units` terms add another (units - 1) u53 on
                         either side: relative (4 K + 2 units) u53
    MEAN_ABS (layer)     the layer's sum is SOME order of adding its E = units K elements: relative 2 E u53; the total row
                         likewise with E the four layers' elements
    DORMANT              between the reference's counts at tau (1 - b) and tau (1 + b), b the layer's SCORE bound
    everything else      (counts, maxima, P / K, UNITS, ELEMENTS, DEAD) equal
"""
import math

import numpy as np

LAYERS = ("conv1", "conv2", "conv3", "fc")
ROWS = LAYERS + ("total",)
CHANNELS = dict(conv1=32, conv2=64, conv3=64)
PIX = dict(conv1=400, conv2=81, conv3=49, fc=1)
UNIT_STATS = ("mean_abs", "positive_fraction", "max_abs", "score", "nonfinite")
LAYER_STATS = ("units", "elements", "mean_abs", "positive_fraction", "max_abs", "dead", "dormant", "nonfinite")
MEAN_ABS, POSITIVE_FRACTION, MAX_ABS, SCORE, NONFINITE = range(5)
L_UNITS, L_ELEMENTS, L_MEAN_ABS, L_POSITIVE_FRACTION, L_MAX_ABS, L_DEAD, L_DORMANT, L_NONFINITE = range(8)
U53 = 2.0 ** -53


def first_units(H):
    """first unit row of each layer, then the unit count"""
    return (0, 32, 96, 160, 160 + H)


def from_oracle_acts(acts, H):
    """oracle_lib.net_forward(want_acts=True)'s saved activations [n, 28224 + 12800 + 5184 + 3136 + H] -> the export's dict"""
    a = np.asarray(acts, np.float32)
    n = a.shape[0]
    o = 4 * 84 * 84
    out = {}
    for name, shape in (("conv1", (32, 20, 20)), ("conv2", (64, 9, 9)), ("conv3", (64, 7, 7)), ("fc", (H,))):
        size = int(np.prod(shape))
        out[name] = a[:, o:o + size].reshape((n,) + shape).copy()
        o += size
    assert o == a.shape[1]
    return out


def unit_rows(x):
    """an exported layer [n, C, ...] -> [C, n * PIX]: one row per unit, samples in order"""
    x = np.asarray(x, np.float32)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(x.shape[1], -1)


def concat(parts):
    """exports of consecutive sample ranges -> one export"""
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def reference(acts, tau):
    """dict(units=float64 [160 + H, 5], layers=float64 [5, 8], unit_rtol=[160 + H, 5], layer_rtol=[5, 8],
    dormant=[(lo, hi)] * 5): the tables of aleppo.h from exported activations, the relative bounds of the module docstring
    (0: equal) and the range DORMANT has to lie in"""
    H = int(np.asarray(acts["fc"]).shape[1])
    first = first_units(H)
    units = np.zeros((first[4], 5), np.float64)
    layers = np.zeros((5, 8), np.float64)
    unit_rtol, layer_rtol = np.zeros_like(units), np.zeros_like(layers)
    dormant, sums, positives = [], [], []
    for l, name in enumerate(LAYERS):
        rows = unit_rows(acts[name])
        C, K = rows.shape
        assert C == first[l + 1] - first[l] and K % PIX[name] == 0
        ok = np.isfinite(rows)
        mag = np.where(ok, np.abs(rows), np.float32(0)).astype(np.float64)
        S = np.array([math.fsum(r.tolist()) for r in mag])
        P = (ok & (rows > 0)).sum(axis=1).astype(np.float64)
        u = units[first[l]:first[l + 1]]
        u[:, MEAN_ABS] = S / K
        u[:, POSITIVE_FRACTION] = P / K
        u[:, MAX_ABS] = mag.max(axis=1)
        u[:, NONFINITE] = K - ok.sum(axis=1)
        layer_mean = math.fsum(u[:, MEAN_ABS].tolist()) / C
        u[:, SCORE] = u[:, MEAN_ABS] / layer_mean if layer_mean != 0 else 0.0
        b = (4 * K + 2 * C) * U53
        unit_rtol[first[l]:first[l + 1], MEAN_ABS] = 2 * K * U53
        unit_rtol[first[l]:first[l + 1], SCORE] = b
        sums.append(math.fsum(S.tolist()))
        positives.append(P.sum())
        E = float(C) * K
        layers[l] = (C, E, sums[l] / E, positives[l] / E, u[:, MAX_ABS].max(), (u[:, MAX_ABS] == 0).sum(),
                     (u[:, SCORE] <= tau).sum(), u[:, NONFINITE].sum())
        layer_rtol[l, L_MEAN_ABS] = 2 * E * U53
        dormant.append((int((u[:, SCORE] <= tau * (1 - b)).sum()), int((u[:, SCORE] <= tau * (1 + b)).sum())))
    E = layers[:4, L_ELEMENTS].sum()
    layers[4] = (layers[:4, L_UNITS].sum(), E, math.fsum(sums) / E, sum(positives) / E, layers[:4, L_MAX_ABS].max(),
                 layers[:4, L_DEAD].sum(), layers[:4, L_DORMANT].sum(), layers[:4, L_NONFINITE].sum())
    layer_rtol[4, L_MEAN_ABS] = 2 * E * U53
    dormant.append((sum(d[0] for d in dormant), sum(d[1] for d in dormant)))
    return dict(units=units, layers=layers, unit_rtol=unit_rtol, layer_rtol=layer_rtol, dormant=dormant)


def unit_name(i, H):
    first = first_units(H)
    l = max(k for k in range(4) if i >= first[k])
    return f"{LAYERS[l]}[{i - first[l]}]"


def check(units, layers, ref):
    """failures of a device answer against reference(): list of (where, stat, device, reference, bound)"""
    units, layers = np.asarray(units, np.float64), np.asarray(layers, np.float64)
    assert units.shape == ref["units"].shape and layers.shape == (5, 8)
    H = units.shape[0] - 160
    bad = []
    bound = ref["unit_rtol"] * np.abs(ref["units"])
    for i, j in zip(*np.nonzero(~(np.abs(units - ref["units"]) <= bound))):
        bad.append((unit_name(i, H), UNIT_STATS[j], float(units[i, j]), float(ref["units"][i, j]), float(bound[i, j])))
    bound = ref["layer_rtol"] * np.abs(ref["layers"])
    for l, j in zip(*np.nonzero(~(np.abs(layers - ref["layers"]) <= bound))):
        if j != L_DORMANT:
            bad.append((ROWS[l], LAYER_STATS[j], float(layers[l, j]), float(ref["layers"][l, j]), float(bound[l, j])))
    for l, (lo, hi) in enumerate(ref["dormant"]):
        if not lo <= layers[l, L_DORMANT] <= hi or layers[l, L_DORMANT] != int(layers[l, L_DORMANT]):
            bad.append((ROWS[l], "dormant", float(layers[l, L_DORMANT]), float(lo), float(hi)))
    return bad


def worst(units, layers, ref):
    """{stat: largest |device - reference| / bound} over the bounded entries (printed by the tests)"""
    out = {}
    for name, dev, want, rtol, col in (("unit mean_abs", units, ref["units"], ref["unit_rtol"], MEAN_ABS),
                                       ("unit score", units, ref["units"], ref["unit_rtol"], SCORE),
                                       ("layer mean_abs", layers, ref["layers"], ref["layer_rtol"], L_MEAN_ABS)):
        b = rtol[:, col] * np.abs(want[:, col])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(b > 0, np.abs(np.asarray(dev)[:, col] - want[:, col]) / b, 0.0)
        out[name] = float(np.max(r))
    return out


# ------------------------------------------------------------------ the fixture: one dead and one dormant unit by design
def modified_params(params, H, A):
    """conv2 channel 5 gets weights 0 and bias -1 (its ReLU never fires: exactly 0 on any implementation); fc row 3 and its
    bias are multiplied by 1e-3 (tau-dormant at tau = 0.025, not dead)"""
    import adam_ref as ar
    offs = ar.param_offsets(H, A)
    p = np.array(params, np.float32, copy=True)
    p[int(offs[2]) + 5 * 512:int(offs[2]) + 6 * 512] = 0
    p[int(offs[3]) + 5] = -1
    p[int(offs[6]) + 3 * 3136:int(offs[6]) + 4 * 3136] *= np.float32(1e-3)
    p[int(offs[7]) + 3] *= np.float32(1e-3)
    return p


def fixture_facts(units, layers, H, tau=0.025):
    """the three facts of the modified fixture, from any pair of tables computed at `tau`: failures as strings"""
    units = np.asarray(units, np.float64)
    first = first_units(H)
    bad = []
    c5 = units[first[1] + 5]
    if not (c5[MAX_ABS] == 0 and c5[MEAN_ABS] == 0 and c5[SCORE] == 0 and c5[POSITIVE_FRACTION] == 0):
        bad.append(f"conv2[5] is not dead: {c5}")
    fc = units[first[3]:first[4]]
    if not (0 < fc[3, SCORE] <= tau and fc[3, MAX_ABS] > 0):
        bad.append(f"fc[3] is not tau-dormant and alive: {fc[3]}")
    others = np.delete(fc[:, SCORE], 3)
    if not others.min() >= 0.3:
        bad.append(f"an fc unit other than 3 has score {others.min()} < 0.3")
    if not (layers[1][L_DEAD] >= 1 and layers[3][L_DORMANT] == 1 and layers[3][L_DEAD] == 0):
        bad.append(f"layer rows: conv2 dead {layers[1][L_DEAD]}, fc dormant {layers[3][L_DORMANT]}, dead {layers[3][L_DEAD]}")
    return bad
