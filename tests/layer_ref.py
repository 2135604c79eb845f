"""One layer of the forward pass, exactly: a float64 reference per layer and the element-wise checks built on it.

A plain helper module (no fixtures), shared by tests/test_layer_ref_cpu.py (the checker has room and teeth) and
tests/test_gpu_layers.py (the engine).  It uses numpy and oracle_lib.round_bf16 and nothing else.

The inputs of a layer are its input activations EXACTLY AS STORED - the byte values for conv1, the exported a1 / a2 / a3
otherwise, the exported fp32 h for the heads; all of them exact in float64 - and the fp32 master parameters.  For the bf16
model the conv and fc weights are rounded with round_bf16 and everything else stays fp32 (the rounding points are the
table in oracle/oracle.h).  Because every layer starts from the stored a(l-1) of whoever is being checked, nothing
propagates: a legitimate one-ulp flip in a1 is an INPUT of the conv2 check, not an error of it.

evaluate() computes, by im2col (sliding_window_view) and one float64 matmul per quantity,
    z  = S * scale + b      the pre-activation; S the sum of products, scale = fp32(1/255) for conv1 and 1 elsewhere.  The
                            K <= 3136 products of (at most) 24-bit significands add up in float64 with a relative error
                            below K 2^-53 Sa: z is exact for every purpose here
    Sa = scale * sum |x||w| the sum of the term magnitudes
and two float32 evaluations of the same layer on the same inputs, epilogue in float32: "blas" (one numpy float32 matmul,
the BLAS order) and "chunks" (float32 matmuls over 32 consecutive k at a time, the chunks added one after the other in
float32 - the order of a k-stepped accumulator).  They are the reference's own summation orders: what they show against z
is the floor the measured margins below are taken from, never the engine.

With u = 2^-24 and K the number of terms:

(a) interval(): a layer stored in bf16, every element, no exceptions.  eps = 2 K u Sa + 4 u |z| is the textbook bound of a
    K-term fp32 accumulation ((K - 1) u Sa, plus u Sa + 2 u |z| for the epilogue's multiply and add), doubled so that it
    does not assume that the MFMA's internal additions round to nearest - what they do has not been measured by anybody
    here, so nothing in (a) rests on it.  bf16 rounding is monotone (so is the fp32 rounding in front of it, which the
    stored fp32 pre-activation passes unchanged), hence bf16(relu(z - eps)) <= got <= bf16(relu(z + eps)).  Where the two
    ends coincide this is bit equality; elsewhere got is one of two neighbouring bf16 values, and a ReLU gate can differ
    only where |z| <= eps.  Nothing in (a) is measured.
(b) mismatches(): the same layers per output channel, the count of elements with got != bf16(relu(z)).  (a) is rigorous but
    too wide to see a weight that is one bf16 ulp off; the count sees it.  Cap per channel = FLOOR_FACTOR x the largest
    per-channel count either float32 evaluation shows on the same inputs, that count never taken below 2.
(c) fp32_check(): fp32 outputs, per element |got - act(z)| <= min(FLOOR_FACTOR R u Sa + 2 u |z|, 2 K u Sa + 4 u |z|), R the
    largest |z32 - z| / (u Sa) the "blas" evaluation shows over the layer; act is the ReLU for the conv layers of an fp32
    context (applied to both sides: a gate may differ only where |z| is within the bound) and the identity for fc and the
    heads."""
import hashlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import oracle_lib as orc

U = 2.0 ** -24
FLOOR_FACTOR = 4  # bf16_check.FLOOR_FACTOR (asserted equal by the tests)
SCALE1 = float(np.float32(1.0) / np.float32(255.0))  # the device's constant 1.0f / 255.0f
# layer: (input channels, kernel, stride, output channels)
CONV = dict(conv1=(4, 8, 4, 32), conv2=(32, 4, 2, 64), conv3=(64, 3, 1, 64))
LAYERS = ("conv1", "conv2", "conv3", "fc")
INPUT_OF = dict(conv1="obs", conv2="conv1", conv3="conv2", fc="conv3", heads="fc")
CHUNK = 32


def split_params(params, H, A, bf16):
    """{layer: (weights [rows, K] float32, bias [rows] float32)} of a flat parameter vector in the reference's order; the two
    heads are one layer "heads" of A + 1 rows (the value last).  bf16: conv and fc weights rounded, the rest untouched"""
    p = np.asarray(params, np.float32).ravel()
    sizes = [(32, 256), (64, 512), (64, 576), (H, 3136), (A, H), (1, H)]
    out, o = [], 0
    for rows, K in sizes:
        w = p[o:o + rows * K].reshape(rows, K)
        b = p[o + rows * K:o + rows * K + rows]
        o += rows * K + rows
        out.append((w, b))
    assert o == p.size, (o, p.size)
    layers = {}
    for name, (w, b) in zip(LAYERS, out[:4]):
        layers[name] = (orc.round_bf16(w) if bf16 else w.copy(), b.copy())
    layers["heads"] = (np.concatenate([out[4][0], out[5][0]]), np.concatenate([out[4][1], out[5][1]]))
    return layers


def im2col(x, k, stride, dtype):
    """[n, C, IH, IW] -> ([n * OH * OW, C * k * k] of dtype, (n, OH, OW)): rows in sample, row, column order, columns in the
    weights' (c, kh, kw) order"""
    win = sliding_window_view(np.asarray(x), (k, k), axis=(2, 3))[:, :, ::stride, ::stride]  # [n, C, OH, OW, k, k]
    n, C, OH, OW = win.shape[:4]
    return np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5), dtype=dtype).reshape(n * OH * OW, C * k * k), (n, OH, OW)


class Layer:
    """what evaluate() returns: z, Sa float64 and z32 = {"blas", "chunks"} float32, all in the export's shape ([n, C, OH, OW],
    [n, H] or [n, A + 1]); K; relu"""

    def __init__(self, name, K, relu, z, Sa, z32):
        self.name, self.K, self.relu, self.z, self.Sa, self.z32 = name, K, relu, z, Sa, z32
        self._memo = {}

    def memo(self, key, make):
        """what the reference alone determines (the floors of (b) and (c)) is computed once per Layer"""
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def act(self, z):
        return np.maximum(z, 0) if self.relu else z

    def eps(self):
        """the rigorous bound: 2 K u Sa + 4 u |z|"""
        return 2 * self.K * U * self.Sa + 4 * U * np.abs(self.z)

    def exact_bf16(self):
        """bf16(relu(z)) as float32"""
        return orc.round_bf16(self.act(self.z)).reshape(self.z.shape)

    def stored32(self, order):
        """what a float32 evaluation stores in bf16: bf16(relu(z32))"""
        return orc.round_bf16(self.act(self.z32[order])).reshape(self.z.shape)

    def channels(self, a):
        """[n, C, ...] -> [C, n * pixels]"""
        a = np.asarray(a)
        a = a.reshape(a.shape[0], a.shape[1], -1)
        return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


def evaluate(name, x, w, b, relu=None):
    """the layer `name` ("conv1" .. "conv3", "fc", "heads") on its stored input x ([n, C, IH, IW]; for fc [n, 64, 7, 7] or
    [n, 3136]; for the heads [n, H]) with weights w [rows, K] and bias b [rows] as split_params gives them"""
    x = np.asarray(x)
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    if name in CONV:
        cin, k, stride, oc = CONV[name]
        assert x.shape[1] == cin and w.shape == (oc, cin * k * k), (x.shape, w.shape)
        cols, (n, OH, OW) = im2col(x, k, stride, np.float64)
        shape = lambda m: np.ascontiguousarray(m.reshape(n, OH, OW, oc).transpose(0, 3, 1, 2))
    else:
        cols = np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], -1)
        assert cols.shape[1] == w.shape[1], (x.shape, w.shape)
        shape = lambda m: m
    K = w.shape[1]
    scale = SCALE1 if name == "conv1" else 1.0
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    z = shape(cols @ w64.T * scale + b64)
    Sa = shape(np.abs(cols) @ np.abs(w64).T * scale)
    cols32 = cols.astype(np.float32)  # exact: bytes, bf16 or fp32 values
    assert np.array_equal(cols32.astype(np.float64), cols)
    wt = np.ascontiguousarray(w.T)
    s32, b32 = np.float32(scale), b[None, :]
    z32 = {"blas": shape((cols32 @ wt) * s32 + b32)}
    acc = np.zeros((cols32.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, K, CHUNK):
        acc += cols32[:, k0:k0 + CHUNK] @ wt[k0:k0 + CHUNK]
    z32["chunks"] = shape(acc * s32 + b32)
    assert z32["blas"].dtype == np.float32 and z32["chunks"].dtype == np.float32
    return Layer(name, K, name in CONV if relu is None else relu, z, Sa, z32)


def forward_refs(params, H, A, bf16, obs, acts, layers=LAYERS, cache=None):
    """{layer: Layer} of a whole export `acts` ({"conv1": ..., "conv2": ..., "conv3": ..., "fc": ...} float32), every layer on
    the export's own previous layer; "heads" (if asked for) on the exported fc.  cache: a dict the caller keeps for ONE set
    of parameters and one precision; a layer whose stored input has the same bytes as before is not evaluated again (routes
    that export identical bits share their references)"""
    p = split_params(params, H, A, bf16)
    src = dict(acts, obs=np.asarray(obs))
    cache = {} if cache is None else cache
    out = {}
    for l in layers:
        x = np.ascontiguousarray(src[INPUT_OF[l]])
        key = (l, x.dtype.str, x.shape, hashlib.sha1(x.view(np.uint8).reshape(-1)).digest())
        if key not in cache:
            cache[key] = evaluate(l, x, *p[l])
        out[l] = cache[key]
    return out


# ------------------------------------------------------------------ (a)
def next_bf16(a, up=True):
    """the neighbouring bf16 value (of positive bf16 values held as float32), away from / towards zero"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (bits + np.uint32(0x10000) if up else bits - np.uint32(0x10000)).view(np.float32)


def interval(ref):
    """(lo, hi) float32: bf16(relu(z - eps)), bf16(relu(z + eps))"""
    eps = ref.eps()
    lo = orc.round_bf16(ref.act(ref.z - eps)).reshape(ref.z.shape)
    hi = orc.round_bf16(ref.act(ref.z + eps)).reshape(ref.z.shape)
    return lo, hi


def interval_check(ref, got):
    """check (a): dict(violations = indices [m, ndim] of the elements outside their interval, single = the share of elements
    whose interval is one value, gates = the number of elements whose gate differs from the exact one (each of them has
    |z| <= eps, or it is a violation), active = the share of elements with z > 0)"""
    got = np.asarray(got, np.float32)
    assert got.shape == ref.z.shape, (got.shape, ref.z.shape)
    lo, hi = interval(ref)
    with np.errstate(invalid="ignore"):
        bad = ~((lo <= got) & (got <= hi))  # (a NaN is outside)
    return dict(violations=np.argwhere(bad), single=float((lo == hi).mean()),
                gates=int(((got > 0) != (ref.z > 0)).sum()), active=float((ref.z > 0).mean()))


# ------------------------------------------------------------------ (b)
def mismatches(ref, got):
    """per output channel, the number of elements with got != bf16(relu(z))"""
    exact = ref.memo("exact", lambda: ref.channels(ref.exact_bf16()))
    return (ref.channels(np.asarray(got, np.float32)) != exact).sum(axis=1)


def mismatch_check(ref, got):
    """check (b): dict(counts [C], cap, floor = the larger of the two float32 evaluations' largest per-channel counts,
    failures = the channels over the cap)"""
    floor = ref.memo("floor", lambda: max(int(mismatches(ref, ref.stored32(o)).max()) for o in ref.z32))
    cap = FLOOR_FACTOR * max(floor, 2)
    counts = mismatches(ref, got)
    return dict(counts=counts, cap=cap, floor=floor, failures=np.flatnonzero(counts > cap))


# ------------------------------------------------------------------ (c)
def measured_ratio(ref, value):
    """max |value - z| / (u Sa) over the elements with Sa > 0 (value a pre-activation, or an activation for which the ReLU is
    then applied to z as well)"""
    d = np.abs(np.asarray(value, np.float64) - ref.z)
    ok = ref.Sa > 0
    return float((d[ok] / (U * ref.Sa[ok])).max()) if ok.any() else 0.0


def fp32_bound(ref):
    """(c)'s bound per element, and R = the "blas" evaluation's ratio it is built on"""
    R = ref.memo("R", lambda: measured_ratio(ref, ref.z32["blas"]))
    return np.minimum(FLOOR_FACTOR * R * U * ref.Sa + 2 * U * np.abs(ref.z), ref.eps()), R


def fp32_check(ref, got, extra=0.0):
    """check (c): dict(violations = indices of the elements outside the bound, R = the "blas" evaluation's ratio, ratio = the
    same measurement of got, worst = the largest |got - act(z)| / bound); extra: more room per element, added to the bound
    (tests/backward_ref.py: what a stated uncertainty of an input can move)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.z.shape, (got.shape, ref.z.shape)
    bound, R = fp32_bound(ref)
    bound = bound + extra
    d = np.abs(got - ref.act(ref.z))
    ok = ref.Sa > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = ~(d <= bound)
        worst = np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0)).max()
    ratio = float((d[ok] / (U * ref.Sa[ok])).max()) if ok.any() else 0.0
    return dict(violations=np.argwhere(bad), R=R, ratio=ratio, worst=float(worst))


# ------------------------------------------------------------------ a whole export
def check_export(params, H, A, bf16, obs, acts, heads=None, layers=LAYERS, cache=None):
    """every layer of an export on the export's own previous layer: (a) and (b) on the conv layers of a bf16 export, (c) on
    its fc and on every layer of an fp32 export; heads = (logits [n, A], values [n]) of the same observations adds (c) on
    the two heads, from the exported fc; layers / cache: as forward_refs takes them.  Returns (failures, report, results):
    failures a list of strings, report {layer: text} (the numbers a test prints), results {layer: the checks' dicts and
    the Layer}"""
    layers = tuple(layers) + (("heads",) if heads is not None else ())
    refs = forward_refs(params, H, A, bf16, obs, acts, layers, cache)
    got = dict(acts)
    if heads is not None:
        got["heads"] = np.concatenate([np.asarray(heads[0], np.float32), np.asarray(heads[1], np.float32)[:, None]], axis=1)
    failures, report, results = [], {}, {}
    for l in layers:
        ref = refs[l]
        if bf16 and l in CONV:
            a, b = interval_check(ref, got[l]), mismatch_check(ref, got[l])
            results[l] = dict(ref=ref, a=a, b=b)
            report[l] = "(a) %d outside, single %.3f, gates %d; (b) worst channel %d/%d (floor %d)" % (
                len(a["violations"]), a["single"], a["gates"], b["counts"].max(), b["cap"], b["floor"])
            if len(a["violations"]):
                i = tuple(a["violations"][0])
                failures.append("%s (a): %d elements outside their interval, first %s: got %r, z %r, eps %r" % (
                    l, len(a["violations"]), i, float(got[l][i]), float(ref.z[i]), float(ref.eps()[i])))
            if len(b["failures"]):
                failures.append("%s (b): channels %s have %s mismatches, cap %d" % (
                    l, b["failures"][:8].tolist(), b["counts"][b["failures"]][:8].tolist(), b["cap"]))
        else:
            c = fp32_check(ref, got[l])
            results[l] = dict(ref=ref, c=c)
            report[l] = "(c) max |d| / (u Sa) %.3g against R %.3g, worst |d| / bound %.3g" % (c["ratio"], c["R"], c["worst"])
            if len(c["violations"]):
                i = tuple(c["violations"][0])
                failures.append("%s (c): %d elements outside the bound, first %s: got %r, z %r, Sa %r, R %.3g" % (
                    l, len(c["violations"]), i, float(got[l][i]), float(ref.z[i]), float(ref.Sa[i]), c["R"]))
    return failures, report, results


def summary(title, report):
    return title + "".join("\n    %-6s %s" % (l, t) for l, t in report.items())
