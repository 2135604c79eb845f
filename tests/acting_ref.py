"""The acting path link by link: the references of tests/test_gpu_acting.py and the inputs of its rows.

A plain helper module (no fixtures) in the style of tests/layer_ref.py, whose evaluate(), interval (a), mismatches (b) and
fp32_check (c) it uses unchanged; shared by tests/test_acting_ref_cpu.py (room and teeth) and tests/test_gpu_acting.py (the
engine).  Every link starts from what aleppo_export_acting returns of the link in front of it, exact in float64, so nothing
propagates and a failure names the link.  u = 2^-24.

Conv links (act_conv_kernel<0 / 1 / 2>, or the generic / fp32 launches).  layer_ref.evaluate on the stored input: the slot's
    byte stack for conv1, the exported a1 / a2 for conv2 / conv3.  bf16: (a) and (b); fp32: (c).  No new bound.
One fc slice (fc_act_kernel, the fp32 split-K gemm_nt_kernel).  Slice z of FC_SPLITS = 7 is the K = 448 product of columns
    [448 z, 448 (z + 1)) of a3 in its STORED order - pixel-major, channel last, i.e. row z of the 7x7 map with its 64
    channels - with the matching fc weights (bf16-rounded for a bf16 context), no bias: slice_refs().  Bounded as (c) with
    K = 448.
The hidden vector.  h = ((bfc + p0) + p1) + ... + p6 in float32, in that order: hidden().  Plain IEEE additions of values
    the export holds exactly, so the restatement is exact and has no bound.  The acting head forms h on the fly
    (act_head.hpp: head_hidden) and never stores it.
The head (head_dot).  Logits and value = the float64 dot of THAT h with Wh, plus bh: layer_ref.evaluate("heads").  Bounded
    as (c) with K = H: min(FLOOR_FACTOR R u Sa + 2u |z|, 2 K u Sa + 4u |z|).  The rigorous form counts one rounding per
    product and one per addition; a contracted s += hv * w (one rounding instead of two) only removes roundings, so the
    bound holds whichever the compiler chose, and head_dot_f32() restates the device's order both ways to show that the
    floor-derived cap has room for either.  On f16 planes the stored value must lie in [f16(z - bound), f16(z + bound)]:
    rounding to binary16 is monotone.
The sampler, on the engine's OWN fp32 logits: eval_ref.sample at tau = 1 (the exponent's multiplication by inv = 1 is exact)
    with its SAMPLE_GAP rule - a draw whose two largest p / q are within 1e-5 of each other is left out, and at most
    LEFT_OUT_CAP of a row's draws may be.  Exact ties have their own restatement, tie_cases(): equal logits and equal noise on
    a subset of lanes give bit-equal p / q there, every other lane is lower by a factor that no rounding bridges
    (asserted in float64), and the first maximum - the lowest index of the subset - must win; with q so small that p / q is
    +inf on the subset the same holds (inf == inf).  sample_f32() is the float32 rule with a selectable tie-break.
The generator (act_head.hpp: exp1_noise).  act_noise(seed, n, E, A) = eval_ref.philox_noise under the key config.seed
    itself, counter words {n lo, n hi, e, k / 4}, q_k = -logf(U(c[k % 4])).  n is the acting counter of include/aleppo.h: + 1
    for every acting head enqueued, with caller noise too, and for aleppo_finish_rollout's discarded draw.
Old log-probs (oldlp_kernel).  The float64 log-softmax of the STORED logits plane, widened; bound = head_ref's derived one
    for a log-softmax with an exact input (backward_ref's e_lp: a max, A expf, the A-term sum, one logf, two subtractions):
    2 (A + 5) u (max |z| + |lse| + 1) + A T, T = 2^-126 on the rows where some p is below 2^-100 and 0 elsewhere.  On f16
    planes the interval form, as for the head."""
import functools

import numpy as np

import eval_ref as er
import hashfill as hf
import layer_ref as lr
import oracle_lib as orc

U = lr.U
FC_SPLITS, KC = 7, 448
TINY = 2.0 ** -126
CONVS = ("conv1", "conv2", "conv3")
LEFT_OUT_CAP = 0.01
TIE_MARGIN = 1e-3  # every lane outside a tie's subset is lower by at least this relative amount (asserted in float64)
Q_INF = np.float32(1e-45)  # the smallest positive float32: p / q overflows for every p above 5e-7 (and p / 0 = +inf if flushed)
LUT = ((np.arange(256) * 7) % 256).astype(np.uint8)
LUT[255] = 255  # (and LUT[0] = 0): the all-zero and the all-255 sample stay what they are through the palette
LUT.setflags(write=False)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------ inputs (CPU only)
@functools.lru_cache(maxsize=None)
def protocol(seed, E, raw, steps=3):
    """the frames of `steps` environment steps and the stacks they leave, through the real protocol: (frames uint8 [steps, E,
    7056 or 2 * 210 * 160], episode starts uint8 [steps, E], stacks uint8 [E, 4, 84, 84] after the last step, by
    oracle_lib.update_observations from an all-zero start).  Sample 0 is all zeros; sample 1 is all 255 with an episode start
    at the first step, so that all four of its frames are 255; the other samples are hashed bytes with hashed starts"""
    per = 2 * 210 * 160 if raw else 84 * 84
    frames = hf.hf_bytes(seed, (steps, E, per)).copy()
    starts = (hf.hf_unit(seed + 1, steps * E) < np.float32(0.25)).astype(np.uint8).reshape(steps, E)
    frames[:, 0] = 0
    if E > 1:
        frames[:, 1] = 255
        starts[0, 1] = 1
    obs = np.zeros((E, 4, 84, 84), np.uint8)
    for t in range(steps):
        f84 = orc.preprocess(frames[t].reshape(E, 2, 210, 160), LUT) if raw else frames[t].reshape(E, 84, 84)
        obs = orc.update_observations(obs, f84, starts[t])
    if E > 1:
        assert not obs[0].any() and (obs[1] == 255).all()
    return _freeze(frames, starts, obs)


@functools.lru_cache(maxsize=None)
def row_params(E, H, A):
    return _freeze(hf.fill_params(9100 + E + H + A, H, A))


def exp1(seed, shape):
    """hashed Exp(1) draws: -log of a hashed uniform in (0, 1), float32"""
    n = int(np.prod(shape))
    u = ((hf.hf_u32(seed, n) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return (-np.log(u)).astype(np.float32).reshape(shape)


REGIMES = dict(uniform=None, peaked=45.0, underflow=120.0)  # the largest per-row logit spread of the CPU oracle's forward


@functools.lru_cache(maxsize=None)
def sampler_case(E, H, A, regime):
    """(parameters, frames, starts, stacks) of a sampler row: one protocol step of hashed frames in which EVERY environment
    starts an episode (four equal frames: the rows' hidden vectors are then of one size, and one scale of the head puts
    the per-row spreads within a factor of 2.7 of each other); hashed parameters with the action head's weights and biases
    scaled so that the largest per-row logit spread of the CPU oracle's fp32 forward is REGIMES[regime] (tests/
    test_gpu_head.py's SPREAD; "uniform": the hashed head as it is).  Measured: "peaked" rows 17 .. 45 with 97 % and more
    at 20 or above, "underflow" rows 46 .. 120"""
    frames = hf.hf_bytes(6100 + E + A, (1, E, 84 * 84))
    starts = np.ones((1, E), np.uint8)
    obs = orc.update_observations(np.zeros((E, 4, 84, 84), np.uint8), frames[0].reshape(E, 84, 84), starts[0])
    _freeze(frames, starts, obs)
    params = np.array(hf.fill_params(6200 + E + H + A, H, A))
    target = REGIMES[regime]
    if target is not None and A > 1:
        offs = orc.param_offsets(H, A)
        logits = orc.net_forward(params, H, A, obs)[0]
        spread = float((logits.max(axis=1) - logits.min(axis=1)).max())
        params[offs[8]:offs[10]] *= np.float32(target / spread)
    return _freeze(params), frames, starts, obs


# ------------------------------------------------------------------ one fc slice
def slice_refs(a3, wfc):
    """the FC_SPLITS layer_ref.Layer of the stored a3 [n, 64, 7, 7] and the fc weights [H, 3136] in the reference's order (as
    layer_ref.split_params gives them): slice z = row z of the map, its columns in the stored (x, channel) order"""
    a3, wfc = np.asarray(a3), np.asarray(wfc, np.float32)
    n, H = a3.shape[0], wfc.shape[0]
    x = a3.reshape(n, 64, 7, 7).transpose(0, 2, 3, 1)       # [n, y, x, c]
    w = wfc.reshape(H, 64, 7, 7).transpose(0, 2, 3, 1)      # [H, y, x, c]
    zero = np.zeros(H, np.float32)
    return [lr.evaluate("fc", np.ascontiguousarray(x[:, z]).reshape(n, KC), np.ascontiguousarray(w[:, z]).reshape(H, KC),
                        zero, relu=False) for z in range(FC_SPLITS)]


def check_slices(refs, parts):
    """(c) on every slice: (failures, worst |d| / bound over the slices, [ratio / R per slice])"""
    failures, worst, ratios = [], 0.0, []
    for z, ref in enumerate(refs):
        c = lr.fp32_check(ref, parts[z])
        worst = max(worst, c["worst"])
        ratios.append((c["ratio"], c["R"]))
        if len(c["violations"]):
            i = tuple(c["violations"][0])
            failures.append("fc slice %d (c): %d elements outside the bound, first %s: got %r, z %r, Sa %r, R %.3g" % (
                z, len(c["violations"]), i, float(parts[z][i]), float(ref.z[i]), float(ref.Sa[i]), c["R"]))
    return failures, worst, ratios


# ------------------------------------------------------------------ the hidden vector and the head
def hidden(bfc, parts):
    """h = ((bfc + p0) + p1) + ... in float32, exactly as head_hidden adds them"""
    parts = np.asarray(parts, np.float32)
    h = np.broadcast_to(np.asarray(bfc, np.float32), parts.shape[1:]).copy()
    for z in range(parts.shape[0]):
        h = h + parts[z]
        assert h.dtype == np.float32
    return h


def head_ref(h, wh, bh):
    """the Layer of the two heads (A + 1 rows, the value last) on the float32 hidden vector"""
    return lr.evaluate("heads", h, wh, bh, relu=False)


def head_got(logits, values):
    return np.concatenate([np.asarray(logits, np.float32), np.asarray(values, np.float32).reshape(-1, 1)], axis=1)


def f16_interval(z, bound):
    """[f16(z - bound), f16(z + bound)] as float64"""
    with np.errstate(over="ignore"):
        return (z - bound).astype(np.float16).astype(np.float64), (z + bound).astype(np.float16).astype(np.float64)


def check_head(ref, got, f16):
    """(failures, worst |d| / bound - on f16 planes the share of elements whose interval is one value)"""
    got = np.asarray(got, np.float64)
    if not f16:
        c = lr.fp32_check(ref, got)
        bad = c["violations"]
        msg = ["head (c): %d elements outside the bound, first %s: got %r, z %r, R %.3g" % (
            len(bad), tuple(bad[0]), float(got[tuple(bad[0])]), float(ref.z[tuple(bad[0])]), c["R"])] if len(bad) else []
        return msg, c["worst"]
    bound, _ = lr.fp32_bound(ref)
    lo, hi = f16_interval(ref.z, bound)
    bad = np.argwhere(~((lo <= got) & (got <= hi)))
    msg = ["head (f16 interval): %d elements outside, first %s: got %r, z %r, bound %r" % (
        len(bad), tuple(bad[0]), float(got[tuple(bad[0])]), float(ref.z[tuple(bad[0])]), float(bound[tuple(bad[0])]))] \
        if len(bad) else []
    return msg, float((lo == hi).mean())


def head_dot_f32(h, wh, bh, contract, drop_second_half_of_lane=None):
    """float32 restatement of head_dot in the device's order: lane l owns hidden units 4l .. 4l + 3 and H / 2 + 4l .., adds
    its eight products one after the other, the 64 lanes meet in the xor butterfly (offsets 32 .. 1), then the bias.
    contract: s += hv * w as one fused multiply-add (the product exact, one rounding) instead of two roundings.
    drop_second_half_of_lane: a fault for the teeth - that lane leaves its H / 2 + 4l .. products out"""
    h, wh, bh = np.asarray(h, np.float32), np.asarray(wh, np.float32), np.asarray(bh, np.float32)
    n, H = h.shape
    out = np.zeros((n, wh.shape[0]), np.float32)
    lanes = np.arange(64)
    own = lanes * 8 < H
    idx = np.stack([np.where(own, lanes * 4 + i, 0) for i in range(4)] + [np.where(own, H // 2 + lanes * 4 + i, 0)
                                                                          for i in range(4)], axis=1)  # [64, 8]
    for a in range(wh.shape[0]):
        s = np.zeros((n, 64), np.float32)
        for i in range(8):
            x, w = h[:, idx[:, i]], wh[a, idx[:, i]][None, :]
            if contract:
                t = (s.astype(np.float64) + x.astype(np.float64) * w.astype(np.float64)).astype(np.float32)
            else:
                t = s + x * w
            live = own.copy()
            if drop_second_half_of_lane is not None and i >= 4:
                live[drop_second_half_of_lane] = False
            s = np.where(live[None, :], t, s).astype(np.float32)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        out[:, a] = s[:, 0] + bh[a]
    return out


# ------------------------------------------------------------------ the sampler
def sample_check(logits, q, actions):
    """the gap rule: (mismatching draws among those the restatement decides, the share it leaves out, the restatement's
    actions)"""
    want, gap = er.sample(logits, 1.0, q)
    decided = gap >= er.SAMPLE_GAP
    return np.flatnonzero(decided & (np.asarray(actions) != want)), float(1.0 - decided.mean()), want


def sample_f32(p, q, last=False):
    """argmax of p / q in float32 - the first maximum, or (a fault for the teeth) the last"""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        r = np.asarray(p, np.float32) / np.asarray(q, np.float32)
    if last:
        return (r.shape[1] - 1 - np.argmax(r[:, ::-1], axis=1)).astype(np.int64)
    return np.argmax(r, axis=1).astype(np.int64)


def tie_subsets(A):
    """the subsets of lanes a tie row ties: pairs at both ends and across the wave's halves of the butterfly; lanes 16 and
    17 at A = 18"""
    if A == 1:
        return [(0,)]
    subs = [(0, A - 1), (A - 2, A - 1), (1, A // 2), tuple(range(A))]
    if A == 18:
        subs += [(16, 17), (3, 16, 17), (7, 8, 15, 16)]
    return [tuple(sorted(set(s))) for s in subs]


@functools.lru_cache(maxsize=None)
def tie_cases(A):
    """(bias float32 [A], probabilities float32 [n, A], noise float32 [n, A], expected int64 [n]) of the exact-tie rows of an
    action count.  The biases are the logits of a zero action head, the same on every lane, so that the softmax gives
    bit-equal p on all lanes and the noise alone decides: row i has q = 1/4 on its subset and 1
    elsewhere (equal p / q on the subset, a quarter of it elsewhere), or q = Q_INF on its subset (p / q = +inf there).
    The probabilities are aleppo_sample's input for the same rows: 1 / |lanes| on the lanes that are not zeroed - every
    lane outside the subset with an odd index is given probability 0.  expected = the lowest lane of the subset."""
    subs = tie_subsets(A)
    n = 2 * len(subs)
    bias = np.full(A, 0.25, np.float32)
    q = np.ones((n, A), np.float32)
    probs = np.zeros((n, A), np.float32)
    expected = np.zeros(n, np.int64)
    for i, s in enumerate(subs + subs):
        inf = i >= len(subs)
        q[i, list(s)] = Q_INF if inf else np.float32(0.25)
        keep = [k for k in range(A) if k in s or k % 2 == 0]
        probs[i, keep] = np.float32(1.0 / len(keep))
        expected[i] = s[0]
    for p in (np.full((n, A), 1.0 / A), probs.astype(np.float64)):  # no rounding bridges the gap to the other lanes
        with np.errstate(divide="ignore", over="ignore"):
            r = p / q.astype(np.float64)
        r = np.where(q == Q_INF, np.inf, r)
        for i, s in enumerate(subs + subs):
            top = r[i, list(s)]
            rest = np.delete(r[i], list(s))
            assert (top == top[0]).all() and (rest.size == 0 or rest.max() <= top[0] * (1 - TIE_MARGIN)), (A, i)
    return _freeze(bias, probs, q, expected)


# ------------------------------------------------------------------ the generator
def act_noise(seed, n, E, A):
    """aleppo_act's built-in Exp(1) draws of acting-counter value n: float32 [E, A] (up to logf's last bits)"""
    return er.philox_noise(seed, n, E, A, "sample")


# ------------------------------------------------------------------ old log-probs
def oldlp_ref(logits):
    """(log-softmax float64, bound float64) of a stored logits plane [..., A], widened"""
    z = np.asarray(logits, np.float32).astype(np.float64)
    A = z.shape[-1]
    mx = z.max(axis=-1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True))
    lp = z - lse
    T = np.where(np.exp(lp).min(axis=-1, keepdims=True) < 2.0 ** -100, TINY, 0.0)
    bound = 2 * (A + 5) * U * (np.abs(z).max(axis=-1, keepdims=True) + np.abs(lse) + 1) + A * T
    return lp, np.broadcast_to(bound, lp.shape)


def check_oldlp(logits, got, f16):
    """(failures, worst |d| / bound - on f16 planes the share of single-valued intervals)"""
    lp, bound = oldlp_ref(logits)
    got = np.asarray(got, np.float64)
    if f16:
        lo, hi = f16_interval(lp, bound)
        bad = np.argwhere(~((lo <= got) & (got <= hi)))
        worst = float((lo == hi).mean())
    else:
        d = np.abs(got - lp)
        bad = np.argwhere(~(d <= bound))
        worst = float((d / bound).max())
    msg = ["old log-probs: %d elements outside, first %s: got %r, want %r, bound %r" % (
        len(bad), tuple(bad[0]), float(got[tuple(bad[0])]), float(lp[tuple(bad[0])]), float(bound[tuple(bad[0])]))] \
        if len(bad) else []
    return msg, worst


# ------------------------------------------------------------------ a whole export
def check_links(params, H, A, bf16, stacks, exp, logits, values, f16=False, samples=None, cache=None):
    """every link of one acting forward: exp = aleppo_export_acting's dict ("conv1" / "conv2" where stored, "conv3",
    "fc_parts"), logits [n, A] / values [n] the slot's planes, stacks the slot's bytes [n, 4, 84, 84].  samples: the conv
    links on these samples only (the slices, the hidden vector and the head always on all).  Returns (failures, report
    {link: text}, numbers {link: ...})"""
    p = lr.split_params(params, H, A, bf16)
    failures, report, numbers = [], {}, {}
    pick = slice(None) if samples is None else np.asarray(samples)
    acts = {l: np.ascontiguousarray(exp[l][pick]) for l in CONVS if l in exp}
    layers = tuple(l for l in CONVS if l in acts and (l == "conv1" or lr.INPUT_OF[l] in acts))
    if layers:
        bad, rep, res = lr.check_export(params, H, A, bf16, np.ascontiguousarray(stacks[pick]), acts, layers=layers,
                                        cache=cache)
        failures += bad
        report.update(rep)
        numbers.update(res)
    refs = slice_refs(exp["conv3"], p["fc"][0])
    bad, worst, ratios = check_slices(refs, exp["fc_parts"])
    failures += bad
    report["slices"] = "(c) worst |d| / bound %.3g; max |d| / (u Sa) against R per slice: %s" % (
        worst, " ".join("%.2f/%.2f" % r for r in ratios))
    numbers["slices"] = worst
    h = hidden(p["fc"][1], exp["fc_parts"])
    ref = head_ref(h, *p["heads"])
    bad, worst = check_head(ref, head_got(logits, values), f16)
    failures += bad
    report["head"] = ("f16 interval: single-valued share %.3f" if f16 else "(c) worst |d| / bound %.3g") % worst
    numbers["head"] = worst
    return failures, report, numbers
