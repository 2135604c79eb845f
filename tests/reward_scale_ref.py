"""Reference of ALEPPO_OPT_REWARD_SCALE (include/aleppo.h): the definition in numpy float64 - the per-environment running
discounted return, the two-pass moments (np.mean, np.var) of one rollout's samples, gym's / SB3's RunningMeanStd merge and
the scale - and the bounds a one-pass double-precision reduction is held to.

The bounds are derived, not tuned, the way tests/batch_stats_ref.py derives its own.  The samples themselves carry no
error: G * gamma + r is two rounded double operations on both sides, so the device's samples are the reference's bits.
What differs is the batch moments: the device sums n, S and Q once, in its own order.  A double sum of n terms carries at
most n * 2^-53 relative error on sums of one sign, and var_b = Q / n - mean_b^2 amplifies it by 1 + mean_b^2 / var_b.  So
    rel_b = 8 * n * 2^-53 * (1 + mean_b^2 / var_b)
bounds the batch variance relatively (d_var_b = rel_b * var_b) and the batch mean by d_mean_b = rel_b * max(|mean_b|,
std_b).  Through the merge (count_new = count + n exactly: the same double addition on both sides)
    mean_new = (mean * count + mean_b * n) / tot
    var_new  = (var * count + var_b * n + d^2 * count * n / tot) / tot,   d = mean_b - mean
the absolute bounds (bm, bv) of the running mean and variance, which start at (0, 0), propagate as
    dd     = d_mean_b + bm
    bm_new = bm * count / tot + d_mean_b * n / tot + ULPS * |mean_new|
    bv_new = bv * count / tot + d_var_b * n / tot + (2 |d| dd + dd^2) * count * n / tot^2 + ULPS * var_new
with ULPS = 8 * 2^-53 for the merge's own dozen roundings.  Every test asserts that a bound, taken relatively (bv / var,
bm / max(|mean|, std)), is <= MAX_BOUND before it uses it, so that a bound cannot grow until it hides a fault.  The scale
s = (float)(1 / sqrt(var + 1e-8)) is held to one ulp of the reference's float (a relative error of 1e-10 in var moves 1 / sqrt by 5e-11, far below half a float ulp, so at most the
rounding can flip), and the scaled reward plane to EXACT equality with clip(r * s_engine, -c, c) computed in numpy
float32 from the s the engine reports - a one-ulp difference in s cannot hide a wrong multiply or clip."""
import numpy as np

NAMES = ("count", "mean", "var", "scale", "batch_count", "clipped")
MAX_BOUND = 1e-6
INITIAL = (1e-4, 0.0, 1.0)
EPS = 1e-8
ULPS = 8.0 * 2.0 ** -53


def scan(rewards, terminals, truncations, starts, G, gamma):
    """time-major [T][E] records -> (x [T][E] float64 the running return after each slot, live [T][E] bool which of them
    are samples, G after).  gamma is the float the engine was configured with, widened."""
    r = np.asarray(rewards, np.float32)
    te, tr, st = (np.asarray(a) != 0 for a in (terminals, truncations, starts))
    g = float(np.float32(gamma))
    G = np.array(G, np.float64).copy()
    T, E = r.shape
    x = np.zeros((T, E))
    live = ~st
    for t in range(T):
        G = np.where(live[t], G * g + r[t].astype(np.float64), G)
        x[t] = G
        G = np.where(live[t] & (te[t] | tr[t]), 0.0, G)
    return x, live, G


def merge(state, mean_b, var_b, n):
    """RunningMeanStd.update_from_moments, left to right as aleppo.h writes it"""
    count, mean, var = state
    if n == 0:
        return (count, mean, var)
    d = mean_b - mean
    tot = count + n
    return (tot, mean + d * n / tot, (var * count + var_b * n + d * d * count * n / tot) / tot)


def scale_of(var):
    return np.float32(1.0 / np.sqrt(var + EPS))


class Reference:
    """the running state of one rank (or of the concatenated environments of all ranks) and its error bounds"""

    def __init__(self, E, gamma, state=INITIAL, G=None):
        self.gamma = gamma
        self.state = tuple(float(v) for v in state)
        self.G = np.zeros(E) if G is None else np.array(G, np.float64)
        self.bm = self.bv = 0.0
        self.scale = np.float32(1.0)
        self.n = 0
        self.rel_b = 0.0

    def rollout(self, rewards, terminals, truncations, starts):
        """merge one rollout ([T][E] records); returns the samples (1-D, time-major order)"""
        x, live, self.G = scan(rewards, terminals, truncations, starts, self.G, self.gamma)
        xs = x[live]
        n = int(xs.size)
        self.n = n
        if n:
            mean_b, var_b = float(np.mean(xs)), float(np.var(xs))
            count, mean, _ = self.state
            new = merge(self.state, mean_b, var_b, n)
            tot = new[0]
            if var_b > 0.0:
                rel = 8.0 * n * 2.0 ** -53 * (1.0 + mean_b * mean_b / var_b)
            else:  # constant samples: exact when their sums are (the tests use such constants)
                rel = 0.0
            self.rel_b = rel
            d_mean = rel * max(abs(mean_b), np.sqrt(var_b))
            d_var = rel * var_b
            d = mean_b - mean
            dd = d_mean + self.bm
            self.bm = self.bm * count / tot + d_mean * n / tot + ULPS * abs(new[1])
            self.bv = (self.bv * count / tot + d_var * n / tot + (2.0 * abs(d) * dd + dd * dd) * count * n / (tot * tot)
                       + ULPS * new[2])
            self.state = new
        self.scale = scale_of(self.state[2])
        return xs

    def scaled(self, rewards, clip, s=None):
        """step 5 in numpy float32 with the given s (default: the reference's own)"""
        return scaled_rewards(rewards, self.scale if s is None else s, clip)


def scaled_rewards(rewards, s, clip):
    r = np.asarray(rewards, np.float32)
    c = np.float32(clip)
    p = r * np.float32(s)
    assert p.dtype == np.float32
    return np.minimum(np.maximum(p, -c), c), int((np.abs(p) > c).sum())


def one_pass_in_device_order(x, live):
    """(n, S, Q) the way the device sums them: every environment in slot order, 64 consecutive environments folded by xor
    butterflies, the groups of 64 added in index order.  x, live: [T][E]."""
    T, E = x.shape
    nb = (E + 63) // 64
    acc = np.zeros((3, nb * 64))
    for t in range(T):
        l = live[t]
        acc[0, :E] += np.where(l, 1.0, 0.0)
        acc[1, :E] += np.where(l, x[t], 0.0)
        acc[2, :E] += np.where(l, x[t] * x[t], 0.0)
    w = acc.reshape(3, nb, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., np.arange(64) ^ o]
    part = w[..., 0]
    sums = np.zeros(3)
    for b in range(nb):
        sums += part[:, b]
    return sums[0], sums[1], sums[2]


def state_from_sums(state, n, S, Q):
    """the device's finalising arithmetic (aleppo.h, steps 2-4) from one-pass sums"""
    if n > 0:
        mean_b = S / n
        var_b = max(0.0, Q / n - mean_b * mean_b)
        state = merge(state, mean_b, var_b, n)
    return state, scale_of(state[2])


def ulp_distance(a, b):
    """distance in float32 ulps between two positive finite floats"""
    ia = int(np.array(a, np.float32).view(np.uint32))
    ib = int(np.array(b, np.float32).view(np.uint32))
    return abs(ia - ib)


def assert_state(got, ref, what=""):
    """got: dict over NAMES (Engine.reward_scale()); ref: a Reference after the same rollouts.  Prints each figure first."""
    count, mean, var = ref.state
    rows = (("count", got["count"], count, 0.0), ("mean", got["mean"], mean, ref.bm), ("var", got["var"], var, ref.bv))
    for name, g, w, b in rows:
        print(f"{what} {name}: got {g!r} want {w!r} err {abs(g - w):.3e} bound {b:.3e}")
    print(f"{what} scale: got {got['scale']!r} want {float(ref.scale)!r} ulps {ulp_distance(got['scale'], ref.scale)}"
          f" rel_b {ref.rel_b:.3e}")
    unit = dict(count=count, mean=max(abs(mean), np.sqrt(var)), var=var)
    for name, g, w, b in rows:
        assert b / unit[name] <= MAX_BOUND, (what, name, b)
        assert abs(g - w) <= b, (what, name, g, w, b)
    assert got["scale"] == float(np.float32(got["scale"])), "the reported scale is not a float32"
    assert ulp_distance(got["scale"], ref.scale) <= 1, (what, got["scale"], float(ref.scale))
    assert got["batch_count"] == ref.n, (what, got["batch_count"], ref.n)


# ---------------------------------------------------------------------------- input generator of the tests
CLIP = 3.0  # the tests' c (see generate): finite, > 0, and small enough that the rare large rewards reach it


def generate(seed, E, T, start=None, p_term=0.02, p_trunc=0.01):
    """One rollout's records, time-major [T][E]: (rewards f32, terminals, truncations, starts u8, start flags for the next
    rollout).  Slot protocol of the rollout: a terminated / truncated slot is followed by one episode-start slot; start =
    the flags carried in from the previous rollout (None: every environment starts).  Rewards: the sparse 1-4 of the
    trainer's Breakout-like emulator (8 % of the slots), and about one slot in 1500 (at least four per rollout) pays a few
    hundred, of either sign.  Those dominate the return's variance (std of the order of 100), so with c = CLIP = 3 they are
    what the clip catches while the ordinary rewards (at most 4 / std) never reach it: the clipped share is above 0 and
    far below 1 %.  (The default c = 10 is mostly out of their reach too: R * s is about 1 / sqrt(50 p) for a share p of
    rewards R, 5 at p = 1 / 1500.)"""
    rng = np.random.default_rng(seed)
    te, tr, st = (np.zeros((T, E), np.uint8) for _ in range(3))
    start = np.ones(E, np.uint8) if start is None else np.asarray(start, np.uint8).copy()
    for t in range(T):
        u = rng.random(E)
        st[t] = start
        te[t] = (u < p_term) & (start == 0)
        tr[t] = (u >= p_term) & (u < p_term + p_trunc) & (start == 0)
        start = (te[t] | tr[t]).astype(np.uint8)
    r = ((rng.random((T, E)) < 0.08) * rng.integers(1, 5, (T, E))).astype(np.float32)
    nbig = max(4, (E * T) // 1500)
    live = np.flatnonzero(st.ravel() == 0)
    pos = rng.choice(live, size=nbig, replace=False)
    sign = np.where(rng.random(nbig) < 0.3, -1.0, 1.0).astype(np.float32)
    sign[:2] = (-1.0, 1.0)  # both ends of the clip in every rollout
    big = rng.integers(300, 800, nbig).astype(np.float32) * sign
    r.ravel()[pos] = big
    return r, te, tr, st, start
