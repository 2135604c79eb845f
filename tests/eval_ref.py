"""numpy restatement of the evaluation lanes' action rules and built-in generator (include/aleppo.h, aleppo_eval_act).

The rules take the ENGINE's fp32 logits (read with aleppo_eval_read), so no forward tolerance enters:
  greedy(z)                 the lowest index of the maximum
  epsilon_greedy(z, eps, uw)  u < eps ? min((int)(w * A), A - 1), w * A rounded once in fp32 : greedy
  sample(z, tau, q)         float64: e = exp((z - max z) * inv), inv = fp32(1 / tau); p = e / sum e; argmax p / q, and the
                            relative gap between the two largest p / q (the test skips a lane only when it is < 1e-5)
philox4x32_10 / philox_noise restate the generator under any key, counter words {n lo, n hi, lane, block}; eval_noise is the
lanes' stream, key = seed ^ 0x4556414C4C414E45 (aleppo_act's key is the seed itself: tests/acting_ref.py).
"""
import numpy as np

SAMPLE_GAP = 1e-5  # a few ulp of expf and the divide: below it the fp32 kernel may legitimately pick the other action
EVAL_KEY_DOMAIN = 0x4556414C4C414E45


def greedy(z):
    return np.argmax(np.asarray(z), axis=1).astype(np.int64)  # (numpy: the first maximum)


def epsilon_greedy(z, eps, uw):
    z, uw = np.asarray(z, np.float32), np.asarray(uw, np.float32)
    A = z.shape[1]
    explore = uw[:, 0] < np.float32(eps)
    rnd = np.minimum((uw[:, 1] * np.float32(A)).astype(np.float32).astype(np.int64), A - 1)
    return np.where(explore, rnd, greedy(z)).astype(np.int64)


def sample(z, tau, q):
    """(actions, relative gap between the largest and second largest p / q) in float64"""
    z, q = np.asarray(z, np.float32).astype(np.float64), np.asarray(q, np.float32).astype(np.float64)
    inv = np.float64(np.float32(1.0) / np.float32(tau))
    e = np.exp((z - z.max(axis=1, keepdims=True)) * inv)
    r = e / e.sum(axis=1, keepdims=True) / q
    a = np.argmax(r, axis=1).astype(np.int64)
    if r.shape[1] == 1:
        return a, np.full(r.shape[0], np.inf)
    s = np.sort(r, axis=1)
    return a, (s[:, -1] - s[:, -2]) / s[:, -1]


def philox4x32_10(c, k0, k1):
    """c: uint32 [n, 4] counters -> uint32 [n, 4] (the block function of kernels.hip)"""
    c = [np.asarray(c[:, i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0, n2 = (p1 >> np.uint64(32)) ^ c[1] ^ k0, (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & m32, p1 & m32, n2 & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def _unit(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def philox_noise(key, n, L, A, rule):
    """the built-in draws of call n under the 64-bit key: rule "sample" -> Exp(1) q float32 [L, A] (up to logf's last bits:
    numpy's float32 log), rule "epsilon" -> uniforms (u, w) float32 [L, 2] (exact)"""
    key &= 0xFFFFFFFFFFFFFFFF
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    nb = (A + 3) // 4 if rule == "sample" else 1
    lane, blk = np.meshgrid(np.arange(L, dtype=np.uint32), np.arange(nb, dtype=np.uint32), indexing="ij")
    c = np.stack([np.full(L * nb, n & 0xFFFFFFFF, np.uint32), np.full(L * nb, n >> 32, np.uint32), lane.ravel(),
                  blk.ravel()], 1)
    w = philox4x32_10(c, k0, k1).reshape(L, nb * 4)
    if rule == "sample":
        return (-np.log(_unit(w[:, :A]))).astype(np.float32)
    return _unit(w[:, :2])


def eval_noise(seed, n, L, A, rule):
    """the built-in draws of evaluation call n: philox_noise under the lanes' key"""
    return philox_noise(seed ^ EVAL_KEY_DOMAIN, n, L, A, rule)
