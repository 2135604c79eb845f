"""numpy restatement of aleppo_state_digest (include/aleppo.h) on the EXPORTED state: what any host can recompute from
aleppo_export_params / _optimizer / _rollout_state / _reward_scale.  uint64 arithmetic wraps."""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x):
    """the function specified at aleppo_read_sample_order, on a uint64 array (or scalar)"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def D(tag, words):
    """sum_i splitmix64(splitmix64(tag) ^ (i << 32 | w_i)) mod 2^64 over a sequence of uint32 words"""
    w = np.ascontiguousarray(words, np.uint32).ravel().astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64) << np.uint64(32)
    with np.errstate(over="ignore"):
        return int(np.sum(splitmix64(splitmix64(np.uint64(tag)) ^ (i | w)), dtype=np.uint64))


def scalar_term(tag, value):
    return int(splitmix64(splitmix64(np.uint64(tag)) ^ np.uint64(int(value) & M64)))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)


def params(flat):
    return D(1, bits32(flat))


def optimizer(exp_avg, exp_avg_sq, step):
    return (D(2, bits32(exp_avg)) + D(3, bits32(exp_avg_sq)) + scalar_term(4, step)) & M64


def rollout(observations, counter):
    o = np.ascontiguousarray(observations, np.uint8).astype(np.uint32)  # [E,4,84,84]
    E = o.shape[0]
    o = o.reshape(E, 4, 84 * 84)
    s = o[:, 0] | (o[:, 1] << 8) | (o[:, 2] << 16) | (o[:, 3] << 24)  # [E, 7056]
    return (D(5, s) + scalar_term(6, counter)) & M64


def reward_scale(stats, returns):
    d = np.concatenate([np.asarray(stats, np.float64).ravel(), np.asarray(returns, np.float64).ravel()])
    return D(7, d.view("<u4"))  # each double as its low then its high word


def digest(run_state):
    """the four words from what Engine.run_state() returns"""
    sd = run_state
    return dict(params=params(sd["params"]),
                optimizer=optimizer(sd["exp_avg"], sd["exp_avg_sq"], int(sd["step"])),
                rollout=rollout(sd["rollout"]["observations"], sd["rollout"]["counter"]),
                reward_scale=reward_scale(sd["reward_scale"]["stats"], sd["reward_scale"]["returns"]))
