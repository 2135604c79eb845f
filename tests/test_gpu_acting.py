"""The acting path link by link, its sampler and its noise stream (pytest -m gpu).

aleppo_export_acting gives what the rollout's last acting forward left: a3, the seven split-K slices of fc and - where the
route stored them, which ALEPPO_OPT_ACT_STORE makes the fused bf16 launch do - a1 and a2.  tests/acting_ref.py evaluates each
link on the engine's OWN previous link (its docstring has every bound): the conv links by layer_ref's (a) and (b) (bf16) or
(c) (fp32), every fc slice by (c) at K = 448, the hidden vector restated exactly, the head by (c) at K = H (an interval on
f16 planes), the sampler on the engine's own fp32 logits under eval_ref's gap rule, exact ties by construction, the built-in
generator against the Philox restatement at the acting counter that include/aleppo.h documents, and oldlp_kernel's plane
against the float64 log-softmax of the stored logits plane.

Routes of the (37, 96, 6) row, settled by reading act_forward and step_enqueue in api_rollout.hip (host frames): the generic
convolutions run the same three launches whatever ALEPPO_OPT_FUSED_ACT and the frame kind are; the patch route runs
act_conv_kernel<0> for (84x84, fused 0) and (raw pair, fused 0 / 1), <1> for (84x84, fused 1 / 2) and <2> for (raw pair,
fused 2).  Routes that run the same launches on the same stacks (the two frame kinds leave different ones) must export the
same bits: per kind the three generic routes, (84x84, fused 1) = (84x84, fused 2) and (raw pair, fused 0) = (raw pair,
fused 1).  The storing and the production instantiation must
agree bit for bit in conv3, every slice, logits, values and actions on all samples of every row.

Measured on the MI355X (256 CUs: the rows at CUs + 1 and 2 CUs + 1 are 257 and 513), each number against the float64
reference and the float32 evaluations' floors, none against the engine:
    (a) no element outside its interval and no gate off the exact one on any bf16 row or route; 56 .. 100 % of the intervals
        are a single value (n = 1), 69 .. 91 % on the larger rows.
    (b) worst channel's mismatch count / cap (the float32 evaluations' own worst count in brackets)
                                   conv1        conv2       conv3
        E = 1,   H = 32            0/8   (0)    0/8  (0)    0/8  (0)
        E = 37,  H = 96, 12 routes 2/12  (3)    1/8  (1)    1/8  (1)
        E = 257, H = 128           9/44  (11)   3/16 (4)    3/16 (4)
        E = 513, H = 32, 4 samples 0/8   (1)    1/8  (0)    0/8  (1)
    (c) worst |d| / bound             conv1  conv2  conv3  slices  head
        bf16 E = 1, H = 32, A = 1                          0.22    0.61
        bf16 E = 37, 12 routes                             0.32    0.32
        bf16 E = 257, H = 128, A = 18                      0.23    0.06
        bf16 E = 513, H = 32, A = 4                        0.24    0.23
        fp32 E = 37, H = 96, A = 18   0.21   0.30   0.40   0.25    0.11
        fp32 E = 260, H = 64, A = 4   0.20   0.25   0.42   0.29    0.22
        the head rows (E = 1 / 37, H = 32 / 96 / 512, A = 1 / 4 / 5 / 18): slices 0.22 .. 0.29 at E = 37 and up to 0.79 (fp32,
        H = 96) and 0.67 (fp32, H = 512) at E = 1, where the floor R is taken from H numbers only; head 0.04 .. 0.26 on fp32
        planes and 0.61 at E = 1, H = 32, A = 1 (two numbers); on f16 planes every value inside its interval, 95 .. 100 % of
        the intervals a single binary16 value.
    Storing and production runs: identical bits in conv3, every slice, logits, values and actions on every row and route;
    routes that run the same launches on the same stacks: identical bits, conv1 and conv2 included.
    Sampler: 0 of 203 draws left out on each of the 12 rows, no mismatch; per-row spreads 1.6 .. 6.5 (near-uniform), 17 .. 45
    (peaked, smallest p 3e-20), 46 .. 120 (underflow, smallest p 7e-53).  Exact ties and +inf quotients: the lowest lane on
    every row, through the head and through aleppo_sample.
    Noise stream: no mismatch at the documented counter in any of the three ways to drive a rollout; left out 1 of 5130
    (seed 123, E = 513, A = 18), 0 of 370 and 0 of 2570.
    Old log-probs: worst |d| / bound 0.07 (A = 4) .. 0.03 (A = 18) on fp32 planes; on f16 planes every value inside its
    interval, 72 .. 99 % of them a single binary16 value.
No kernel fault was found.  The whole file takes five seconds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (asked for its device before the library is loaded: the other order leaves torch without a GPU)

import acting_ref as ar
import eval_ref as er
import layer_ref as lr
from shared_fixtures import pkg  # noqa: F401

pytestmark = pytest.mark.gpu


CUS = int(torch.cuda.get_device_properties(0).multi_processor_count) if torch.cuda.is_available() else 0


def cus():
    assert CUS > 0
    return CUS


def _E(e):
    """a row's environment count: an int, or (k, d) for k * CUs + d"""
    return e if isinstance(e, int) else e[0] * cus() + e[1]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _engine(pkg, E, T, H, A, prec, f16=False, seed=42, opts=()):
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=seed,
                     rollout_precision=pkg.ROLLOUT_FP16 if f16 else pkg.ROLLOUT_FP32)
    for opt, val in opts:
        eng.set_option(opt, val)
        assert eng.get_option(opt) == val
    return eng


def _zeros(E):
    return np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.uint8)


def acting_run(pkg, E, H, A, prec, raw=False, fused=1, generic=0, store=0, f16=False, steps=3, params=None, seed=0):
    """`steps` protocol steps, the act on the stacks they leave, the export, then the rollout's end: dict(exp, stored, logits
    [E, A], values [E], actions [E] of that slot, obs the slot's bytes)"""
    frames, starts, stacks = ar.protocol(5000 + seed + E, E, raw, steps)
    params = ar.row_params(E, H, A) if params is None else params
    T = steps + 1
    eng = _engine(pkg, E, T, H, A, prec, f16, opts=((pkg.OPT_FUSED_ACT, fused), (pkg.OPT_GENERIC_CONV, generic),
                                                   (pkg.OPT_ACT_STORE, store)))
    eng.load_params(params)
    eng.set_gray_lut(ar.LUT)
    noise = ar.exp1(5100 + E + A, (T + 1, E, A))
    rew, te, tr = _zeros(E)
    kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
    for t in range(steps):
        eng.act(noise[t])
        eng.step(frames[t], rew, te, tr, starts[t], kind=kind)
    eng.act(noise[steps])
    exp, n, stored = eng.export_acting()
    assert n == E
    eng.step(frames[0], rew, te, tr, te, kind=kind)
    eng.finish_rollout(noise[T])
    out = dict(exp=exp, stored=stored, logits=eng.read_batch("logits")[:, steps], values=eng.read_batch("values")[:, steps],
               actions=eng.read_batch("actions")[:, steps], obs=eng.read_batch("observations")[:, steps],
               noise=noise[steps], params=params)
    eng.close()
    np.testing.assert_array_equal(out["obs"], stacks)  # the real protocol left the stacks the restatement gives
    return out


SAME = ("conv3", "fc_parts", "logits", "values", "actions")


def _assert_same(a, b, keys, what):
    for k in keys:
        x, y = (a["exp"][k], b["exp"][k]) if k in ("conv1", "conv2", "conv3", "fc_parts") else (a[k], b[k])
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


def _check(run, H, A, prec, f16=False, samples=None, cache=None, title=""):
    bf16 = prec == "bf16"
    failures, report, numbers = ar.check_links(run["params"], H, A, bf16, run["obs"], run["exp"], run["logits"],
                                                run["values"], f16, samples, cache)
    print(lr.summary("ACTSTAT %s:" % title, report))
    if bf16:
        for l in ar.CONVS:
            if l in run["exp"]:
                assert not (_bits(run["exp"][l]) & 0xFFFF).any() and run["exp"][l].min() >= 0, l
    return failures, numbers


# ------------------------------------------------------------------ the conv chain
# (E, H, A, precision, [(frame kind raw?, OPT_FUSED_ACT, OPT_GENERIC_CONV)], samples of the conv links)
ONE = ((False, 1, 0),)
ALL_ROUTES = tuple((raw, fused, generic) for generic in (0, 1) for raw in (False, True) for fused in (0, 1, 2))
CHAIN_ROWS = [
    (1, 32, 1, "bf16", ONE, None),
    (37, 96, 6, "bf16", ALL_ROUTES, None),
    ((1, 1), 128, 18, "bf16", ONE, None),    # CUs + 1: one workgroup takes a second sample (the loop body)
    ((2, 1), 32, 4, "bf16", ONE, "corners"),  # 2 CUs + 1: a third sample; the links on samples 0, CUs, 2 CUs and the last
    (37, 96, 18, "fp32", ONE, None),
    ((1, 4), 64, 4, "fp32", ONE, None),
]


def _cid(r):
    e = r[0] if isinstance(r[0], int) else "%dCU+%d" % r[0]
    return "E%s-H%d-A%d-%s" % (e, r[1], r[2], r[3])


def _launches(route, prec):
    """which launches a route's acting forward runs (api_rollout.hip, host frames)"""
    raw, fused, generic = route
    if generic or prec == "fp32":
        return "three launches"
    if not raw:
        return "act_conv_kernel<1>" if fused else "act_conv_kernel<0>"
    return "act_conv_kernel<2>" if fused == 2 else "act_conv_kernel<0>"


@pytest.mark.parametrize("row", CHAIN_ROWS, ids=[_cid(r) for r in CHAIN_ROWS])
def test_every_link_of_the_acting_forward_on_the_engines_own_previous_link(pkg, row):
    e, H, A, prec, routes, corners = row
    E = _E(e)
    samples = None if corners is None else sorted({0, cus(), 2 * cus(), E - 1})
    failures, cache, by_launch = [], {}, {}
    for route in routes:
        raw, fused, generic = route
        stored = acting_run(pkg, E, H, A, prec, raw, fused, generic, store=1)
        plain = acting_run(pkg, E, H, A, prec, raw, fused, generic, store=0)
        title = "%s %s" % (_cid(row), route)
        assert stored["stored"] == 15, title  # a1 and a2 are there: the storing instantiation, or a route that stores anyway
        patch = prec == "bf16" and not generic
        assert plain["stored"] == (12 if patch else 15), title
        assert ("conv1" in plain["exp"]) == (not patch)
        _assert_same(stored, plain, SAME, title)  # the storing run changes no bit of what the production run computes
        bad, _ = _check(stored, H, A, prec, samples=samples, cache=cache, title=title)
        failures += ["%s: %s" % (title, f) for f in bad]
        first = by_launch.setdefault((_launches(route, prec), raw), (title, stored))  # (per frame kind: other stacks)
        _assert_same(first[1], stored, SAME + ("conv1", "conv2"), (first[0], title))  # the same launches: the same bits
    assert not failures, failures


# ------------------------------------------------------------------ fc slices and the head at every H, both plane types
# (E, H, A, precision, f16 planes): E = 1 and 37 leave the fc kernels a ragged 32-row tile, and 37 = 9 * 4 + 1 gives the head a
# last workgroup with one live wave; H = 32 / 96 / 512 are one, three and sixteen 32-column tiles and 4 .. 64 live lanes of
# head_dot; A on both sides of the Philox block and with the value lane at 1, 4, 5 and 18
HEAD_ROWS = [(1, 32, 1, "bf16", False), (1, 96, 4, "fp32", True), (1, 512, 5, "bf16", True), (1, 512, 18, "fp32", False),
             (37, 32, 18, "bf16", True), (37, 32, 5, "fp32", False), (37, 96, 5, "bf16", False), (37, 96, 1, "fp32", True),
             (37, 512, 4, "bf16", True), (37, 512, 18, "fp32", False), (37, 512, 1, "bf16", False), (37, 96, 18, "bf16", True)]


@pytest.mark.parametrize("row", HEAD_ROWS, ids=["E%d-H%d-A%d-%s-%s" % (r[:4] + ("f16" if r[4] else "f32",)) for r in HEAD_ROWS])
def test_fc_slices_hidden_vector_and_head(pkg, row):
    E, H, A, prec, f16 = row
    run = acting_run(pkg, E, H, A, prec, f16=f16, steps=1, seed=7)
    assert run["exp"]["fc_parts"].shape == (pkg.FC_SPLITS, E, H)
    failures, _ = _check(run, H, A, prec, f16, title="head E%d H%d A%d %s %s" % (E, H, A, prec, "f16" if f16 else "f32"))
    assert not failures, failures


# ------------------------------------------------------------------ the sampler and the old log-probs
SAMPLER_E, SAMPLER_H = 203, 32
SAMPLER_ROWS = [(A, regime) for regime in ar.REGIMES for A in (1, 4, 6, 18)]


@functools.lru_cache(maxsize=None)
def _sampler_run(A, regime, f16):
    """two slots with caller noise on a sampler row's parameters, then finish_rollout: the planes [E, T, ...]"""
    import __graft_entry__ as g
    p = g.load_package()
    E, H, T = SAMPLER_E, SAMPLER_H, 2
    params, frames, starts, _ = ar.sampler_case(E, H, A, regime)
    eng = _engine(p, E, T, H, A, "bf16", f16)
    eng.load_params(params)
    noise = ar.exp1(6300 + A, (T + 1, E, A))
    rew, te, tr = _zeros(E)
    for t in range(T):
        eng.act(noise[t])
        eng.step(frames[0], rew, te, tr, starts[0] if t == 0 else te)
    eng.finish_rollout(noise[T])
    out = {k: eng.read_batch(k) for k in ("logits", "actions", "log_probs")}
    eng.close()
    out["noise"] = noise
    return out


@pytest.mark.parametrize("A,regime", SAMPLER_ROWS, ids=["A%d-%s" % r for r in SAMPLER_ROWS])
def test_sampler_on_the_engines_own_logits(A, regime, pkg):
    b = _sampler_run(A, regime, False)
    t = 1  # the slot that acts on the pushed frames
    logits, actions = b["logits"][:, t], b["actions"][:, t]
    wrong, left_out, want = ar.sample_check(logits, b["noise"][t], actions)
    spread = logits.max(axis=1) - logits.min(axis=1)
    p_min = np.exp(ar.oldlp_ref(logits)[0]).min()
    print("ACTSTAT sampler A%d %s: spread %.3g .. %.3g, smallest p %.3g, left out %.4f, actions seen %d" % (
        A, regime, spread.min(), spread.max(), p_min, left_out, len(set(actions.tolist()))))
    assert not len(wrong), (wrong[:8], actions[wrong[:8]], want[wrong[:8]])
    assert left_out <= ar.LEFT_OUT_CAP
    if A > 1 and regime == "uniform":
        assert len(set(actions.tolist())) > 1
    if A > 1 and regime == "peaked":
        assert 40 <= spread.max() <= 50 and (spread >= 20).mean() >= 0.9
    if A > 1 and regime == "underflow":
        assert 110 <= spread.max() <= 130 and (np.exp(ar.oldlp_ref(logits)[0]).min(axis=1) < ar.TINY).mean() >= 0.15


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("A,regime", SAMPLER_ROWS, ids=["A%d-%s" % r for r in SAMPLER_ROWS])
def test_old_log_probs_from_the_stored_logits_plane(A, regime, f16, pkg):
    b = _sampler_run(A, regime, f16)
    failures, worst = ar.check_oldlp(b["logits"], b["log_probs"], f16)
    print("ACTSTAT oldlp A%d %s %s: %s %.3g" % (A, regime, "f16" if f16 else "f32",
                                               "single-valued share" if f16 else "worst |d| / bound", worst))
    assert not failures, failures


# ------------------------------------------------------------------ exact ties
@pytest.mark.parametrize("A", [1, 4, 6, 18])
def test_exact_ties_take_the_lowest_lane(pkg, A):
    import hashfill as hf
    import oracle_lib as orc
    bias, probs, q, expected = ar.tie_cases(A)
    E, H = len(expected), 32
    params = np.array(hf.fill_params(6400 + A, H, A))
    offs = orc.param_offsets(H, A)
    params[offs[8]:offs[9]] = 0       # zero action-head weights: the logits are the biases exactly
    params[offs[9]:offs[10]] = bias
    frames, starts, _ = ar.protocol(6500 + A, E, False, 1)
    eng = _engine(pkg, E, 2, H, A, "bf16")
    eng.load_params(params)
    rew, te, tr = _zeros(E)
    eng.act(np.ones((E, A), np.float32))
    eng.step(frames[0], rew, te, tr, starts[0])
    got = eng.act(q).copy()
    eng.step(frames[0], rew, te, tr, te)
    eng.finish_rollout(np.ones((E, A), np.float32))
    logits = eng.read_batch("logits")[:, 1]
    eng.close()
    assert np.array_equal(_bits(logits), _bits(np.broadcast_to(bias, (E, A))))
    np.testing.assert_array_equal(got, expected)
    np.testing.assert_array_equal(pkg.sampling.multinomial_with_noise(probs, q), expected)  # aleppo_sample: probs_in, zeros
    np.testing.assert_array_equal(ar.sample_f32(probs, q), expected)


# ------------------------------------------------------------------ the noise stream
STREAM_ROWS = [(123, (2, 1), 18), (123, 37, 6), (0xDEADBEEF12345678, (1, 1), 1)]
STREAM_T = 5


def _mapped(eng, nbytes):
    addr = eng.host_alloc(nbytes)
    return addr, np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(addr))


def _stream_run(pkg, seed, E, A, mode):
    """two rollouts of STREAM_T slots on a zero network with the built-in generator; the first rollout's finish_rollout
    takes caller noise (a call in between that draws nothing and still advances the counter), and in the act / step and
    arm / release modes so does slot 2 of each rollout.  Returns [(actions [T, E], caller-noise slots)]"""
    H, T = 32, STREAM_T
    eng = _engine(pkg, E, T, H, A, "bf16", seed=seed)
    eng.load_params(np.zeros(eng.param_count, np.float32))
    frames = np.zeros((T, E, 7056), np.uint8)
    rew, te, tr = _zeros(E)
    caller = ar.exp1(6600 + A, (E, A))
    out = []
    if mode != "act/step":
        f_addr, f_map = _mapped(eng, frames.nbytes if mode == "replay" else E * 7056)
        s_addr, s_map = _mapped(eng, E)
        f_map[:], s_map[:] = 0, 0
    for r in range(2):
        if mode == "replay":
            z = np.zeros((T, E), np.uint8)
            eng.replay_rollout(f_addr, pkg.FRAMES_84, E * 7056, np.zeros((T, E), np.float32), z, z, z, noise=None,
                               location=pkg.HOST_MAPPED)
            given = ()
        elif mode == "act/step":
            for t in range(T):
                eng.act(caller if t == 2 else None)
                eng.step(frames[t], rew, te, tr, te)
            given = (2,)
        else:
            eng.act()
            for t in range(T):
                eng.arm_step(f_addr, s_addr, noise_next=caller if t + 1 == 2 else None)
                eng.release_step(rew, te, tr)
                if t + 1 < T:
                    eng.act()
            given = (2,)
        eng.finish_rollout(caller if r == 0 else None)
        out.append((eng.read_batch("actions").T.copy(), given))
    if mode != "act/step":
        eng.synchronize()
        eng.host_free(f_addr), eng.host_free(s_addr)
    eng.close()
    return out, caller


@pytest.mark.parametrize("mode", ["act/step", "replay", "arm/release"])
@pytest.mark.parametrize("seed,e,A", STREAM_ROWS, ids=["seed%x-E%s-A%d" % (s, e if isinstance(e, int) else "%dCU+%d" % e, a)
                                                       for s, e, a in STREAM_ROWS])
def test_builtin_noise_stream_at_the_documented_counter(pkg, seed, e, A, mode):
    E, T = _E(e), STREAM_T
    rollouts, caller = _stream_run(pkg, seed, E, A, mode)
    z = np.zeros((E, A), np.float32)
    total = left = 0
    other_differs = False
    for r, (actions, given) in enumerate(rollouts):
        for t in range(T):
            n = r * (T + 1) + t  # every acting head advances the counter, finish_rollout's (n = r (T + 1) + T) included
            q = caller if t in given else ar.act_noise(seed, n, E, A)
            wrong, share, want = ar.sample_check(z, q, actions[t])
            assert not len(wrong), (r, t, wrong[:8])
            total += E
            left += int(round(share * E))
            other_differs |= bool((er.sample(z, 1.0, ar.act_noise(seed + 1, n, E, A))[0] != actions[t]).any())
    print("ACTSTAT stream seed %x E%d A%d %s: %d of %d draws within the gap" % (seed, E, A, mode, left, total))
    assert left <= ar.LEFT_OUT_CAP * total
    assert other_differs or A == 1  # another seed is another stream


# ------------------------------------------------------------------ the export hook's refusals
def test_export_acting_refusals_and_the_precomputed_slot(pkg):
    import hashfill as hf
    E, T, H, A = 8, 4, 32, 4
    lib, RUN, INV = pkg.lib(), pkg.ERR_RUNTIME, pkg.ERR_INVALID_ARGUMENT
    eng = _engine(pkg, E, T, H, A, "bf16", opts=((pkg.OPT_ACT_STORE, 1),))
    eng.load_params(ar.row_params(E, H, A))
    frames, starts, _ = ar.protocol(6700, E, False, 3)
    rew, te, tr = _zeros(E)
    buf = {k: np.full(s, -7, np.float32) for k, s in (("conv1", (E, 32, 20, 20)), ("conv2", (E, 64, 9, 9)),
                                                      ("conv3", (E, 64, 7, 7)), ("fc_parts", (7, E, H)))}

    def raw(cap=E, outputs=True):
        n, stored = C.c_int64(-1), C.c_uint32(99)
        ptrs = [buf[k].ctypes.data_as(C.c_void_p) if outputs else None for k in ("conv1", "conv2", "conv3", "fc_parts")]
        rc = lib.aleppo_export_acting(eng._ctx, C.c_int64(cap), *ptrs, C.byref(n), C.byref(stored))
        return rc, n.value, stored.value

    def untouched():
        return all((a == -7).all() for a in buf.values())

    assert raw() == (RUN, -1, 99) and untouched()  # before any act
    eng.act()
    assert raw(cap=E - 1) == (INV, -1, 99) and untouched()  # a wrong capacity
    assert raw(outputs=False)[0] == INV
    assert raw() == (pkg.OK, E, 15) and not untouched()
    first = {k: a.copy() for k, a in buf.items()}
    eng.step(frames[0], rew, te, tr, starts[0])  # fused ingest: the coming slot's forward is pre-computed ...
    between, _, _ = eng.export_acting()
    eng.act()
    after, _, _ = eng.export_acting()
    for k in between:  # ... and an export between step and act returns it
        assert np.array_equal(_bits(between[k]), _bits(after[k])), k
    assert not np.array_equal(between["conv3"], first["conv3"])
    eng.step(frames[1], rew, te, tr, starts[1])
    obs = hf.hf_bytes(6710, (E, 4, 84, 84))
    for name, call in (("forward", lambda: eng.forward(obs)), ("load_params", lambda: eng.load_params(ar.row_params(E, H, A))),
                       ("activation_stats", lambda: eng.activation_stats(obs))):
        eng.act()
        assert raw()[0] == pkg.OK
        for a in buf.values():
            a[...] = -7
        call()
        assert raw() == (RUN, -1, 99) and untouched(), name
        eng.step(frames[2], rew, te, tr, te) if name == "forward" else None
    # while armed
    eng.act()  # (slot 3; the rollout has one slot left)
    f_addr, s_addr = eng.host_alloc(E * 7056), eng.host_alloc(E)
    C.memset(f_addr, 0, E * 7056), C.memset(s_addr, 0, E)
    eng.arm_step(f_addr, s_addr)
    assert raw() == (RUN, -1, 99) and untouched()
    with pytest.raises(pkg.AleppoError):
        eng.set_option(pkg.OPT_ACT_STORE, 0)
    eng.release_step(rew, te, tr)
    assert raw()[0] == pkg.OK
    eng.finish_rollout()
    assert raw()[0] == pkg.OK  # the bootstrap forward
    eng.train(2.5e-4, 1, 1)
    for a in buf.values():
        a[...] = -7
    assert raw() == (RUN, -1, 99) and untouched()  # after an update
    for t in range(T):  # a second rollout: a refresh is valid between its finish_rollout and the next act
        eng.act()
        assert raw()[0] == pkg.OK
        eng.step(frames[t % 3], rew, te, tr, te)
    eng.finish_rollout()
    assert raw()[0] == pkg.OK
    eng.refresh_advantages()
    for a in buf.values():
        a[...] = -7
    assert raw() == (RUN, -1, 99) and untouched()  # after a refresh
    eng.synchronize()
    eng.host_free(f_addr), eng.host_free(s_addr)
    eng.close()
