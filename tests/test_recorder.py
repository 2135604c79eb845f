"""GPU: the episode recorders (include/aleppo.h: aleppo_rec_open / aleppo_rec_count / aleppo_rec_read / aleppo_rec_clear)
through the C ABI, in the manner of tests/test_device_env.py: one context runs the device path with a recorder open, a
second one with the same seed and parameters the host loop through tests/device_env_ref.py.  Every recorded row is compared
with what the host loop saw in that step - the reference's frame and record, the host context's stack, logits, value and
action - and the recorded context's own planes, episode log, environment state and digest with the host context's.  There
are no tolerances: every comparison is of bytes.  Each case asserts from the REFERENCE's records that the branch it exists
for occurred."""
import ctypes as C

import numpy as np
import pytest

import device_env_ref as ref
import recorder_ref as rr
from __graft_entry__ import load_package
from test_device_env import LUT, Ctx, same
from test_eval_env import Lanes

pytestmark = pytest.mark.gpu
A, H = 4, 32


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def host_rollout(h, index):
    """Ctx.host_rollout that also keeps, per slot, the recorded environment's lives after the step"""
    h.slots, lives = [], []
    for _ in range(h.T):
        actions = h.eng.act().copy()
        o = h.envs.step(actions)
        h.eng.step(o.frames, o.rewards, o.term, o.trunc, o.start, kind=h.kind)
        h.slots.append(o)
        lives.append(h.envs.envs[index].lives)
    h.eng.finish_rollout()
    out = h.read()
    out["episodes"] = dict(zip("abcd", ref.compact(h.slots)))
    out["env_state"] = h.envs.state(h.pkg.ENV_STATE_DTYPE)
    return out, lives


def drain(eng, source):
    """every plane of the log, then clear"""
    n = eng.rec_count(source)
    out = dict(steps=eng.rec_read(source, "steps"), logits=eng.rec_read(source, "logits"))
    if n["frame_bytes"]:
        out["frames"] = eng.rec_read(source, "frames")
    if n["observation_bytes"]:
        out["observations"] = eng.rec_read(source, "observations")
    eng.rec_clear(source)
    return out


def check_rollout_rows(rows, rh, slots, lives, i, T, ordinal0, what):
    """rows: one rollout's drained log of environment i; rh / slots / lives: the host loop's planes and records"""
    st = rows["steps"]
    assert len(st) == T and st["ordinal"].tolist() == list(range(ordinal0, ordinal0 + T)), (what, st["ordinal"])
    assert not st["reserved"].any()
    for t in range(T):
        o, w = slots[t], f"{what} slot {t}"
        assert rows["frames"][t].tobytes() == o.frames[i].tobytes(), f"{w}: frame"
        newest = rh["observations"][i, t + 1, 0] if t + 1 < T else rh["current_obs"][i, 0]
        assert rows["observations"][t].tobytes() == newest.tobytes(), f"{w}: observation"
        assert rows["logits"][t].tobytes() == rh["logits"][i, t].tobytes(), f"{w}: logits"
        assert st["value"][t].tobytes() == rh["values"][i, t].tobytes(), f"{w}: value"
        assert int(st["action"][t]) == int(rh["actions"][i, t]), f"{w}: action"
        assert st["reward"][t].tobytes() == o.rewards[i].tobytes(), f"{w}: reward"
        got = (int(st["start"][t]), int(st["terminated"][t]), int(st["truncated"][t]), int(st["game_over"][t]), int(st["lives"][t]))
        want = (int(o.start[i]), int(o.term[i]), int(o.trunc[i]), int(o.game_over[i]), int(lives[t]))
        assert got == want, f"{w}: start / terminated / truncated / game_over / lives {got} != {want}"


def recorded_run(pkg, kw, index, rollouts, opts=()):
    """-> (all rows' steps, the reference's slots of all rollouts): a recorded device context against the host loop, and
    against an unrecorded device context after one update"""
    kw = dict(kw, opts=tuple(opts))
    d, h, u = Ctx(pkg, **kw), Ctx(pkg, device_env=False, **kw), Ctx(pkg, **kw)
    d.eng.rec_open("rollout", index=index)
    n = d.eng.rec_count("rollout")
    fb = 2 * 210 * 160 if kw.get("raw") else 7056
    assert n == dict(rows=0, dropped=0, next_ordinal=0, capacity=d.T, frame_bytes=fb, observation_bytes=7056, actions=A), n
    steps, slots = [], []
    for k in range(rollouts):
        rd = d.device_rollout()
        u.device_rollout()
        rh, lives = host_rollout(h, index)
        same(rh, rd, f"rollout {k}: the recorded context's own planes")
        n = d.eng.rec_count("rollout")
        assert (n["rows"], n["dropped"], n["next_ordinal"]) == (d.T, 0, (k + 1) * d.T), n
        rows = drain(d.eng, "rollout")
        check_rollout_rows(rows, rh, h.slots, lives, index, d.T, k * d.T, f"rollout {k}")
        if not kw.get("raw"):  # (an 84x84 frame IS the newest plane of the stack it is ingested into)
            assert rows["observations"].tobytes() == rows["frames"].tobytes()
        steps.append(rows["steps"])
        slots += h.slots
    d.eng.train(2.5e-4, 1, 2), u.eng.train(2.5e-4, 1, 2)
    assert d.eng.export_params().tobytes() == u.eng.export_params().tobytes()
    assert d.eng.state_digest() == u.eng.state_digest()
    d.close(), h.close(), u.close()
    return np.concatenate(steps), slots


VARIANTS = {
    "84-fp32": (dict(), ()),
    "raw-lut-bf16": (dict(prec="bf16", raw=True, lut=LUT), ()),
    "rollout-fp16": (dict(prec="bf16", rollout_fp16=True), ()),
    "fused-act-0": (dict(prec="bf16"), (("OPT_FUSED_ACT", 0),)),
    "fused-act-2": (dict(prec="bf16", raw=True, lut=LUT), (("OPT_FUSED_ACT", 2),)),
}


@pytest.mark.parametrize("index", [0, 2])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rollout_rows_across_truncations(pkg, variant, index):
    """max_steps = 40: ten agent steps per episode whatever the actions are, so every environment truncates in slots 10 and
    21 of the 24: two whole episodes, each across a rollout boundary (T = 8)"""
    kw, opts = VARIANTS[variant]
    opts = tuple((getattr(pkg, o), v) for o, v in opts)
    steps, slots = recorded_run(pkg, dict(E=3, T=8, max_steps=40, **kw), index, 3, opts)
    trunc = [t for t, o in enumerate(slots) if o.trunc[index]]
    assert trunc == [10, 21] and not any(o.term[index] for o in slots), trunc  # from the reference
    assert any(o.rewards[index] != 0 for o in slots)
    episodes, unfinished = rr.split_episodes(steps)
    assert episodes == [(0, 10, True), (11, 21, True)] and unfinished == 22, (episodes, unfinished)
    assert steps["game_over"][[10, 21]].tolist() == [1, 1] and steps["lives"][[10, 21]].tolist() == [0, 0]


def test_rollout_rows_across_a_life_loss(pkg):
    steps, slots = recorded_run(pkg, dict(E=3, T=16, max_steps=400), 1, 2)
    term = [t for t, o in enumerate(slots) if o.term[1]]
    assert term, "the reference saw no life loss in environment 1"  # from the reference
    assert steps["terminated"][term].all() and steps["start"][[t + 1 for t in term if t + 1 < len(steps)]].all()
    assert (steps["lives"][term] < 5).all() and (steps["lives"][term] > 0).all() and not steps["game_over"][term].any()


def test_capacity_drops_and_ordinals(pkg):
    kw = dict(E=3, T=8, max_steps=40)
    d, f = Ctx(pkg, **kw), Ctx(pkg, **kw)
    d.eng.rec_open("rollout", index=1, capacity=5)
    f.eng.rec_open("rollout", index=1)
    d.device_rollout(), f.device_rollout()
    n = d.eng.rec_count("rollout")
    assert (n["rows"], n["dropped"], n["next_ordinal"], n["capacity"]) == (5, 3, 8, 5), n
    with pytest.raises(pkg.AleppoInvalidArgument, match="out of range"):
        d.eng.rec_read("rollout", "steps", first=0, rows=6)
    full, got = drain(f.eng, "rollout"), drain(d.eng, "rollout")
    assert got["steps"]["ordinal"].tolist() == [0, 1, 2, 3, 4]
    for k in full:  # rows 0..4 are the first five steps
        assert got[k].tobytes() == full[k][:5].tobytes(), k
    assert d.eng.rec_count("rollout")["rows"] == 0 and d.eng.rec_count("rollout")["next_ordinal"] == 8
    d.device_rollout()
    n = d.eng.rec_count("rollout")
    assert (n["rows"], n["dropped"], n["next_ordinal"]) == (5, 3, 16), n
    assert drain(d.eng, "rollout")["steps"]["ordinal"].tolist() == [8, 9, 10, 11, 12]
    # a host-driven rollout: T more ordinals, no row
    d.envs.load_state(d.eng.env_state())
    d.host_rollout()
    d.eng.load_env_state(d.envs.state(pkg.ENV_STATE_DTYPE))
    n = d.eng.rec_count("rollout")
    assert (n["rows"], n["dropped"], n["next_ordinal"]) == (0, 0, 24), n
    d.device_rollout()
    assert drain(d.eng, "rollout")["steps"]["ordinal"].tolist() == [24, 25, 26, 27, 28]
    # the same config again: an empty log, ordinal 0
    d.device_rollout()
    d.eng.rec_open("rollout", index=1, capacity=5)
    n = d.eng.rec_count("rollout")
    assert (n["rows"], n["dropped"], n["next_ordinal"]) == (0, 0, 0), n
    d.close(), f.close()


# ------------------------------------------------------------------ the evaluation source
def eval_host_steps(h, n, lane, **rule):
    """the host loop eval_act -> reference -> eval_push_frames; per step what the recorder must have captured"""
    out = []
    for _ in range(n):
        actions = h.eng.eval_act(**rule).copy()
        logits, value = h.eng.eval_read("logits")[lane].copy(), h.eng.eval_read("values")[lane].copy()
        action = int(h.eng.eval_read("actions")[lane])
        assert action == int(actions[lane])
        o = h.envs.step(actions)
        h.eng.eval_push_frames(o.frames, o.start, kind=h.kind)
        out.append(dict(o=o, logits=logits, value=value, action=action, lives=h.envs.envs[lane].lives,
                        newest=h.eng.eval_read("observations")[lane, 0].copy()))
    return out


def check_eval_rows(rows, want, lane, ordinal0, what):
    st = rows["steps"]
    assert st["ordinal"].tolist() == list(range(ordinal0, ordinal0 + len(want))), (what, st["ordinal"])
    for s, w in enumerate(want):
        o, tag = w["o"], f"{what} step {s}"
        assert rows["frames"][s].tobytes() == o.frames[lane].tobytes(), f"{tag}: frame"
        assert rows["observations"][s].tobytes() == w["newest"].tobytes(), f"{tag}: observation"
        assert rows["logits"][s].tobytes() == w["logits"].tobytes(), f"{tag}: logits"
        assert st["value"][s].tobytes() == w["value"].tobytes(), f"{tag}: value"
        assert int(st["action"][s]) == w["action"], f"{tag}: action"
        assert st["reward"][s].tobytes() == o.rewards[lane].tobytes(), f"{tag}: reward"
        got = (int(st["start"][s]), int(st["terminated"][s]), int(st["truncated"][s]), int(st["game_over"][s]), int(st["lives"][s]))
        assert got == (int(o.start[lane]), int(o.term[lane]), int(o.trunc[lane]), int(o.game_over[lane]), int(w["lives"])), tag


@pytest.mark.parametrize("case", ["greedy-84-fp32", "sample-raw-lut-bf16"])
def test_eval_rows(pkg, case):
    rule = dict(rule="greedy") if case.startswith("greedy") else dict(rule="sample", temperature=1.0)
    kw = dict(prec="fp32") if case.startswith("greedy") else dict(prec="bf16", raw=True, lut=LUT)
    d, h = Lanes(pkg, 2, max_steps=40, S=4, **kw), Lanes(pkg, 2, max_steps=40, S=4, device=False, **kw)
    d.eng.rec_open("eval", index=1)
    assert d.eng.rec_count("eval")["capacity"] == 4
    steps, recs = [], []
    for k in range(6):
        d.eng.eval_env_run(steps=4, **rule)
        want = eval_host_steps(h, 4, 1, **rule)
        assert d.eng.rec_count("eval")["rows"] == 4
        rows = drain(d.eng, "eval")
        check_eval_rows(rows, want, 1, 4 * k, f"run {k}")
        steps.append(rows["steps"])
        recs += [w["o"] for w in want]
    for name in ("observations", "logits", "values", "actions"):  # the lanes themselves are where the host loop's are
        assert d.eng.eval_read(name).tobytes() == h.eng.eval_read(name).tobytes(), name
    assert [s for s, o in enumerate(recs) if o.trunc[1]] == [10, 21]  # from the reference
    episodes, unfinished = rr.split_episodes(np.concatenate(steps))
    assert episodes == [(0, 10, True), (11, 21, True)] and unfinished == 22
    # a host-driven step on the recorded context: one more ordinal, no row
    d.envs.load_state(d.eng.eval_env_state())
    d.host_steps(1, **rule)
    n = d.eng.rec_count("eval")
    assert (n["rows"], n["next_ordinal"]) == (0, 25), n
    d.close(), h.close()


def test_both_recorders_and_evaluation_runs_change_nothing(pkg):
    """a: the rollout recorder only; b: both recorders and evaluation runs between the rollouts; c: the evaluation recorder
    only; p: no recorder, no evaluation.  Rollout rows a == b, evaluation rows b == c, and training is bit-identical in
    all of them"""
    kw = dict(E=3, T=8, prec="bf16", max_steps=40)
    a, b, p = Ctx(pkg, **kw), Ctx(pkg, **kw), Ctx(pkg, **kw)
    c = Lanes(pkg, 2, max_steps=40, S=4, E=3, T=8)
    b.eng.eval_open(2)
    b.eng.eval_env_open(run_steps=4, max_steps=40)
    a.eng.rec_open("rollout", index=2)
    b.eng.rec_open("rollout", index=2), b.eng.rec_open("eval", index=0)
    c.eng.rec_open("eval", index=0)
    for k in range(3):
        b.eng.eval_env_run(steps=4, rule="sample"), c.eng.eval_env_run(steps=3 + (k & 1), rule="sample")
        if not k & 1:
            c.eng.eval_env_run(steps=1, rule="sample")
        ra, rp = a.device_rollout(), p.device_rollout()
        rb = b.device_rollout(between=lambda: b.eng.eval_env_run(steps=2, rule="greedy"))
        c.eng.eval_env_run(steps=2, rule="greedy")
        same(rp, ra, f"rollout {k} with the rollout recorder"), same(rp, rb, f"rollout {k} with both and evaluation runs")
        ea, eb = drain(a.eng, "rollout"), drain(b.eng, "rollout")
        for key in ea:
            assert ea[key].tobytes() == eb[key].tobytes(), f"rollout rows: {key}"
        assert b.eng.rec_count("eval")["dropped"] == 2 and c.eng.rec_count("eval")["dropped"] == 2  # (6 steps, capacity 4)
        eb, ec = drain(b.eng, "eval"), drain(c.eng, "eval")
        for key in eb:
            assert len(eb[key]) == 4 and eb[key].tobytes() == ec[key].tobytes(), f"evaluation rows: {key}"
    for x in (a, b, p):  # (once, after the loop: c has no rollout to train on and must keep b's parameters)
        x.eng.train(2.5e-4, 1, 2)
    assert a.eng.export_params().tobytes() == p.eng.export_params().tobytes() == b.eng.export_params().tobytes()
    assert a.eng.state_digest() == p.eng.state_digest() == b.eng.state_digest()
    for x in (a, b, p, c):
        x.close()


# ------------------------------------------------------------------ every refusal; a refused call changes nothing
def test_arguments(pkg):
    E, T, L = 3, 8, 2
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    x = Ctx(pkg, E=E, T=T, max_steps=40, device_env=False)
    ctx = x.eng._ctx
    INV, RUN, OK = pkg.ERR_INVALID_ARGUMENT, pkg.ERR_RUNTIME, pkg.OK

    def cfg(source=0, index=0, content=3, capacity=T, reserved=(0, 0, 0, 0)):
        return pkg.RecConfig(source, index, content, capacity, (C.c_int32 * 4)(*reserved))

    def open_(**kw):
        return lib.aleppo_rec_open(ctx, C.byref(cfg(**kw)))

    def read(source, field, first, rows, buf, nbytes):
        return lib.aleppo_rec_read(ctx, C.c_int(source), C.c_int(field), C.c_uint64(first), C.c_uint64(rows),
                                   None if buf is None else ptr(buf), C.c_size_t(nbytes))
    counts = lambda: (x.eng.rec_count("rollout"), x.eng.rec_count("eval"))
    zero = dict(rows=0, dropped=0, next_ordinal=0, capacity=0, frame_bytes=0, observation_bytes=0, actions=0)
    buf = np.zeros(T * 7056, np.uint8)
    # before aleppo_env_open / aleppo_eval_env_open
    assert open_() == RUN and open_(source=1) == RUN and counts() == (zero, zero)
    assert read(0, 0, 0, 0, buf, 0) == RUN and lib.aleppo_rec_clear(ctx, 0) == RUN and lib.aleppo_rec_clear(ctx, 1) == RUN
    x.eng.env_open(**x.env_args)
    x.eng.eval_open(L)
    assert open_(source=1) == RUN  # (evaluation lanes, but no evaluation environments)
    x.eng.eval_env_open(run_steps=4, max_steps=40)
    # aleppo_rec_open's invalid arguments, for both sources, closed and open
    bad = [dict(source=2), dict(source=-1), dict(index=-1), dict(index=E), dict(source=1, index=L), dict(source=1, index=-1),
           dict(content=0), dict(content=4), dict(content=7), dict(source=1, content=0), dict(capacity=0),
           dict(capacity=65537), dict(capacity=-1), dict(source=1, capacity=0)] + \
          [dict(reserved=tuple(int(j == k) for j in range(4))) for k in range(4)]
    for state in ("closed", "open"):
        before = counts()
        assert lib.aleppo_rec_open(ctx, None) == INV
        for kw in bad:
            assert open_(**kw) == INV, (state, kw)
            assert counts() == before, (state, kw)
        if state == "closed":
            assert before == (zero, zero)
            assert open_(index=1, content=pkg.REC_OBSERVATION) == OK and open_(source=1, capacity=4) == OK
    x.device_rollout()
    before = counts()
    assert before[0]["rows"] == T and before[0]["frame_bytes"] == 0 and before[0]["observation_bytes"] == 7056
    # another config for an open source
    for kw in (dict(index=0, content=2), dict(index=1, content=3), dict(index=1, content=2, capacity=T - 1),
               dict(source=1, capacity=3), dict(source=1, capacity=4, index=1)):
        assert open_(**kw) == RUN and counts() == before, kw
    # aleppo_rec_count / aleppo_rec_clear
    n = pkg.RecCounts()
    assert lib.aleppo_rec_count(ctx, 0, None) == INV and lib.aleppo_rec_count(ctx, 2, C.byref(n)) == INV
    assert lib.aleppo_rec_clear(ctx, 2) == INV and lib.aleppo_rec_clear(ctx, -1) == INV and counts() == before
    # aleppo_rec_read
    F = pkg.REC_FIELDS
    assert read(0, F["observations"], 0, T, buf, T * 7056) == OK
    assert read(0, F["observations"], T, 0, buf, 0) == OK and read(0, F["steps"], 3, 2, buf, 64) == OK
    for args in ((0, F["observations"], 0, T + 1, buf, (T + 1) * 7056), (0, F["observations"], T + 1, 0, buf, 0),
                 (0, F["observations"], T, 1, buf, 7056), (0, F["steps"], 2 ** 63, 2 ** 63, buf, 0),
                 (0, F["observations"], 0, T, buf, T * 7056 - 1), (0, F["steps"], 0, T, buf, T * 32 + 1),
                 (0, F["logits"], 0, T, buf, T * A * 4 - 4), (0, 4, 0, 1, buf, 32), (0, -1, 0, 1, buf, 32),
                 (0, F["frames"], 0, 1, buf, 7056),  # not part of content
                 (0, F["steps"], 0, 1, None, 32), (2, F["steps"], 0, 1, buf, 32), (1, F["steps"], 0, 1, buf, 32)):  # (eval: no rows)
        assert read(*args) == INV, args
        assert counts() == before, args
    # while a step is armed: everything but aleppo_rec_count
    x.envs.load_state(x.eng.env_state())
    f_addr, s_addr = x.eng.host_alloc(E * 7056), x.eng.host_alloc(E)
    f_map = np.ctypeslib.as_array((C.c_uint8 * (E * 7056)).from_address(f_addr))
    s_map = np.ctypeslib.as_array((C.c_uint8 * E).from_address(s_addr))
    o = x.envs.step(x.eng.act().copy())
    x.eng.arm_step(f_addr, s_addr)
    assert open_(index=1, content=2) == RUN and read(0, F["steps"], 0, 1, buf, 32) == RUN and lib.aleppo_rec_clear(ctx, 0) == RUN
    assert counts() == before
    f_map[:], s_map[:] = o.frames.ravel(), o.start
    x.eng.release_step(o.rewards, o.term, o.trunc)
    for _ in range(T - 1):
        o = x.envs.step(x.eng.act().copy())
        x.eng.step(o.frames, o.rewards, o.term, o.trunc, o.start, kind=x.kind)
    x.eng.finish_rollout()
    n = x.eng.rec_count("rollout")
    assert (n["rows"], n["dropped"], n["next_ordinal"]) == (T, 0, 2 * T), n  # (the host-driven slots: ordinals only)
    assert lib.aleppo_rec_clear(ctx, 0) == OK and x.eng.rec_count("rollout")["rows"] == 0
    x.eng.host_free(f_addr), x.eng.host_free(s_addr)
    x.close()
