"""GPU: the device-resident evaluation environments (include/aleppo.h: aleppo_eval_env_open / aleppo_eval_env_run /
aleppo_eval_env_export_state / aleppo_eval_env_import_state / aleppo_eval_env_read) through the C ABI.  The reference is
the host loop on a second context with the same seed and parameters: eval_act -> tests/device_env_ref.py's EnvSet.step ->
eval_push_frames.  Everything is compared byte for byte - the lanes' fields, the frame buffer, the exported state, the
four [S,L] log planes - and each case asserts from the REFERENCE's records that the branch it is there for occurred."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import device_env_ref as ref
import hashfill as hf
from conftest import ROOT
from shared_fixtures import trainer  # noqa: F401
from __graft_entry__ import load_package
from test_device_env import LUT, PLANES
from test_eval_lanes import scalars

pytestmark = pytest.mark.gpu
A, H = 4, 32
FIELDS = ("observations", "logits", "values", "actions")
LOGS = ("episode_returns", "episode_lengths", "game_returns", "game_lengths")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


class Lanes:
    """one Engine with L evaluation lanes, and the reference environments of the host loop (kept on a device context too:
    they are what state and frames are compared with, and what a host-driven step on it steps)"""

    def __init__(self, pkg, L, prec="bf16", raw=False, max_steps=108000, max_return=-1.0, seed_base=0, lut=None, opts=(),
                 S=32, device=True, E=4, T=8):
        self.pkg, self.L, self.S, self.raw = pkg, L, S, raw
        self.kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
        self.env_args = dict(frame_kind=self.kind, seed_base=seed_base, max_steps=max_steps, max_return=max_return)
        self.eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=5)
        self.eng.load_params(hf.fill_params(310, H, A))
        if lut is not None:
            self.eng.set_gray_lut(lut)
        for o, v in opts:  # (before eval_open: the lanes' scratch follows the acting path)
            self.eng.set_option(o, v)
        self.eng.eval_open(L)
        self.envs = ref.EnvSet(L, seed_base, max_steps, max_return, raw)
        if device:
            self.eng.eval_env_open(run_steps=S, **self.env_args)
        self.recs = []  # the reference's records of every host-driven step

    def host_steps(self, n, **rule):
        for _ in range(n):
            actions = self.eng.eval_act(**rule).copy()
            o = self.envs.step(actions)
            self.eng.eval_push_frames(o.frames, o.start, kind=self.kind)
            self.recs.append(o)

    def fields(self):
        return {k: self.eng.eval_read(k) for k in FIELDS}

    def close(self):
        self.eng.close()


def same(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), f"{what}.{k} differs"


def device_side(d):
    out = d.fields()
    out["frames"], out["state"] = d.eng.eval_env_read("frames"), d.eng.eval_env_state()
    out.update({k: d.eng.eval_env_read(k) for k in LOGS})
    return out


def host_side(h, steps, S):
    """what the device context must hold after a run of `steps` steps: the host context's fields, the reference's last
    frames and state, and its last `steps` records as [S,L] planes with the rows past the run zero"""
    out = h.fields()
    recs = h.recs[-steps:]
    out["frames"], out["state"] = recs[-1].frames, h.envs.state(h.pkg.ENV_STATE_DTYPE)
    for k, attr, dt in zip(LOGS, ("ep_ret", "ep_len", "game_ret", "game_len"), (np.float32, np.uint32) * 2):
        p = np.zeros((S, h.L), dt)
        p[:steps] = np.stack([getattr(o, attr) for o in recs])
        out[k] = p
    return out


def run_both(d, h, steps, what, **rule):
    d.eng.eval_env_run(steps=steps, **rule)
    h.host_steps(steps, **rule)
    same(host_side(h, steps, d.S), device_side(d), what)


def seen(recs):
    return dict(term=sum(int(o.term.sum()) for o in recs), trunc=sum(int(o.trunc.sum()) for o in recs),
                game_over=sum(int((o.game_len > 0).sum()) for o in recs),
                game_over_by_life_loss=sum(int(((o.game_len > 0) & (o.term > 0)).sum()) for o in recs))


def pair(pkg, L, **kw):
    return Lanes(pkg, L, **kw), Lanes(pkg, L, device=False, **kw)


# ------------------------------------------------------------------ 1. the device run IS the host loop
def test_a_fp32_greedy_one_run_with_truncations_and_game_overs(pkg):
    d, h = pair(pkg, 5, prec="fp32", max_steps=40, S=24)
    run_both(d, h, 24, "a", rule="greedy")
    s = seen(h.recs)
    assert s["trunc"] == 10 and s["term"] == 0 and s["game_over"] == 10, s  # 10 agent steps per episode whatever the actions
    el = d.eng.eval_env_episodes()
    assert el[1].tolist() == [10] * 10 and el[3].tolist() == [10] * 10
    d.close(), h.close()


def test_b_raw_lut_sample_two_runs_then_mixing(pkg):
    """case b: L = 65 (17 head workgroups, the last partial), bf16, raw pairs under a non-identity LUT, sample at tau = 1,
    max_return = 6, two runs of 16 at S = 16: state, counter and the log's reset cross a run boundary.  Then the mixing
    checks on the same contexts.  A return of 6 takes three brick rows (1 + 1 + 4), the third no sooner than the 34th
    step: the truncation this case is there for is met in the steps of the mixing part, which are compared like the rest."""
    rule = dict(rule="sample", temperature=1.0)
    d, h = pair(pkg, 65, raw=True, max_return=6.0, lut=LUT, S=16)
    run_both(d, h, 16, "b run 0", **rule)
    run_both(d, h, 16, "b run 1", **rule)
    assert seen(h.recs)["term"] >= 1
    # one act with the built-in generator: counter and ticket agree
    ad, ah = d.eng.eval_act(**rule).copy(), h.eng.eval_act(**rule).copy()
    assert ad.tobytes() == ah.tobytes() and d.eng.eval_read("logits").tobytes() == h.eng.eval_read("logits").tobytes()
    # one host-driven step on the device context (the same reference environments, loaded from its exported state), then a
    # device run of 4: equal to 5 host-driven steps
    d.envs.load_state(d.eng.eval_env_state())
    d.host_steps(1, **rule)
    d.eng.load_eval_env_state(d.envs.state(pkg.ENV_STATE_DTYPE))
    d.eng.eval_env_run(steps=4, **rule)
    h.host_steps(5, **rule)
    same(host_side(h, 4, 16), device_side(d), "b mixed")
    s = seen(h.recs)
    print("b", s)
    assert s["trunc"] >= 1, s
    d.close(), h.close()


def test_c_epsilon_runs_of_1_and_19(pkg):
    rule = dict(rule="epsilon", epsilon=0.3)
    d, h = pair(pkg, 3, max_steps=40, S=32)
    run_both(d, h, 1, "c run of 1", **rule)
    run_both(d, h, 19, "c run of 19", **rule)
    assert seen(h.recs)["trunc"] >= 1
    d.close(), h.close()


def test_d_life_loss_and_game_over_by_life_loss(pkg):
    rule = dict(rule="sample", temperature=1.0)
    d, h = pair(pkg, 65, max_steps=400, S=48)
    for c in (d, h):  # lives = 1 in the first 16 lanes, on both sides
        st = c.envs.state(pkg.ENV_STATE_DTYPE)
        st["lives"][:16] = 1
        c.envs.load_state(st)
    d.eng.load_eval_env_state(st)
    run_both(d, h, 48, "d", **rule)
    s = seen(h.recs)
    print("d", s)
    assert s["term"] >= 1 and s["game_over_by_life_loss"] >= 1, s
    d.close(), h.close()


@pytest.mark.parametrize("path", ["fused-act-0", "generic-conv"])
def test_e_separate_launch_acting_paths(pkg, path):
    opts = ((pkg.OPT_FUSED_ACT, 0),) if path == "fused-act-0" else ((pkg.OPT_GENERIC_CONV, 1),)
    d, h = pair(pkg, 5, max_steps=40, S=16, opts=opts)
    run_both(d, h, 16, path, rule="greedy")
    assert seen(h.recs)["trunc"] >= 1
    d.close(), h.close()


# ------------------------------------------------------------------ 3. re-seeding equals a fresh context
def test_reseeding_equals_a_fresh_context(pkg):
    kw = dict(max_steps=40, S=16)
    d = Lanes(pkg, 5, **kw)
    d.eng.eval_env_run(rule="greedy", steps=16)
    d.eng.eval_env_open(run_steps=16, **dict(d.env_args, seed_base=1000))
    assert all((d.eng.eval_env_read(k) == 0).all() for k in LOGS)  # (the log is empty again)
    f = Lanes(pkg, 5, seed_base=1000, **kw)
    for c in (d, f):
        c.eng.eval_env_run(rule="greedy", steps=12)
    a, b = device_side(d), device_side(f)
    for k in ("frames", "state", "observations") + LOGS:  # (every lane starts with a start step: the stacks agree too)
        assert a[k].tobytes() == b[k].tobytes(), k
    assert int((a["episode_lengths"] > 0).sum()) >= 5
    d.close(), f.close()


# ------------------------------------------------------------------ 4. isolation
def _training_run(pkg, device_rollout, with_eval):
    E, T = 4, 8
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16, seed=5)
    eng.load_params(hf.fill_params(310, H, A))
    envs = ref.EnvSet(E, 0, 40, -1.0, False)
    eng.env_open(max_steps=40)
    n = [0]

    def ev():
        if not with_eval:
            return
        if n[0] == 0:
            eng.eval_open(3)
        eng.eval_env_open(seed_base=50 + n[0], max_steps=40, run_steps=8)
        eng.eval_env_run(rule="epsilon", epsilon=0.3, steps=5)
        n[0] += 1
    out = []
    for _ in range(2):
        ev()
        if device_rollout:
            eng.env_rollout()
        else:
            for _ in range(T):
                o = envs.step(eng.act().copy())
                eng.step(o.frames, o.rewards, o.term, o.trunc, o.start)
        ev()
        eng.finish_rollout()
        ev()
        batch = {k: eng.read_batch(k) for k in PLANES}
        eng.train(2.5e-4, 1, 2)
        sd = eng.state_dict()
        batch.update({k: np.asarray(sd[k]) for k in ("params", "exp_avg", "exp_avg_sq", "step")})
        batch["digest"] = np.array(list(eng.state_digest().values()), np.uint64)
        batch["env_state"] = eng.env_state()
        out.append(batch)
    eng.close()
    return out


@pytest.mark.parametrize("device_rollout", [False, True], ids=["host-steps", "env-rollout"])
def test_training_run_is_unchanged_by_evaluation_runs(pkg, device_rollout):
    plain, mixed = _training_run(pkg, device_rollout, False), _training_run(pkg, device_rollout, True)
    for r in range(2):
        same(plain[r], mixed[r], f"rollout {r}")


# ------------------------------------------------------------------ 5. refusals change nothing
def test_refusals_change_nothing(pkg):
    L, S = 5, 8
    lib = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st, plane = np.zeros(L, pkg.ENV_STATE_DTYPE), np.zeros((S, L), np.float32)
    cfg = lambda **kw: pkg.EnvConfig(*[kw.get(k, v) for k, v in (("kind", 0), ("frame_kind", 0), ("seed_base", 0),
                                                                ("max_steps", 40), ("max_return", -1.0), ("reserved", 0))])

    def calls(ctx):
        return (lib.aleppo_eval_env_run(ctx, 0, C.c_float(0), 1), lib.aleppo_eval_env_export_state(ctx, p(st), C.c_size_t(L)),
                lib.aleppo_eval_env_import_state(ctx, p(st), C.c_size_t(L)),
                lib.aleppo_eval_env_read(ctx, 1, p(plane), C.c_size_t(plane.nbytes)))
    x = Lanes(pkg, L, max_steps=40, S=S, device=False)
    y = Lanes(pkg, L, max_steps=40, S=S)  # the twin on which none of this is tried
    ctx = x.eng._ctx
    # before eval_open (a context of its own) and before eval_env_open
    e0 = pkg.Engine(4, 8, A, H, precision=pkg.BF16, seed=5)
    assert lib.aleppo_eval_env_open(e0._ctx, C.byref(cfg()), S) == pkg.ERR_RUNTIME
    assert calls(e0._ctx) == (pkg.ERR_RUNTIME,) * 4
    e0.close()
    assert calls(ctx) == (pkg.ERR_RUNTIME,) * 4
    # bad configs, S out of range
    for bad in (dict(kind=1), dict(frame_kind=2), dict(reserved=1)):
        assert lib.aleppo_eval_env_open(ctx, C.byref(cfg(**bad)), S) == pkg.ERR_INVALID_ARGUMENT, bad
    for s_bad in (0, 1025, -1):
        assert lib.aleppo_eval_env_open(ctx, C.byref(cfg()), s_bad) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_open(ctx, None, S) == pkg.ERR_INVALID_ARGUMENT
    assert calls(ctx) == (pkg.ERR_RUNTIME,) * 4  # (a refused open leaves them closed)
    x.eng.eval_env_open(run_steps=S, **x.env_args)
    for other in (dict(frame_kind=1), dict(max_steps=44), dict(max_return=3.0)):
        assert lib.aleppo_eval_env_open(ctx, C.byref(cfg(**other)), S) == pkg.ERR_RUNTIME, other
    assert lib.aleppo_eval_env_open(ctx, C.byref(cfg()), S + 1) == pkg.ERR_RUNTIME
    # steps, rule and param
    nan, inf = float("nan"), float("inf")
    for rule, param, steps in ((0, 0.0, 0), (0, 0.0, S + 1), (0, 0.0, -1), (3, 0.0, 1), (-1, 0.0, 1), (0, 0.5, 1), (0, nan, 1),
                               (1, 0.0, 1), (1, -1.0, 1), (1, nan, 1), (1, inf, 1), (2, -0.01, 1), (2, 1.01, 1), (2, nan, 1)):
        assert lib.aleppo_eval_env_run(ctx, rule, C.c_float(param), steps) == pkg.ERR_INVALID_ARGUMENT, (rule, param, steps)
    # byte counts, fields, sizes, null pointers
    for field, nbytes in ((0, L * 7056), (1, 4 * S * L), (2, 4 * S * L), (3, 4 * S * L), (4, 4 * S * L)):
        buf = np.zeros(nbytes + 8, np.uint8)
        for wrong in (nbytes - 1, nbytes + 1, 0):
            assert lib.aleppo_eval_env_read(ctx, field, p(buf), C.c_size_t(wrong)) == pkg.ERR_INVALID_ARGUMENT
        assert lib.aleppo_eval_env_read(ctx, field, p(buf), C.c_size_t(nbytes)) == pkg.OK
    for field in (5, -1):
        assert lib.aleppo_eval_env_read(ctx, field, p(plane), C.c_size_t(plane.nbytes)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_read(ctx, 0, None, C.c_size_t(L * 7056)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_export_state(ctx, p(st), C.c_size_t(L + 1)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_import_state(ctx, p(st), C.c_size_t(L - 1)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_export_state(ctx, None, C.c_size_t(L)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_eval_env_import_state(ctx, None, C.c_size_t(L)) == pkg.ERR_INVALID_ARGUMENT
    # each invalid aleppo_env_state field: refused, and nothing is taken over
    good = x.eng.eval_env_state()
    assert good.tobytes() == y.eng.eval_env_state().tobytes()
    for field, value in (("lives", 6), ("lives", -1), ("paddle", 3), ("paddle", 80), ("ball_x", 84), ("ball_y", -1),
                         ("prev_x", 84), ("prev_y", 100), ("dx", 0), ("dy", 2), ("bricks", -1), ("start", 2),
                         ("game_over", 2), ("reward", np.nan), ("ep_ret", np.inf), ("game_ret", -np.inf),
                         ("episode_return", np.nan), ("reserved", 1)):
        bad = good.copy()
        bad[field][L - 1] = value  # (the LAST lane: nothing in front of it may have been taken over either)
        with pytest.raises(pkg.AleppoInvalidArgument, match=f"lane {L - 1}"):
            x.eng.load_eval_env_state(bad)
        assert x.eng.eval_env_state().tobytes() == good.tobytes(), field
    # while a step is armed: all five are refused
    fbuf, sbuf = x.eng.host_alloc(4 * 7056), x.eng.host_alloc(4)
    x.eng.act()
    x.eng.arm_step(fbuf, sbuf)
    assert calls(ctx) == (pkg.ERR_RUNTIME,) * 4
    with pytest.raises(pkg.AleppoError, match="armed"):
        x.eng.eval_env_open(run_steps=S, **x.env_args)
    C.memset(fbuf, 0, 4 * 7056)
    C.memmove(sbuf, np.ones(4, np.uint8).ctypes.data, 4)
    x.eng.release_step(np.zeros(4, np.float32), np.zeros(4, np.uint8), np.zeros(4, np.uint8))
    # after the whole list a run of 8 steps is the twin's
    for c in (x, y):
        c.eng.eval_env_run(rule="epsilon", epsilon=0.3, steps=8)
    same(device_side(y), device_side(x), "the run after the refused calls")
    assert int((x.eng.eval_env_read("episode_lengths") > 0).sum()) == 0 and x.eng.eval_env_state()["steps"].min() == 28
    x.eng.host_free(fbuf), x.eng.host_free(sbuf)
    x.close(), y.close()


# ------------------------------------------------------------------ 6. the trainer
def _train(trainer, d, txt):
    os.makedirs(d / "tb")
    cfg = d / "debug.yaml"
    cfg.write_text(txt)
    dump = d / "final.bin"
    r = subprocess.run([trainer, "breakout.bin", str(d / "tb" / "run.log"), str(d), "grp", str(cfg)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, ALEPPO_TRAINER_DUMP_FINAL=str(dump)))
    assert r.returncode == 0, r.stderr[-2000:]
    tail = re.search(r"steps (\d+) episodes (\d+)", r.stdout).groups()
    files = [f for f in os.listdir(d / "tb") if f.startswith("run.tfevents.")]
    assert len(files) == 1
    sc = scalars(str(d / "tb" / files[0]))
    return dict(tail=tail, params=np.fromfile(dump, np.float32), train=[s for s in sc if not s[0].startswith("eval/")],
                eval=[s for s in sc if s[0].startswith("eval/")])


@pytest.mark.parametrize("device_envs", ["", "device_environments: true\n"], ids=["host-envs", "device-envs"])
def test_trainer_device_evaluation_logs_what_host_evaluation_logs(trainer, tmp_path, device_envs):
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read().replace("num_rollouts: 10", "num_rollouts: 3")
    txt = txt.replace("precision: fp32", "precision: bf16") + device_envs
    keys = "eval_interval: 1\neval_environments: 3\neval_episodes: 4\neval_rule: epsilon\neval_epsilon: 0.05\n"
    plain = _train(trainer, tmp_path / "plain", txt)
    host = _train(trainer, tmp_path / "host", txt + keys)
    assert not plain["eval"] and len(host["eval"]) == 3 * 4
    for k in ("tail", "train"):
        assert plain[k] == host[k], k
    assert plain["params"].tobytes() == host["params"].tobytes()
    for S in (1, 4, 32):
        dev = _train(trainer, tmp_path / f"dev{S}", txt + keys + f"device_evaluation: true\ndevice_evaluation_steps: {S}\n")
        print(S, [(t, struct.unpack("<f", struct.pack("<I", v))[0]) for t, _, v in dev["eval"]])
        assert dev["eval"] == host["eval"], S
        assert dev["train"] == host["train"] and dev["tail"] == host["tail"], S
        assert dev["params"].tobytes() == host["params"].tobytes(), S
