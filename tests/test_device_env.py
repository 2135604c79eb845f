"""GPU: the device-resident environments (include/aleppo.h: aleppo_env_open / aleppo_env_rollout / aleppo_env_export_state /
aleppo_env_import_state / aleppo_env_read) through the C ABI.  Every test drives two contexts with the same seed and
parameters: one runs env_rollout, the other the host loop act -> reference environment (tests/device_env_ref.py, pinned
against trainer/emulator.hpp by tests/test_device_env_ref.py) -> step with host frames.  After finish_rollout every plane
of read_batch, the episode log, the exported environment state and state_digest are compared byte for byte: there is no
tolerance anywhere.  Each case asserts from the REFERENCE's records that the branch it is there for occurred."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import device_env_ref as ref
import hashfill as hf
from conftest import ROOT
from __graft_entry__ import load_package

A, H = 4, 32
PLANES = ("observations", "actions", "rewards", "terminals", "truncations", "masks", "logits", "values", "advantages",
          "returns", "log_probs", "next_values", "current_obs")
LUT = ((np.arange(256) * 7 + 3) % 256).astype(np.uint8)  # a permutation of the palette: not the identity


@pytest.fixture(scope="module")
def pkg():
    return load_package()


class Ctx:
    """one Engine, its parameters and options, and (for the host loop) the reference environments"""

    def __init__(self, pkg, E, T, prec="fp32", raw=False, max_steps=108000, max_return=-1.0, seed_base=0, lut=None,
                 opts=(), rollout_fp16=False, advantage_norm=False, actions=A, device_env=True):
        self.pkg, self.E, self.T, self.raw = pkg, E, T, raw
        self.kind = pkg.FRAMES_RAW_PAIR if raw else pkg.FRAMES_84
        self.env_args = dict(frame_kind=self.kind, seed_base=seed_base, max_steps=max_steps, max_return=max_return)
        self.eng = pkg.Engine(E, T, actions, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=5,
                              rollout_precision=pkg.ROLLOUT_FP16 if rollout_fp16 else pkg.ROLLOUT_FP32,
                              advantage_norm=advantage_norm)
        self.eng.load_params(hf.fill_params(310, H, actions))
        if lut is not None:
            self.eng.set_gray_lut(lut)
        for o, v in opts:
            if o == "reward_scale":
                self.eng.set_reward_scaling(True)
            else:
                self.eng.set_option(o, v)
        self.envs = ref.EnvSet(E, seed_base, max_steps, max_return, raw)  # (the device context keeps it for load / compare)
        if device_env:
            self.eng.env_open(**self.env_args)
        self.slots = []  # the reference's records of the last host rollout

    def read(self):
        out = {n: self.eng.read_batch(n) for n in PLANES}
        out["digest"] = np.array(list(self.eng.state_digest().values()), np.uint64)
        return out

    def device_rollout(self, between=None):
        self.eng.env_rollout()
        if between:
            between()
        self.eng.finish_rollout()
        out = self.read()
        out["episodes"] = dict(zip("abcd", self.eng.env_episodes()))
        out["env_state"] = self.eng.env_state()
        return out

    def host_rollout(self):
        self.slots = []
        for _ in range(self.T):
            actions = self.eng.act().copy()
            o = self.envs.step(actions)
            self.eng.step(o.frames, o.rewards, o.term, o.trunc, o.start, kind=self.kind)
            self.slots.append(o)
        self.eng.finish_rollout()
        out = self.read()
        out["episodes"] = dict(zip("abcd", ref.compact(self.slots)))
        out["env_state"] = self.envs.state(self.pkg.ENV_STATE_DTYPE)
        return out

    def seen(self):
        """what the reference recorded in the last host rollout: terminals, truncations, game overs, game overs by life loss"""
        s = self.slots
        return dict(term=sum(int(o.term.sum()) for o in s), trunc=sum(int(o.trunc.sum()) for o in s),
                    game_over=sum(int((o.game_len > 0).sum()) for o in s),
                    game_over_by_life_loss=sum(int(((o.game_len > 0) & (o.term > 0)).sum()) for o in s))

    def close(self):
        self.eng.close()


def same(a, b, what):
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], f"{what}.{k}")
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
            assert x.tobytes() == y.tobytes(), f"{what}.{k} differs"


def E_first_slot(r):
    return r["masks"].shape[0]  # (every environment starts its first rollout with a start slot)


def pair(pkg, **kw):
    return Ctx(pkg, **kw), Ctx(pkg, device_env=False, **kw)


def set_lives(c, n_envs, lives):
    """import `lives` into the first n_envs environments of a device context and of a host context's reference"""
    st = c.envs.state(c.pkg.ENV_STATE_DTYPE)
    st["lives"][:n_envs] = lives
    c.envs.load_state(st)
    return st


# ------------------------------------------------------------------ the device rollout IS the host loop's rollout
CASES = {
    # two consecutive rollouts each: the state carried across the rollout boundary is part of what is compared
    "life-loss-bf16-84-E65": dict(kw=dict(E=65, T=48, prec="bf16", max_steps=400), want="term", rollouts=2),
    "max-steps-40-fp32-84-E3": dict(kw=dict(E=3, T=24, max_steps=40), want="trunc", count=6, rollouts=2),
    "max-return-6-raw-lut-E65": dict(kw=dict(E=65, T=64, raw=True, max_return=6.0, lut=LUT), want="trunc", rollouts=2),
    "game-over-raw-bf16-E130": dict(kw=dict(E=130, T=32, prec="bf16", raw=True), want="game_over_by_life_loss", lives=(16, 1),
                                     rollouts=2),
    # options that read the records, and both start-flag paths of the ingest
    "reward-scale": dict(kw=dict(E=5, T=16, max_steps=40, opts=(("reward_scale", 1),)), want="trunc", rollouts=2),
    "advantage-norm": dict(kw=dict(E=5, T=16, max_steps=40, advantage_norm=True), want="trunc", rollouts=1),
    "rollout-fp16": dict(kw=dict(E=5, T=16, prec="bf16", max_steps=40, rollout_fp16=True), want="trunc", rollouts=2),
    "fused-act-0": dict(kw=dict(E=5, T=16, prec="bf16", max_steps=40), fused=0, want="trunc", rollouts=1),
    "fused-act-2": dict(kw=dict(E=5, T=16, prec="bf16", raw=True, max_steps=40, lut=LUT), fused=2, want="trunc", rollouts=1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_device_rollout_equals_the_host_loop(pkg, case):
    c = CASES[case]
    kw = dict(c["kw"])
    if "fused" in c:
        kw["opts"] = ((pkg.OPT_FUSED_ACT, c["fused"]),)
    d, h = pair(pkg, **kw)
    if "lives" in c:
        d.eng.load_env_state(set_lives(d, *c["lives"]))
        set_lives(h, *c["lives"])
    seen = dict(term=0, trunc=0, game_over=0, game_over_by_life_loss=0)
    for k in range(c["rollouts"]):
        rd, rh = d.device_rollout(), h.host_rollout()
        for key, v in h.seen().items():
            seen[key] += v
        if k == 0 and "count" in c:  # max_steps = 40: 10 agent steps per episode whatever the actions are
            assert seen["trunc"] == c["count"] and seen["term"] == 0, seen
        same(rh, rd, f"{case} rollout {k}")
        if k == 0:
            assert int(rh["masks"].size - rh["masks"].sum()) > E_first_slot(rh)  # (start slots past slot 0: stale rewards)
    print(case, seen)
    assert seen[c["want"]] >= 1, seen
    d.close(), h.close()


# ------------------------------------------------------------------ the renderer on its own
@pytest.mark.gpu
@pytest.mark.parametrize("raw", [False, True], ids=["84", "raw"])
def test_renderer_on_hand_made_states(pkg, raw):
    """two actions only (NOOP, FIRE): the paddle stays where the imported state puts it - at 4 and at 79, where its
    rectangle is clipped - and the ball, eight emulator frames on, is at x = 82 in half of the environments"""
    E, T = 8, 2
    d = Ctx(pkg, E, T, raw=raw, actions=2)
    st = d.envs.state(pkg.ENV_STATE_DTYPE)
    st["start"], st["lives"] = 0, 3
    st["paddle"] = [4, 79, 4, 79, 42, 5, 78, 40]
    st["ball_x"], st["dx"] = [66, 66, 18, 18, 66, 50, 30, 66], [1, 1, -1, -1, 1, 1, -1, 1]
    st["ball_y"], st["dy"] = [30, 36, 40, 44, 48, 50, 30, 26], [1, 1, 1, 1, -1, -1, 1, -1]
    st["prev_x"], st["prev_y"] = st["ball_x"] - 2 * st["dx"], st["ball_y"] - 2 * st["dy"]
    st["bricks"] = np.arange(E)
    d.eng.load_env_state(st)
    d.envs.load_state(st)
    d.eng.env_rollout()
    d.eng.finish_rollout()
    actions = d.eng.read_batch("actions")  # [E, T]
    for t in range(T):
        o = d.envs.step(actions[:, t])
    frames = d.eng.env_read("frames")
    assert frames.shape == o.frames.shape and frames.tobytes() == o.frames.tobytes()
    after = d.envs.state(pkg.ENV_STATE_DTYPE)
    assert d.eng.env_state().tobytes() == after.tobytes()
    assert list(after["paddle"][:4]) == [4, 79, 4, 79] and list(after["ball_x"][[0, 1, 4, 7]]) == [82] * 4
    assert (after["ball_x"][[2, 3]] == 2).all() and after["bricks"][7] > 7  # (the left wall; a brick row hit)
    d.close()


# ------------------------------------------------------------------ continuity, mixing, isolation
@pytest.mark.gpu
def test_exported_state_continues_in_a_fresh_context(pkg):
    kw = dict(E=5, T=16, prec="bf16", max_steps=40)
    a = Ctx(pkg, **kw)
    a.device_rollout()
    a.eng.train(2.5e-4, 1, 2)
    a.device_rollout()
    run, envs = a.eng.run_state(), a.eng.env_state()
    b = Ctx(pkg, **kw)
    b.eng.load_run_state(run)
    b.eng.load_env_state(envs)
    assert b.eng.env_state().tobytes() == envs.tobytes() and b.eng.state_digest() == a.eng.state_digest()
    ra, rb = a.device_rollout(), b.device_rollout()
    same(ra, rb, "the rollout after the import")
    assert ra["episodes"]["b"].size > 0 and int(ra["truncations"].sum()) > 0
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["device", "host"])
def test_host_and_device_rollouts_mix(pkg, first):
    """device, host, device (or host, device, host) on one context, each rollout equal to the all-host run's"""
    kw = dict(E=5, T=16, max_steps=40)
    x, h = pair(pkg, **kw)
    on_device = first == "device"
    for k in range(3):
        want = h.host_rollout()
        if on_device:
            x.eng.load_env_state(x.envs.state(pkg.ENV_STATE_DTYPE))  # (what the host rollout before left; initially the same)
            got = x.device_rollout()
            x.envs.load_state(got["env_state"])
        else:
            got = x.host_rollout()
        same(want, got, f"rollout {k} ({'device' if on_device else 'host'})")
        on_device = not on_device
    assert h.seen()["trunc"] > 0
    x.close(), h.close()


@pytest.mark.gpu
def test_evaluation_calls_around_env_rollout_change_nothing(pkg):
    kw = dict(E=5, T=16, prec="bf16", max_steps=40)
    a, b = Ctx(pkg, **kw), Ctx(pkg, **kw)
    b.eng.eval_open(3)
    frames, start = hf.hf_bytes(77, (3, 84, 84)), np.array([1, 0, 1], np.uint8)

    def evaluate():
        b.eng.eval_push_frames(frames, start)
        b.eng.eval_act("sample")
    for k in range(2):
        evaluate()
        ra = a.device_rollout()
        rb = b.device_rollout(between=evaluate)
        evaluate()
        same(ra, rb, f"rollout {k}")
    a.close(), b.close()


# ------------------------------------------------------------------ errors; a failed call changes nothing
@pytest.mark.gpu
def test_errors_and_a_failed_call_changes_nothing(pkg):
    E, T = 5, 8
    lib = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    kw = dict(E=E, T=T, max_steps=40)
    x, y = Ctx(pkg, device_env=False, **kw), Ctx(pkg, **kw)
    st = np.zeros(E, pkg.ENV_STATE_DTYPE)
    logs = np.zeros((T, E), np.float32)

    def calls(ctx):
        return (lib.aleppo_env_rollout(ctx), lib.aleppo_env_export_state(ctx, p(st), C.c_size_t(E)),
                lib.aleppo_env_import_state(ctx, p(st), C.c_size_t(E)),
                lib.aleppo_env_read(ctx, pkg.ENV_FIELDS["episode_returns"], p(logs), C.c_size_t(logs.nbytes)))
    # before env_open
    assert calls(x.eng._ctx) == (pkg.ERR_RUNTIME,) * 4
    with pytest.raises(pkg.AleppoError, match="aleppo_env_open first"):
        x.eng.env_rollout()
    for bad in (dict(kind=1), dict(frame_kind=2), dict(reserved=1)):
        with pytest.raises(pkg.AleppoInvalidArgument):
            x.eng.env_open(**dict(x.env_args, **bad))
    assert calls(x.eng._ctx) == (pkg.ERR_RUNTIME,) * 4  # (a refused open leaves them closed)
    x.eng.env_open(**x.env_args)
    with pytest.raises(pkg.AleppoError, match="another config"):
        x.eng.env_open(**dict(x.env_args, seed_base=1))
    # wrong byte counts, sizes and null pointers
    ctx = x.eng._ctx
    for name, nbytes in (("frames", E * 7056), ("episode_returns", 4 * T * E), ("game_lengths", 4 * T * E), ("step_ms", 16)):
        buf = np.zeros(nbytes + 8, np.uint8)
        for wrong in (nbytes - 1, nbytes + 1, 0):
            assert lib.aleppo_env_read(ctx, pkg.ENV_FIELDS[name], p(buf), C.c_size_t(wrong)) == pkg.ERR_INVALID_ARGUMENT
        assert lib.aleppo_env_read(ctx, pkg.ENV_FIELDS[name], p(buf), C.c_size_t(nbytes)) == pkg.OK
    assert lib.aleppo_env_read(ctx, 6, p(logs), C.c_size_t(logs.nbytes)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_env_read(ctx, 0, None, C.c_size_t(E * 7056)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_env_export_state(ctx, p(st), C.c_size_t(E + 1)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_env_import_state(ctx, p(st), C.c_size_t(E - 1)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_env_export_state(ctx, None, C.c_size_t(E)) == pkg.ERR_INVALID_ARGUMENT
    assert lib.aleppo_env_import_state(ctx, None, C.c_size_t(E)) == pkg.ERR_INVALID_ARGUMENT
    # a refused import changes nothing
    x.device_rollout(), y.device_rollout()
    good = x.eng.env_state()
    for field, value in (("lives", 6), ("lives", -1), ("paddle", 3), ("paddle", 80), ("ball_x", 84), ("ball_y", -1),
                         ("prev_x", 84), ("prev_y", 100), ("dx", 0), ("dy", 2), ("bricks", -1), ("start", 2),
                         ("game_over", 2), ("reward", np.nan), ("ep_ret", np.inf), ("game_ret", -np.inf),
                         ("episode_return", np.nan), ("reserved", 1)):
        bad = good.copy()
        bad[field][E - 1] = value  # (the LAST environment: nothing in front of it may have been taken over either)
        with pytest.raises(pkg.AleppoInvalidArgument, match=f"environment {E - 1}"):
            x.eng.load_env_state(bad)
        assert x.eng.env_state().tobytes() == good.tobytes(), field
    # t != 0 and an armed step: ALEPPO_ERR_RUNTIME from all of them, and the run goes on as the twin's that never asked
    for c in (x, y):
        c.envs.load_state(c.eng.env_state())
    f_addr, s_addr = x.eng.host_alloc(E * 7056), x.eng.host_alloc(E)
    f_map = np.ctypeslib.as_array((C.c_uint8 * (E * 7056)).from_address(f_addr))
    s_map = np.ctypeslib.as_array((C.c_uint8 * E).from_address(s_addr))
    seen = []
    for t in range(T):
        actions = x.eng.act().copy()
        o = x.envs.step(actions)
        x.eng.arm_step(f_addr, s_addr)
        seen.append(calls(ctx))  # armed
        with pytest.raises(pkg.AleppoError, match="a step is armed"):
            x.eng.env_open(**x.env_args)
        f_map[:], s_map[:] = o.frames.ravel(), o.start
        x.eng.release_step(o.rewards, o.term, o.trunc)
        seen.append(calls(ctx))  # t != 0 (t = T after the last slot: the buffer is full, not finished)
    assert len(seen) == 2 * T and all(s[:3] == (pkg.ERR_RUNTIME,) * 3 for s in seen), seen
    assert all(s[3] == pkg.ERR_RUNTIME for s in seen[0::2]) and all(s[3] == pkg.OK for s in seen[1::2])  # (a read only reads)
    x.eng.finish_rollout()
    y.host_rollout()
    assert x.eng.state_digest() == y.eng.state_digest()
    x.eng.load_env_state(x.envs.state(pkg.ENV_STATE_DTYPE)), y.eng.load_env_state(y.envs.state(pkg.ENV_STATE_DTYPE))
    same(x.device_rollout(), y.device_rollout(), "the device rollout after the refused calls")
    x.eng.host_free(f_addr), x.eng.host_free(s_addr)
    x.close(), y.close()


# ------------------------------------------------------------------ the trainer
@pytest.mark.gpu
@pytest.mark.parametrize("preprocess", ["false", "true"])
def test_trainer_writes_the_same_checkpoint_with_device_environments(tmp_path, preprocess):
    """debug.yaml for 3 rollouts with and without device_environments: the checkpoint files are byte-identical"""
    from __graft_entry__ import build
    build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer")])
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read().replace("num_rollouts: 10", "num_rollouts: 3")
    txt += f"device_preprocess: {preprocess}\n"
    blobs, tails = [], []
    for name, extra in (("host", ""), ("device", "device_environments: true\n")):
        d = tmp_path / name
        os.makedirs(d / "tb")
        cfg = d / "debug.yaml"
        cfg.write_text(txt + extra + f"checkpoint_path: {d / 'run.ckpt'}\ncheckpoint_interval: 3\n")
        r = subprocess.run([os.path.join(ROOT, "trainer", "train"), "breakout.bin", str(d / "tb" / "run.log"), str(d), "grp",
                            str(cfg)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        blobs.append((d / "run.ckpt").read_bytes())
        tails.append(re.search(r"steps (\d+) episodes (\d+) pending_starts (\d+)", r.stdout).groups())
    assert tails[0] == tails[1] and int(tails[0][1]) > 0, tails
    assert blobs[0] == blobs[1]
