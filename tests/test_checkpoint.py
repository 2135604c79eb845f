"""Checkpoint and resume, verified by aleppo_state_digest (include/aleppo.h; trainer keys checkpoint_path,
checkpoint_interval, resume).  CPU: tests/checkpoint_ref.py on a hand-computed case, the trainer's load-time refusals, the
checkpoint file's framing and atomic rename against host-only stand-ins.  GPU: the rollout state's round trip, a resumed
context continuing bit for bit on every acting / update route, the digest against its numpy restatement, single-bit
sensitivity, the errors, isolation, and the trainer resuming to the parameters of the uninterrupted run.
Every comparison is bit equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import checkpoint_ref as cr
import hashfill as hf
from conftest import ROOT
from shared_fixtures import trainer  # noqa: F401
from __graft_entry__ import load_package

T, A = 4, 4
BASE = "total_environments: 8\nhidden_size: 32\nhorizon: 8\nnum_mini_batches: 4\nnum_rollouts: 4\ndeterministic: true\n" \
       "num_workers: 2\n"


# ------------------------------------------------------------------ CPU: the restatement
def _splitmix_py(x):
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_reference_digest_of_three_words_by_hand():
    """D(tag, w) written out with Python integers; splitmix64(0) is the first output of the published generator"""
    assert _splitmix_py(0) == 0xE220A8397B1DCDAF
    w = [0x00000000, 0xFFFFFFFF, 0x3F800000]
    for tag in (1, 5):
        want = sum(_splitmix_py(_splitmix_py(tag) ^ ((i << 32) | x)) for i, x in enumerate(w)) & ((1 << 64) - 1)
        assert cr.D(tag, np.array(w, np.uint32)) == want
    # the sections are built from it: one parameter 1.0f, moments 0, step 3
    p = np.array([1.0], np.float32)
    assert cr.params(p) == _splitmix_py(_splitmix_py(1) ^ 0x3F800000)
    z = np.zeros(1, np.float32)
    assert cr.optimizer(z, z, 3) == (_splitmix_py(_splitmix_py(2)) + _splitmix_py(_splitmix_py(3)) +
                                     _splitmix_py(_splitmix_py(4) ^ 3)) & ((1 << 64) - 1)
    # order matters (the index is hashed in), and a double enters as its low then its high word
    assert cr.D(1, np.array([1, 2], np.uint32)) != cr.D(1, np.array([2, 1], np.uint32))
    lo, hi = struct.unpack("<II", struct.pack("<d", 1e-4))
    assert cr.reward_scale([1e-4], []) == (_splitmix_py(_splitmix_py(7) ^ lo) +
                                           _splitmix_py(_splitmix_py(7) ^ ((1 << 32) | hi))) & ((1 << 64) - 1)
    obs = np.zeros((1, 4, 84, 84), np.uint8)
    obs[0, :, 0, 1] = (1, 2, 3, 4)
    s = np.zeros(7056, np.uint32)
    s[1] = 0x04030201
    assert cr.rollout(obs, 9) == (cr.D(5, s) + _splitmix_py(_splitmix_py(6) ^ 9)) & ((1 << 64) - 1)


# ------------------------------------------------------------------ CPU: the trainer's keys and the file
@pytest.fixture(scope="module")
def trainer_tsan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_tsan"])
    return os.path.join(ROOT, "trainer", "train_tsan")


@pytest.fixture(scope="module")
def trainer_stub():
    """trainer/train.cc against tests/stub/aleppo_stub_state.cc: the existing stand-in plus host-only checkpoint entry points"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_ckpt_stub"])
    return os.path.join(ROOT, "trainer", "train_ckpt_stub")


def _run(exe, tmp_path, extra, env=None, base=BASE, name="c.yaml"):
    cfg = tmp_path / name
    cfg.write_text(base + extra)
    return subprocess.run([exe, "rom.bin", str(tmp_path / "x.log"), str(tmp_path), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_checkpoint_keys_are_refused_when_the_config_is_loaded(trainer, tmp_path):
    r = _run(trainer, tmp_path, "checkpoint_interval: 2\n")
    assert r.returncode == 1 and "checkpoint_interval needs checkpoint_path" in r.stderr, r.stderr
    for bad in ("0", "-3"):
        r = _run(trainer, tmp_path, f"checkpoint_path: {tmp_path / 'ck.bin'}\ncheckpoint_interval: {bad}\n")
        assert r.returncode == 1 and "checkpoint_interval must be positive" in r.stderr, r.stderr
    r = _run(trainer, tmp_path, f"resume: {tmp_path / 'nope.bin'}\n")
    assert r.returncode == 1 and "cannot open checkpoint" in r.stderr and "nope.bin" in r.stderr, r.stderr
    junk = tmp_path / "junk.bin"
    junk.write_bytes(b"NOTACKPT" + bytes(200))
    r = _run(trainer, tmp_path, f"resume: {junk}\n")
    assert r.returncode == 1 and "wrong magic" in r.stderr, r.stderr
    junk.write_bytes(b"ALEPPOCK" + struct.pack("<I", 99) + bytes(200))
    r = _run(trainer, tmp_path, f"resume: {junk}\n")
    assert r.returncode == 1 and "format version 99" in r.stderr, r.stderr
    junk.write_bytes(b"ALEPPO")
    r = _run(trainer, tmp_path, f"resume: {junk}\n")
    assert r.returncode == 1 and "truncated" in r.stderr, r.stderr
    # valid keys pass load_config (the run then stops at the initial-parameter dump: no GPU needed)
    r = _run(trainer, tmp_path, f"checkpoint_path: {tmp_path / 'ck.bin'}\ncheckpoint_interval: 2\n",
             env=dict(ALEPPO_TRAINER_DUMP_INIT=str(tmp_path / "i.bin")))
    assert r.returncode == 0, r.stderr


def test_library_without_the_entry_points_refuses_the_three_keys(trainer_tsan, tmp_path):
    for extra in (f"checkpoint_path: {tmp_path / 'ck.bin'}\n",
                  f"checkpoint_path: {tmp_path / 'ck.bin'}\ncheckpoint_interval: 1\n",
                  f"resume: {tmp_path / 'ck.bin'}\n"):
        r = _run(trainer_tsan, tmp_path, extra)
        assert r.returncode != 0 and "aleppo_export_rollout_state is missing" in r.stderr, r.stderr
        assert not (tmp_path / "ck.bin").exists()


def _final(stdout):
    return re.search(r"steps (\d+) episodes (\d+)", stdout).groups()


def test_checkpoint_file_round_trip_and_refusals_without_a_gpu(trainer_stub, tmp_path):
    """the host-only build: an interrupted and resumed run ends where the uninterrupted one does, down to the checkpoint
    file it leaves after the last rollout; the file appears under its final name only, whole; truncated / corrupt / other-shape files and a digest that does not match are refused"""
    ck = tmp_path / "run.ckpt"
    full = _run(trainer_stub, tmp_path, f"checkpoint_path: {tmp_path / 'full.ckpt'}\ncheckpoint_interval: 2\n",
                env=dict(ALEPPO_TRAINER_DUMP_FINAL=str(tmp_path / "full.bin")))
    assert full.returncode == 0 and "Success" in full.stdout, full.stderr[-2000:]
    (tmp_path / "run.ckpt.tmp").write_bytes(b"a leftover of an interrupted write")
    keys = f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n"
    part = _run(trainer_stub, tmp_path, keys, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert part.returncode == 0 and "stopped after the checkpoint of rollout 2" in part.stdout, part.stderr[-2000:]
    assert "Rollout 3 of 4" not in part.stdout
    assert re.search(r"checkpoint rollout 2 digest params=[0-9a-f]{16} optimizer=[0-9a-f]{16} rollout=[0-9a-f]{16} "
                     r"reward_scale=[0-9a-f]{16}", part.stdout)
    assert ck.exists() and not (tmp_path / "run.ckpt.tmp").exists()
    blob = ck.read_bytes()
    assert blob[:8] == b"ALEPPOCK" and blob[-8:] == b"ALEPPOEN" and struct.unpack("<I", blob[8:12])[0] == 1
    assert struct.unpack("<8I", blob[12:44])[:7] == (8, 8, 4, 32, 0, 1, 0)  # E T A H precision world rank
    res = _run(trainer_stub, tmp_path, keys + f"resume: {ck}\n",
               env=dict(ALEPPO_TRAINER_DUMP_FINAL=str(tmp_path / "resumed.bin")))
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert "at rollout 2 of 4, state digest verified" in res.stdout
    assert "Rollout 3 of 4" in res.stdout and "Rollout 2 of 4" not in res.stdout and "Rollout 4 of 4" in res.stdout
    assert _final(res.stdout) == _final(full.stdout)
    assert (tmp_path / "resumed.bin").read_bytes() == (tmp_path / "full.bin").read_bytes()
    assert "checkpoint rollout 4 digest" in res.stdout  # (after the last rollout too; the file now continues at 4)
    # ... and is, byte for byte, the file the uninterrupted run left after rollout 4: what the reader restores is what the
    # writer wrote, for every field
    assert ck.read_bytes() == (tmp_path / "full.ckpt").read_bytes()
    # a checkpoint that cannot be written is an error, and nothing is left under the final name
    gone = tmp_path / "no_such_dir" / "x.ckpt"
    r = _run(trainer_stub, tmp_path, f"checkpoint_path: {gone}\ncheckpoint_interval: 1\n")
    assert r.returncode == 1 and "cannot write checkpoint" in r.stderr and not gone.exists()
    # refusals: every one before the run starts
    bad = tmp_path / "bad.ckpt"
    for cut in (len(blob) - 1, len(blob) - 8, len(blob) // 2, 30, 11):
        bad.write_bytes(blob[:cut])
        r = _run(trainer_stub, tmp_path, f"resume: {bad}\n")
        assert r.returncode == 1 and "truncated" in r.stderr and "Rollout" not in r.stdout, (cut, r.stderr)
    bad.write_bytes(blob + b"\0")
    r = _run(trainer_stub, tmp_path, f"resume: {bad}\n")
    assert r.returncode == 1 and "resume:" in r.stderr and "Rollout" not in r.stdout, r.stderr
    sec_len_at = 44 + 8 + 4  # magic, version, shape header (40 bytes), then section 1's id and its length
    bad.write_bytes(blob[:sec_len_at] + struct.pack("<Q", 16) + blob[sec_len_at + 8:])
    r = _run(trainer_stub, tmp_path, f"resume: {bad}\n")
    assert r.returncode == 1 and "resume:" in r.stderr and "Rollout" not in r.stdout, r.stderr
    for key, val, what in (("total_environments", 16, "total_environments"), ("horizon", 16, "horizon"),
                           ("action_size", 6, "action_size"), ("hidden_size", 64, "hidden_size"),
                           ("precision", "bf16", "precision")):
        base = re.sub(rf"(?m)^{key}: .*\n", "", BASE) + f"{key}: {val}\n"
        r = _run(trainer_stub, tmp_path, f"resume: {ck}\n", base=base)
        assert r.returncode == 1 and f"was written for {what}" in r.stderr and "Rollout" not in r.stdout, r.stderr
    r = _run(trainer_stub, tmp_path, f"resume: {ck}\n", env=dict(WORLD_SIZE="2", RANK="1"),
             base=BASE.replace("total_environments: 8", "total_environments: 16"))
    assert r.returncode == 1 and "cannot open checkpoint" in r.stderr and "run.ckpt.rank1" in r.stderr, r.stderr
    os.link(ck, str(ck) + ".rank1")
    r = _run(trainer_stub, tmp_path, f"resume: {ck}\n", env=dict(WORLD_SIZE="2", RANK="1"),
             base=BASE.replace("total_environments: 8", "total_environments: 16"))
    assert r.returncode == 1 and "was written for WORLD_SIZE = 1" in r.stderr, r.stderr
    # a state that does not hash to what the file recorded is fatal, and the message names the section
    part2 = _run(trainer_stub, tmp_path, f"checkpoint_path: {tmp_path / 'two.ckpt'}\ncheckpoint_interval: 2\n",
                 env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert part2.returncode == 0
    for k, name in enumerate(("params", "optimizer", "rollout", "reward_scale")):
        r = _run(trainer_stub, tmp_path, f"resume: {tmp_path / 'two.ckpt'}\n", env=dict(ALEPPO_STUB_DIGEST_FLIP=str(k)))
        assert r.returncode == 1 and f"the {name} digest after the import" in r.stderr and "Rollout" not in r.stdout, r.stderr


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _term(g, E):  # terminal flags of global slot g (a fixed pattern, so that nothing of it has to be carried)
    return (((g * 7 + np.arange(E) * 3) % 11) == 0).astype(np.uint8)


def _start(g, E):
    return np.ones(E, np.uint8) if g == 0 else _term(g - 1, E)


class _Run:
    """drives one Engine through rollouts whose environment is a function of (global slot, actions)"""

    def __init__(self, pkg, E, H=32, prec=None, mode="step", kind=None, opts=(), seed=11):
        self.pkg, self.E, self.mode = pkg, E, mode
        self.kind = pkg.FRAMES_84 if kind is None else kind
        self.eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec is None else prec, seed=seed)
        self.eng.load_params(hf.fill_params(310, H, A))
        for o in opts:
            if o == "reward_scale":
                self.eng.set_reward_scaling(True)
            else:
                self.eng.set_option(o, 1)
        self.per = 2 * 210 * 160 if self.kind == pkg.FRAMES_RAW_PAIR else 84 * 84
        if mode == "arm":
            self.f_addr, self.s_addr = self.eng.host_alloc(E * self.per), self.eng.host_alloc(E)
            self.f_map = np.ctypeslib.as_array((C.c_uint8 * (E * self.per)).from_address(self.f_addr))
            self.s_map = np.ctypeslib.as_array((C.c_uint8 * E).from_address(self.s_addr))

    def slot(self, g, after_act=None):
        E = self.E
        actions = self.eng.act().copy()
        start, term = _start(g, E), _term(g, E) * (1 - _start(g, E))
        frames = np.random.default_rng(1000 + g).integers(0, 256, E * self.per, dtype=np.uint8)
        rewards = ((actions + np.arange(E)) % 3).astype(np.float32)
        zeros = np.zeros(E, np.uint8)
        if self.mode == "arm":
            self.eng.arm_step(self.f_addr, self.s_addr, self.kind)
            if after_act:
                after_act()
            self.f_map[:] = frames
            self.s_map[:] = start
            self.eng.release_step(rewards, term, zeros)
        else:
            if after_act:
                after_act()
            self.eng.step(frames, rewards, term, zeros, start, kind=self.kind)
        return actions

    def rollout(self, k):
        acts = np.stack([self.slot(k * T + t) for t in range(T)])
        self.eng.finish_rollout()
        out = {n: self.eng.read_batch(n) for n in ("observations", "actions", "logits", "values", "advantages", "returns",
                                                   "rewards", "masks", "current_obs")}
        out["acted"] = acts
        return out

    def train(self, k):
        m = self.eng.train(2.5e-4 * (1 - k / 4), 2, 2)
        sd = self.eng.state_dict()
        return dict(metrics=m, params=sd["params"], exp_avg=sd["exp_avg"], exp_avg_sq=sd["exp_avg_sq"], step=int(sd["step"]))

    def close(self):
        if self.mode == "arm":
            self.eng.host_free(self.f_addr)
            self.eng.host_free(self.s_addr)
        self.eng.close()


def _same(a, b, what):
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], f"{what}.{k}")
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
            assert x.tobytes() == y.tobytes(), f"{what}.{k} differs"


def _differs(a, b):
    return any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() for k in a if not isinstance(a[k], dict))


CASES = {
    "fp32-step-84-E1": dict(E=1),
    "fp32-step-84-E5": dict(E=5),
    "fp32-step-84-E130": dict(E=130),
    "bf16-step-84": dict(E=5, prec="bf16"),
    "bf16-arm-84": dict(E=5, prec="bf16", mode="arm"),
    "fp32-arm-raw": dict(E=5, mode="arm", raw=True),
    "bf16-step-raw": dict(E=5, prec="bf16", raw=True),
    "fp32-reward-scale": dict(E=5, opts=("reward_scale",)),
    "fp32-shuffle": dict(E=5, opts=("shuffle",)),
    "bf16-graph": dict(E=5, prec="bf16", opts=("graph",)),
}


def _make(pkg, case):
    c = CASES[case]
    names = dict(shuffle=pkg.OPT_MINIBATCH_SHUFFLE, graph=pkg.OPT_UPDATE_GRAPH)
    return _Run(pkg, c["E"], prec=pkg.BF16 if c.get("prec") == "bf16" else pkg.FP32, mode=c.get("mode", "step"),
                kind=pkg.FRAMES_RAW_PAIR if c.get("raw") else pkg.FRAMES_84,
                opts=tuple(names.get(o, o) for o in c.get("opts", ())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_resumed_context_continues_bit_for_bit(pkg, case):
    """A: rollout 1, train, rollout 2, train.  B: rollout 1, train, export, destroyed.  C: fresh, import, rollout 2, train.
    Rollout 2 and its update are bit-identical in A and C, and so are the digests at every point; without the rollout
    state (the control) they are not."""
    a = _make(pkg, case)
    a.rollout(0), a.train(0)
    dg_a1 = a.eng.state_digest()
    ra, ta = a.rollout(1), a.train(1)
    dg_a2 = a.eng.state_digest()
    a.close()
    b = _make(pkg, case)
    b.rollout(0), b.train(0)
    sd = b.eng.run_state()
    assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step", "reward_scale", "rollout"}
    assert b.eng.state_digest() == dg_a1 == cr.digest(sd)
    b.close()
    c = _make(pkg, case)
    c.eng.load_run_state(sd)
    assert c.eng.state_digest() == dg_a1
    rc_, tc = c.rollout(1), c.train(1)
    assert c.eng.state_digest() == dg_a2
    c.close()
    _same(ra, rc_, "rollout 2")
    _same(ta, tc, "update 2")
    # control: the learner state alone (what state_dict carried before) gives another rollout
    d = _make(pkg, case)
    d.eng.load_state_dict(sd)
    assert d.eng.state_digest()["rollout"] != dg_a1["rollout"]
    rd = d.rollout(1)
    d.close()
    assert _differs(ra, rd)


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 5, 130])
def test_rollout_state_round_trip(pkg, E):
    a = _Run(pkg, E)
    st = a.eng.rollout_state()
    assert st["counter"] == 0 and st["observations"].shape == (E, 4, 84, 84) and not st["observations"].any()
    r = a.rollout(0)
    st = a.eng.rollout_state()
    assert st["counter"] == T + 1  # T acts and the bootstrap forward
    assert st["observations"].tobytes() == r["current_obs"].tobytes() and st["observations"].any()
    batch_obs = r["observations"]
    a.eng.load_rollout_state(st)  # into the exporting context itself: the batch it still holds is left alone
    assert a.eng.read_batch("observations").tobytes() == batch_obs.tobytes()
    a.close()
    b = _Run(pkg, E)
    b.eng.load_rollout_state(st)
    st2 = b.eng.rollout_state()
    assert st2["counter"] == st["counter"] and st2["observations"].tobytes() == st["observations"].tobytes()
    assert b.eng.read_batch("current_obs").tobytes() == st["observations"].tobytes()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("E", [1, 5, 130])
def test_digest_equals_the_restatement_on_the_exported_state(pkg, E, H):
    a = _Run(pkg, E, H=H, opts=("reward_scale",))
    for k in range(3):  # after zero, one and two updates
        sd = a.eng.run_state()
        assert a.eng.state_digest() == cr.digest(sd), f"after {k} updates"
        assert int(sd["step"]) == 4 * k and sd["rollout"]["counter"] == (T + 1) * k
        if k < 2:
            a.rollout(k), a.train(k)
    a.close()


def _flip(arr, i):
    v = np.ascontiguousarray(arr).copy()
    w = v.reshape(-1).view(np.uint8)
    w[i] ^= 1
    return v


@pytest.mark.gpu
def test_one_flipped_bit_changes_its_section_and_no_other(pkg):
    a = _Run(pkg, 5, opts=("reward_scale",))
    a.rollout(0), a.train(0)
    sd = a.eng.run_state()
    base = a.eng.state_digest()
    assert base == cr.digest(sd)
    ro, rs = sd["rollout"], sd["reward_scale"]
    flips = {
        "stack byte": ("rollout", dict(sd, rollout=dict(ro, observations=_flip(ro["observations"], 3 * 28224 + 2 * 7056 + 100)))),
        "counter": ("rollout", dict(sd, rollout=dict(ro, counter=ro["counter"] + 1))),
        "parameter": ("params", dict(sd, params=_flip(sd["params"], 4 * 1234))),
        "moment": ("optimizer", dict(sd, exp_avg_sq=_flip(sd["exp_avg_sq"], 4 * 77))),
        "step": ("optimizer", dict(sd, step=np.int64(int(sd["step"]) + 1))),
        "G": ("reward_scale", dict(sd, reward_scale=dict(rs, returns=_flip(rs["returns"], 8 * 2)))),
    }
    for what, (section, mod) in flips.items():
        a.eng.load_run_state(mod)
        got = a.eng.state_digest()
        assert got == cr.digest(mod), what
        assert {k for k in got if got[k] != base[k]} == {section}, what
    a.eng.load_run_state(sd)
    assert a.eng.state_digest() == base
    a.close()


@pytest.mark.gpu
def test_errors_and_a_failed_call_changes_nothing(pkg):
    E = 5
    lib = pkg.lib()
    obs, words, dg = np.zeros((E, 4, 84, 84), np.uint8), np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def calls(ctx, n=E, o=obs, w=words, d=dg):
        return (lib.aleppo_export_rollout_state(ctx, None if o is None else p(o), None if w is None else p(w), C.c_size_t(n)),
                lib.aleppo_import_rollout_state(ctx, None if o is None else p(o), None if w is None else p(w), C.c_size_t(n)),
                lib.aleppo_state_digest(ctx, None if d is None else p(d)))

    # invalid arguments between rollouts: the digest before equals the digest after
    x = _Run(pkg, E, mode="arm")
    x.rollout(0)
    before, st = x.eng.state_digest(), x.eng.rollout_state()
    assert calls(x.eng._ctx, n=E + 1)[:2] == (pkg.ERR_INVALID_ARGUMENT,) * 2
    assert calls(x.eng._ctx, o=None, d=None) == (pkg.ERR_INVALID_ARGUMENT,) * 3
    assert calls(x.eng._ctx, w=None)[:2] == (pkg.ERR_INVALID_ARGUMENT,) * 2
    for k in (1, 2, 3):
        w = np.zeros(4, np.uint64)
        w[k] = 1
        assert lib.aleppo_import_rollout_state(x.eng._ctx, p(obs), p(w), C.c_size_t(E)) == pkg.ERR_INVALID_ARGUMENT
    assert x.eng.state_digest() == before
    after = x.eng.rollout_state()
    assert after["counter"] == st["counter"] and after["observations"].tobytes() == st["observations"].tobytes()
    # mid-rollout and while armed: ALEPPO_ERR_RUNTIME from all three, and the run goes on as the twin's that never asked
    y = _Run(pkg, E, mode="arm")
    y.rollout(0)
    seen = []
    for t in range(T):
        x.slot(T + t, after_act=lambda: seen.append(calls(x.eng._ctx)))  # armed
        if t < T - 1:
            seen.append(calls(x.eng._ctx))  # t != 0, nothing armed
        y.slot(T + t)
    assert len(seen) == 2 * T - 1 and all(s == (pkg.ERR_RUNTIME,) * 3 for s in seen), seen
    with pytest.raises(pkg.AleppoError, match="between rollouts"):  # (the buffer is full but not finished: t = T)
        x.eng.state_digest()
    x.eng.finish_rollout(), y.eng.finish_rollout()
    assert x.eng.state_digest() == y.eng.state_digest()
    x.close(), y.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_export_and_digest_calls_do_not_change_the_run(pkg, prec):
    P = pkg.BF16 if prec == "bf16" else pkg.FP32
    a, b = _Run(pkg, 5, prec=P), _Run(pkg, 5, prec=P)
    b.eng.run_state(), b.eng.state_digest()
    for k in range(3):
        ra, ta = a.rollout(k), a.train(k)
        rb, tb = b.rollout(k), b.train(k)
        b.eng.run_state(), b.eng.state_digest(), b.eng.rollout_state()
        _same(ra, rb, f"rollout {k}")
        _same(ta, tb, f"update {k}")
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", ["true", "false"])
def test_trainer_resumes_to_the_parameters_of_the_uninterrupted_run(trainer, tmp_path, ahead):
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read().replace("num_rollouts: 10", "num_rollouts: 4")
    txt += f"slot_ahead: {ahead}\n"
    ck = tmp_path / "run.ckpt"

    def run(name, extra, env):
        d = tmp_path / name
        os.makedirs(d / "tb")
        cfg = d / "debug.yaml"
        cfg.write_text(txt + extra)
        r = subprocess.run([trainer, "breakout.bin", str(d / "tb" / "run.log"), str(d), "grp", str(cfg)], capture_output=True,
                           text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    full = run("full", "", dict(ALEPPO_TRAINER_DUMP_FINAL=str(tmp_path / "full.bin")))
    keys = f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n"
    part = run("part", keys, dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert "stopped after the checkpoint of rollout 2" in part and "Rollout 3 of 4" not in part
    line = re.search(r"checkpoint rollout 2 digest (params=[0-9a-f]{16} optimizer=[0-9a-f]{16} rollout=[0-9a-f]{16} "
                     r"reward_scale=[0-9a-f]{16})", part)
    assert line and ck.exists() and not os.path.exists(str(ck) + ".tmp")
    blob = ck.read_bytes()  # (the resumed run writes its own checkpoints over it)
    res = run("res", keys + f"resume: {ck}\n", dict(ALEPPO_TRAINER_DUMP_FINAL=str(tmp_path / "res.bin")))
    assert "at rollout 2 of 4, state digest verified" in res
    assert "Rollout 3 of 4" in res and "Rollout 4 of 4" in res and "Rollout 2 of 4" not in res and "Success" in res
    assert _final(res) == _final(full) and int(_final(full)[1]) > 0
    assert (tmp_path / "res.bin").read_bytes() == (tmp_path / "full.bin").read_bytes()
    # the digest the rollout-2 file carries is the restatement's, computed from the file's own sections
    secs, pos = {}, 52
    while blob[pos:] != b"ALEPPOEN":
        sid, n = struct.unpack("<IQ", blob[pos:pos + 12])
        secs[sid] = blob[pos + 12:pos + 12 + n]
        pos += 12 + n
    npar = len(secs[1]) // 4
    opt = np.frombuffer(secs[2][:8 * npar], np.float32)
    rs = np.frombuffer(secs[3], np.float64)
    want = dict(params=cr.params(np.frombuffer(secs[1], np.float32)),
                optimizer=cr.optimizer(opt[:npar], opt[npar:], struct.unpack("<q", secs[2][8 * npar:])[0]),
                rollout=cr.rollout(np.frombuffer(secs[4][32:], np.uint8).reshape(8, 4, 84, 84),
                                   struct.unpack("<Q", secs[4][:8])[0]),
                reward_scale=cr.reward_scale(rs[:3], rs[3:]))
    got = dict(zip(("params", "optimizer", "rollout", "reward_scale"), struct.unpack("<4Q", secs[6])))
    assert got == want
    assert line.group(1) == " ".join(f"{k}={v:016x}" for k, v in got.items())
