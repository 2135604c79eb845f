"""CPU: tests/device_env_ref.py (the numpy reference of the device-resident environments) against trainer/emulator.hpp
ITSELF.  tests/tools/device_env_driver.cc is compiled here and runs the header on scripted actions; every frame, record
entry, episode-log entry and the final state must agree byte for byte.  The same driver runs the plain-C++ half of
csrc/env_synth.hpp - the game logic and the per-pixel renderers env_step_kernel is made of - next to the header and fails
on the first difference, so the kernel's arithmetic is checked here without a GPU as well."""
import os
import subprocess

import numpy as np
import pytest

import device_env_ref as ref
from conftest import ROOT
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("envdrv") / "device_env_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "tools", "device_env_driver.cc"), "-o", exe])
    return exe


def scripted_actions(T, E, seed):
    """a paddle that follows a drifting target for stretches, then idles: rallies of different lengths"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (T, E)).astype(np.int32)
    a[T // 3: T // 2] = 2   # hard right: the paddle reaches 79
    a[T // 2: 2 * T // 3] = 3  # hard left: it reaches 4
    return a


CASES = [  # raw, max_steps, max_return, E, T
    pytest.param(False, 108000, -1.0, 5, 400, id="84-life-loss"),
    pytest.param(True, 108000, -1.0, 3, 120, id="raw-life-loss"),
    pytest.param(False, 40, -1.0, 3, 50, id="84-max-steps-40"),
    pytest.param(True, 40, -1.0, 2, 30, id="raw-max-steps-40"),
    pytest.param(False, 108000, 6.0, 4, 200, id="84-max-return-6"),
    pytest.param(True, 108000, 6.0, 2, 90, id="raw-max-return-6"),
]


@pytest.mark.parametrize("raw,max_steps,max_return,E,T", CASES)
def test_reference_equals_the_header(driver, tmp_path, raw, max_steps, max_return, E, T):
    pkg = load_package()
    actions = scripted_actions(T, E, 7 + E + T)
    actions.tofile(tmp_path / "a.bin")
    seed_base = 11
    subprocess.check_call([driver, str(int(raw)), str(max_steps), repr(max_return), str(E), str(T), str(seed_base),
                           str(tmp_path / "a.bin"), str(tmp_path / "o.bin")])
    blob = np.fromfile(tmp_path / "o.bin", np.uint8)
    fb = 2 * 210 * 160 if raw else 84 * 84
    per_slot = E * (fb + 4 + 4 + 4 * 4)
    assert blob.size == T * per_slot + E * pkg.ENV_STATE_DTYPE.itemsize
    envs = ref.EnvSet(E, seed_base, max_steps, max_return, raw)
    seen = dict(term=0, trunc=0, game_over=0)
    for t in range(T):
        s = blob[t * per_slot:(t + 1) * per_slot]
        o = envs.step(actions[t])
        pos = 0

        def take(n, dt=np.uint8):
            nonlocal pos
            v = s[pos:pos + n].view(dt)
            pos += n
            return v
        assert np.array_equal(take(E * fb), o.frames.ravel()), f"frames differ in slot {t}"
        assert take(4 * E).tobytes() == o.rewards.tobytes(), t
        for name in ("term", "trunc", "start", "game_over"):
            assert np.array_equal(take(E), getattr(o, name)), (name, t)
        assert take(4 * E).tobytes() == o.ep_ret.tobytes(), t
        assert np.array_equal(take(4 * E, np.uint32), o.ep_len), t
        assert take(4 * E).tobytes() == o.game_ret.tobytes(), t
        assert np.array_equal(take(4 * E, np.uint32), o.game_len), t
        seen["term"] += int(o.term.sum())
        seen["trunc"] += int(o.trunc.sum())
        seen["game_over"] += int((o.game_len > 0).sum())
    final = blob[T * per_slot:].view(pkg.ENV_STATE_DTYPE)
    assert final.tobytes() == envs.state(pkg.ENV_STATE_DTYPE).tobytes()
    # the branch each case is there for occurred
    if max_steps == 40:  # 10 agent steps of 4 frames, whatever the actions: reset slot + 10 steps per episode
        assert seen["trunc"] == E * ((T - 1) // 11) and seen["term"] == 0 and seen["game_over"] == seen["trunc"]
    elif max_return > 0:
        assert seen["trunc"] >= E and seen["game_over"] >= seen["trunc"]  # (a truncation ends the game)
    else:
        assert seen["term"] >= E and seen["trunc"] == 0
        print("terminals", seen["term"], "game overs", seen["game_over"])


@pytest.mark.parametrize("raw", [False, True], ids=["84", "raw"])
def test_per_pixel_renderers_equal_the_header_on_hand_made_states(driver, raw):
    """every ball position (83 included, where the ball is clipped), the paddle at 4 and 79, every brick phase"""
    out = subprocess.run([driver, "sweep", str(int(raw))], capture_output=True, text=True)
    assert out.returncode == 0 and "sweep ok" in out.stdout, out.stderr


def test_state_struct_is_88_bytes_in_the_header_order():
    pkg = load_package()
    dt = pkg.ENV_STATE_DTYPE
    assert dt.itemsize == 88
    assert [dt.fields[k][1] for k in ("rng", "steps", "ep_len", "game_len", "lives", "bricks", "episode_return", "reward",
                                      "game_ret", "start", "game_over", "reserved")] == [0, 8, 16, 24, 32, 64, 68, 72, 80, 84,
                                                                                         85, 86]
    import ctypes as C
    assert C.sizeof(pkg.EnvConfig) == 32 and pkg.EnvConfig.max_return.offset == 24
