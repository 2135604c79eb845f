"""numpy restatement of trainer/emulator.hpp (SyntheticAtari, EnvSet::step) and of the slot bookkeeping of the trainer's
collect(): the reference the device-resident environments are compared with, byte for byte.  It is itself pinned against
emulator.hpp by tests/test_device_env_ref.py (a C++ driver runs the header on the same scripted actions).

The renderers are the header's memset + overdraw, NOT the per-pixel formulas of csrc/env_synth.hpp: the two
implementations share nothing but the specification."""
import numpy as np

M64 = (1 << 64) - 1
STATE_FIELDS = ("rng", "steps", "ep_len", "game_len", "lives", "paddle", "ball_x", "ball_y", "prev_x", "prev_y", "dx", "dy",
                "bricks", "episode_return", "reward", "ep_ret", "game_ret", "start", "game_over")
F32 = np.float32


def cdiv(a, b):
    """C's integer division: truncates toward zero"""
    q = abs(a) // b
    return q if a >= 0 else -q


class Env:
    """SyntheticAtari plus the trainer-side fields of one environment (TrainerState / EnvSet)"""

    def __init__(self, seed, max_steps, max_return, raw):
        self.rng = (seed * 0x9E3779B97F4A7C15 + 12345) & M64
        self.max_steps, self.max_return, self.raw = int(max_steps), F32(max_return), bool(raw)
        self.lives, self.paddle, self.ball_x, self.ball_y, self.prev_x, self.prev_y = 0, 42, 42, 60, 42, 60
        self.dx, self.dy, self.bricks, self.steps = 1, -1, 0, 0
        self.episode_return = F32(0)
        # trainer side
        self.start, self.game_over, self.reward = 1, 0, F32(0)
        self.ep_ret, self.game_ret, self.ep_len, self.game_len = F32(0), F32(0), 0, 0

    def next(self):
        r = self.rng
        r ^= (r << 13) & M64
        r ^= r >> 7
        r ^= (r << 17) & M64
        self.rng = r
        return r

    def reset(self):
        if self.lives == 0:
            self.lives, self.steps, self.episode_return, self.bricks = 5, 0, F32(0), 0
        self.ball_x, self.ball_y = 42, 60
        self.prev_x, self.prev_y = self.ball_x, self.ball_y
        self.dx = 1 if self.next() & 1 else -1
        self.dy = -1
        return self.render()

    def step(self, action):
        """-> (frame, reward, terminated, truncated, game_over)"""
        reward, terminated, truncated = F32(0), False, False
        self.paddle += 3 if action == 2 else -3 if action == 3 else 0
        self.paddle = min(max(self.paddle, 4), 79)
        for _ in range(4):
            self.prev_x, self.prev_y = self.ball_x, self.ball_y
            self.ball_x += self.dx * 2
            self.ball_y += self.dy * 2
            if self.ball_x <= 1 or self.ball_x >= 82:
                self.dx = -self.dx
            if self.ball_y <= 20:
                self.dy = 1
                reward = F32(reward + F32(1 + 3 * (self.bricks % 3 == 2)))
                self.bricks += 1
            if self.ball_y >= 78:
                if abs(self.ball_x - self.paddle) <= 8 or self.next() % 3 == 0:
                    self.dy = -1
                else:
                    self.lives -= 1
                    terminated = True
                    break
        self.steps += 4
        self.episode_return = F32(self.episode_return + reward)
        game_over = self.lives == 0
        if not terminated and (self.steps >= self.max_steps or
                               (self.max_return > 0 and self.episode_return >= self.max_return)):
            truncated = True
            self.lives = 0
            game_over = True
        return self.render(), reward, terminated, truncated, game_over

    def render(self):
        if self.raw:
            f = np.zeros((2, 210, 160), np.uint8)
            for k in range(2):
                g = f[k]

                def rect(x0, x1, y0, y1, c):
                    ya, yb = cdiv(y0 * 210, 84), cdiv(y1 * 210, 84)
                    xa, xb = cdiv(x0 * 160, 84), cdiv(x1 * 160, 84)
                    ya, yb, xa, xb = max(ya, 0), min(yb, 210), max(xa, 0), min(xb, 160)
                    if ya < yb and xa < xb:
                        g[ya:yb, xa:xb] = c
                for y in range(8, 20, 3):
                    for x in range(0, 84, 6):
                        rect(x, x + 6, y, y + 3, ((((x // 6 + y // 3 + self.bricks) % 4) * 50 + 60) & 0xFF) & ~1)
                rect(self.paddle - 6, self.paddle + 7, 80, 82, 200)
                bx, by = (self.prev_x, self.prev_y) if k == 0 else (self.ball_x, self.ball_y)
                rect(bx, bx + 2, by, by + 2, 236)
            return f
        f = np.zeros((84, 84), np.uint8)
        x = np.arange(84)
        for y in range(8, 20):
            f[y] = ((x // 6 + y // 3 + self.bricks) % 4) * 50 + 60
        xa, xb = max(self.paddle - 6, 0), min(self.paddle + 6, 83)
        f[80:82, xa:xb + 1] = 200
        ya, yb = max(self.ball_y, 0), min(self.ball_y + 2, 84)
        xa, xb = max(self.ball_x, 0), min(self.ball_x + 2, 84)
        if ya < yb and xa < xb:
            f[ya:yb, xa:xb] = 236
        return f


class Slot:
    """what one slot hands to aleppo_step, and what collect() appended to its episode log"""

    def __init__(self, E, fshape):
        self.frames = np.zeros((E,) + fshape, np.uint8)
        self.rewards = np.zeros(E, np.float32)
        self.term, self.trunc, self.start = (np.zeros(E, np.uint8) for _ in range(3))
        self.game_over = np.zeros(E, np.uint8)  # of the emulator's step (0 in a start slot)
        self.ep_ret, self.game_ret = np.zeros(E, np.float32), np.zeros(E, np.float32)
        self.ep_len, self.game_len = np.zeros(E, np.uint32), np.zeros(E, np.uint32)


class EnvSet:
    """E environments stepped the way the trainer's collect() steps them"""

    def __init__(self, E, seed_base=0, max_steps=108000, max_return=-1.0, raw=False):
        self.E, self.raw = E, raw
        self.fshape = (2, 210, 160) if raw else (84, 84)
        self.envs = [Env(seed_base + e, max_steps, max_return, raw) for e in range(E)]
        self.total_steps = self.episodes = 0

    def step(self, actions):
        o = Slot(self.E, self.fshape)
        for i, v in enumerate(self.envs):
            o.start[i] = v.start
            term = trunc = False
            if v.start:  # EnvSet::step: a start slot resets; the stale reward stays
                o.frames[i] = v.reset()
            else:
                o.frames[i], r, term, trunc, go = v.step(int(actions[i]))
                v.reward, v.game_over = r, int(go)
                v.ep_ret, v.game_ret = F32(v.ep_ret + r), F32(v.game_ret + r)
                v.ep_len += 1
                v.game_len += 1
                self.total_steps += 1
                o.game_over[i] = go
            o.rewards[i], o.term[i], o.trunc[i] = v.reward, term, trunc
            if term or trunc:
                v.start = 1
                self.episodes += 1
                o.ep_ret[i], o.ep_len[i] = v.ep_ret, v.ep_len
                v.ep_ret, v.ep_len = F32(0), 0
                if v.game_over:
                    o.game_ret[i], o.game_len[i] = v.game_ret, v.game_len
                    v.game_ret, v.game_len = F32(0), 0
            elif v.start:
                v.start = 0
        return o

    def state(self, dtype):
        """the environments as a structured array of the package's ENV_STATE_DTYPE"""
        st = np.zeros(self.E, dtype)
        for i, v in enumerate(self.envs):
            for k in STATE_FIELDS:
                st[k][i] = getattr(v, k)
        return st

    def load_state(self, st):
        for i, v in enumerate(self.envs):
            for k in STATE_FIELDS:
                x = st[k][i]
                setattr(v, k, F32(x) if st.dtype[k].kind == "f" else int(x))


def compact(slots):
    """the episode log of a list of slots in the order collect() appends: slot, then environment"""
    el = np.concatenate([s.ep_len for s in slots])
    gl = np.concatenate([s.game_len for s in slots])
    return (np.concatenate([s.ep_ret for s in slots])[el > 0], el[el > 0],
            np.concatenate([s.game_ret for s in slots])[gl > 0], gl[gl > 0])
