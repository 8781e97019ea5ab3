"""Catch (Catch-v0), numpy restatement.  Test infrastructure only (imported by
tests/test_catch_cpu.py and tests/test_gpu_catch.py).

The rules, as include/a3c_hip.h states them: an 8-column, 10-row board; state = ball column c, ball
row r, paddle column p, which *is* the pool frame index f = (c*ROWS + r)*COLS + p < 640; ep_step = r,
ep_len = ROWS-1, lives = 0.  reset: episode += 1, (x0, x1, ..) = philox(episode, id, P_RESET, 0),
c = x0 % COLS, p = x1 % COLS, r = 0, reward 0, terminal 0; new_game and new_random_game are the
reset.  step(a): r += 1, p = clamp(p + (a == 2) - (a == 1)), landing = r == ROWS-1, reward = +1 / -1
at the landing (paddle under the ball or not) else 0, terminal = landing; a step on a landed state
changes nothing and returns reward 0, terminal 1.  act: the repeat loop of GymEnvironment.act
(environment.py:78-96) -- sum the rewards, stop at a terminal.

CatchEnv has oracle.synthetic_env.SyntheticAtari's interface, stepped one raw step at a time (the
kernels split the act around the action draw instead); CatchEngineRef is oracle.engine_ref.EngineRef
on it.  random_policy_return() is the exact expected return of the uniformly random policy."""
from fractions import Fraction

import numpy as np

from oracle import philox as px
from oracle import ref_cpu as R
from oracle.engine_ref import EngineRef

COLS, ROWS = 8, 10
FRAMES = COLS * ROWS * COLS          # 640
ACTIONS = 3                          # 0 stay, 1 left, 2 right
CELL_W, CELL_H = 20, 21              # 8 x 20 = 160, 10 x 21 = 210
BALL_RGB, PADDLE_RGB = (236, 236, 236), (92, 186, 92)


def encode(c, r, p):
    return (np.asarray(c) * ROWS + np.asarray(r)) * COLS + np.asarray(p)


def decode(f):
    f = np.asarray(f)
    return f // (ROWS * COLS), (f // COLS) % ROWS, f % COLS


def render(f):
    """Frame f of the pool, u8 [210, 160, 3]: black, the ball's cell, then the paddle over it."""
    c, r, p = (int(v) for v in decode(int(f)))
    img = np.zeros((210, 160, 3), np.uint8)
    img[CELL_H * r:CELL_H * r + CELL_H, CELL_W * c:CELL_W * c + CELL_W] = BALL_RGB
    img[200:210, CELL_W * p:CELL_W * p + CELL_W] = PADDLE_RGB
    return img


def step_state(f, a):
    """One raw step of state f under action a: (f', reward, terminal)."""
    c, r, p = (int(v) for v in decode(int(f)))
    if r == ROWS - 1:
        return int(f), 0.0, True
    r += 1
    p = min(max(p + (1 if a == 2 else 0) - (1 if a == 1 else 0), 0), COLS - 1)
    landing = r == ROWS - 1
    return int(encode(c, r, p)), ((1.0 if p == c else -1.0) if landing else 0.0), landing


def random_policy_return():
    """Exact expected return of the uniformly random policy over the 64 equally likely reset states
    (2^32 is a multiple of COLS, so x % COLS is uniform), by dynamic programming over the paddle
    column: the ball only falls, so the return is 2 P(p_9 = c) - 1."""
    total = Fraction(0)
    for c in range(COLS):
        for p0 in range(COLS):
            dist = [Fraction(0)] * COLS
            dist[p0] = Fraction(1)
            for _ in range(ROWS - 1):
                nxt = [Fraction(0)] * COLS
                for p, w in enumerate(dist):
                    for d in (0, -1, 1):                      # stay, left, right
                        nxt[min(max(p + d, 0), COLS - 1)] += w / ACTIONS
                dist = nxt
            total += 2 * dist[c] - 1
    return total / (COLS * COLS)


R_RAND = float(random_policy_return())
LEARNING_BAR = R_RAND + 0.5 * (1.0 - R_RAND)      # halfway from random to optimal (+1)


class CatchEnv:
    """Vectorised over E envs with global ids ``ids`` (SyntheticAtari's fields and methods)."""

    def __init__(self, seed, num_envs, num_frames=FRAMES, action_size=ACTIONS, start_lives=0, random_start=30,
                 action_repeat=1, env_id_base=0):
        assert int(num_frames) >= FRAMES and int(action_size) == ACTIONS and int(start_lives) == 0
        self.seed = int(seed)
        self.k0, self.k1 = px.seed_key(seed)
        self.E, self.P, self.A, self.L0 = num_envs, int(num_frames), ACTIONS, 0
        self.random_start = int(random_start)       # ignored: the reset is the random start
        self.action_repeat = int(action_repeat)
        self.ids = np.arange(env_id_base, env_id_base + num_envs, dtype=np.uint32)
        self.episode = np.zeros(num_envs, np.uint32)
        self.ep_step = np.zeros(num_envs, np.uint32)
        self.ep_len = np.zeros(num_envs, np.uint32)
        self.lives = np.zeros(num_envs, np.int32)
        self.frame = np.zeros(num_envs, np.uint32)
        self.reward = np.zeros(num_envs, np.float32)
        self.terminal = np.zeros(num_envs, bool)

    def _reset(self, m):
        self.episode[m] += 1
        x0, x1, _, _ = px.philox4x32(self.episode, self.ids, px.P_RESET, 0, self.k0, self.k1)
        self.ep_step[m] = 0
        self.ep_len[m] = ROWS - 1
        self.lives[m] = 0
        self.frame[m] = encode(x0 % COLS, 0, x1 % COLS).astype(np.uint32)[m]
        self.reward[m] = 0
        self.terminal[m] = False

    def _step(self, action, m):
        action = np.broadcast_to(np.asarray(action, np.int64), (self.E,))
        for e in np.flatnonzero(m):
            f, rew, term = step_state(self.frame[e], int(action[e]))
            self.frame[e], self.reward[e], self.terminal[e] = f, rew, term
            self.ep_step[e] = decode(f)[1]
            self.ep_len[e] = ROWS - 1

    def new_game(self, m=None):
        self._reset(np.ones(self.E, bool) if m is None else np.asarray(m, bool))

    def new_random_game(self, m=None):
        self.new_game(m)

    def act(self, action, is_training=True):
        """GymEnvironment.act, environment.py:78-96 (no life is ever lost: is_training is moot).
        Returns (frame_idx, reward, terminal)."""
        cum = np.zeros(self.E, np.float32)
        active = np.ones(self.E, bool)
        for _ in range(self.action_repeat):
            self._step(action, active)
            cum = np.where(active, cum + self.reward, cum)
            active = active & ~self.terminal
            if not active.any():
                break
        self.reward = cum.astype(np.float32)
        return self.frame.copy(), self.reward.copy(), self.terminal.copy()

    def simple_act(self, action):
        self._step(action, np.ones(self.E, bool))
        return self.frame.copy(), self.reward.copy(), self.terminal.copy()

    def screens_rgb(self, frames=None):
        frames = self.frame if frames is None else frames
        return np.stack([render(int(f)) for f in frames])


class CatchEngineRef(EngineRef):
    """oracle.engine_ref.EngineRef playing Catch: the same replay on a CatchEnv, screens rendered."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        env = self.env
        self.env = CatchEnv(self.seed, self.E, max(env.P, FRAMES), env.A, env.L0, env.random_start, env.action_repeat,
                            int(env.ids[0]))
        self.ids = self.env.ids

    def _screen(self, f):
        return R.screen(render(int(f)))
