"""Catch with rule parameters (CatchMemory-v0), numpy restatement.  Test infrastructure
only (imported by tests/test_catch_memory_cpu.py and tests/test_gpu_catch_memory.py).

The rules, as include/a3c_hip.h states them, on top of tests/_catch_ref.py's Catch: visible_rows V in
1..10, frozen_rows F in 0..8; (10, 0) is Catch, CatchMemory-v0 is RULES = (1, 4).
  render: the ball's cell is drawn only in the frames of ball rows r < V; the paddle always is.
  step:   the paddle moves only if the row before the step is >= F; the row always advances.
  reset:  the same Philox draw; p = x1 % 8, M = 9 - F, lo = max(0, p - M), hi = min(7, p + M),
          c = lo + x0 % (hi - lo + 1).

The theorem (F >= V + 3, action_repeat 1): the first state whose action moves the paddle is the one at
row F, and its stack holds rows F-3 .. F, none of which shows the ball.  So the paddle's path under a
policy that is a function of the 4-frame stack does not depend on c given p, and its return is
2 P(c = q(p)) - 1 with q(p) the column the path ends in.  reset_distribution() is the exact law of
(c, p) under the Philox modulo, bias included; R_ML is the return with the bias dropped (c uniform over
its hi - lo + 1 columns), ml_return_bounds() the exact least and greatest return any such policy can
have with it (the least and the most likely column for every p)."""
from fractions import Fraction

import numpy as np

import _catch_ref as C
from oracle import philox as px
from oracle import ref_cpu as R

COLS, ROWS, FRAMES, ACTIONS = C.COLS, C.ROWS, C.FRAMES, C.ACTIONS
RULES = (1, 4)                       # CatchMemory-v0: (visible_rows, frozen_rows)
encode, decode = C.encode, C.decode


def reach(p, frozen):
    """(lo, hi): the columns the paddle at p can still reach in its 9 - frozen free steps."""
    m = ROWS - 1 - frozen
    return max(0, p - m), min(COLS - 1, p + m)


def render(f, visible=RULES[0]):
    """Frame f of the pool under the rules: Catch's, without the ball in rows >= visible."""
    c, r, p = (int(v) for v in decode(int(f)))
    if r < visible:
        return C.render(f)
    img = np.zeros((210, 160, 3), np.uint8)
    img[200:210, C.CELL_W * p:C.CELL_W * p + C.CELL_W] = C.PADDLE_RGB
    return img


def step_state(f, a, frozen=RULES[1]):
    """One raw step of state f under action a: (f', reward, terminal)."""
    c, r, p = (int(v) for v in decode(int(f)))
    if r == ROWS - 1:
        return int(f), 0.0, True
    if r >= frozen:
        p = min(max(p + (1 if a == 2 else 0) - (1 if a == 1 else 0), 0), COLS - 1)
    r += 1
    landing = r == ROWS - 1
    return int(encode(c, r, p)), ((1.0 if p == c else -1.0) if landing else 0.0), landing


def reset_distribution(frozen=RULES[1]):
    """{(c, p): probability} of a reset, exact: x1 % 8 is uniform (8 divides 2^32); x0 % m takes the
    value k for floor(2^32 / m) + (k < 2^32 % m) of the 2^32 words."""
    dist = {}
    for p in range(COLS):
        lo, hi = reach(p, frozen)
        m = hi - lo + 1
        q, rem = divmod(1 << 32, m)
        for k in range(m):
            dist[(lo + k, p)] = Fraction(1, COLS) * Fraction(q + (1 if k < rem else 0), 1 << 32)
    return dist


def memoryless_return(frozen=RULES[1]):
    """R_ML: 2 mean_p(1 / (hi - lo + 1)) - 1."""
    return 2 * sum(Fraction(1, reach(p, frozen)[1] - reach(p, frozen)[0] + 1) for p in range(COLS)) / COLS - 1


def ml_return_bounds(frozen=RULES[1]):
    """(least, greatest) exact return of a policy whose paddle path depends on p alone."""
    dist = reset_distribution(frozen)
    lo = hi = Fraction(0)
    for p in range(COLS):
        col = [w for (c, pp), w in dist.items() if pp == p]
        lo += 2 * min(col) - Fraction(1, COLS)
        hi += 2 * max(col) - Fraction(1, COLS)
    return lo, hi


R_ML = memoryless_return()                       # -121/168 = -0.7202380952...
LEARNING_BAR = R_ML + (1 - R_ML) / 2             # 47/336 = 0.1398809523...: halfway to the optimal +1


class CatchMemoryEnv(C.CatchEnv):
    """CatchEnv under the rules of the class attribute RULES (with_rules() makes other classes)."""
    RULES = RULES

    def _reset(self, m):
        self.episode[m] += 1
        x0, x1, _, _ = px.philox4x32(self.episode, self.ids, px.P_RESET, 0, self.k0, self.k1)
        p = (x1 % COLS).astype(np.int64)
        mm = ROWS - 1 - self.RULES[1]
        lo, hi = np.maximum(0, p - mm), np.minimum(COLS - 1, p + mm)
        c = lo + (x0.astype(np.int64) % (hi - lo + 1))
        self.ep_step[m] = 0
        self.ep_len[m] = ROWS - 1
        self.lives[m] = 0
        self.frame[m] = encode(c, 0, p).astype(np.uint32)[m]
        self.reward[m] = 0
        self.terminal[m] = False

    def _step(self, action, m):
        action = np.broadcast_to(np.asarray(action, np.int64), (self.E,))
        for e in np.flatnonzero(m):
            f, rew, term = step_state(self.frame[e], int(action[e]), self.RULES[1])
            self.frame[e], self.reward[e], self.terminal[e] = f, rew, term
            self.ep_step[e] = decode(f)[1]
            self.ep_len[e] = ROWS - 1

    def screens_rgb(self, frames=None):
        frames = self.frame if frames is None else frames
        return np.stack([render(int(f), self.RULES[0]) for f in frames])


class CatchMemoryEngineRef(C.CatchEngineRef):
    """oracle.engine_ref.EngineRef playing Catch under ENV.RULES."""
    ENV = CatchMemoryEnv

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        env = self.env
        self.env = self.ENV(self.seed, self.E, env.P, env.A, env.L0, env.random_start, env.action_repeat, int(env.ids[0]))
        self.ids = self.env.ids

    def _screen(self, f):
        return R.screen(render(int(f), self.ENV.RULES[0]))


def with_rules(visible, frozen):
    """(Env, EngineRef) classes under other rules, e.g. (10, 0): Catch."""
    env = type('CatchEnv_%d_%d' % (visible, frozen), (CatchMemoryEnv,), dict(RULES=(int(visible), int(frozen))))
    return env, type('CatchEngineRef_%d_%d' % (visible, frozen), (CatchMemoryEngineRef,), dict(ENV=env))
