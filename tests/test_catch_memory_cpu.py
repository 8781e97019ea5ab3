"""CatchMemory-v0 without a GPU: the rules as tests/_catch_memory_ref.py restates them
(exhaustively: 640 states), the theorem the GPU tests measure against -- no policy of the 4-frame
stack does better than R_ML, one with memory reaches +1 -- by brute force over every reset state
with its exact probability, the command line, the header and the two setters' argument checks."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _catch_memory_ref as M
import _catch_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')
V, F = M.RULES


def env_at(cls, frames, action_repeat=1):
    env = cls(7, len(frames), action_repeat=action_repeat)
    env.new_game()
    env.frame[:] = np.asarray(frames, np.uint32)
    env.ep_step[:] = C.decode(env.frame)[1]
    return env


# ------------------------------------------------------------------ the rules, exhaustively
def test_rules_are_catch_memory():
    assert (V, F) == (1, 4) and F >= V + 3


@pytest.mark.parametrize('repeat', [1, 3])
def test_every_state_and_action(repeat):
    """All 640 states x actions 0..5: the result stays in [0, 640); an elementary step from a frozen
    row (< 4) is no paddle move, every other one is Catch's step; row, terminal and reward as Catch
    states them."""
    states = np.arange(M.FRAMES)
    c0, r0, p0 = C.decode(states)
    for a in range(6):
        env = env_at(M.CatchMemoryEnv, states, repeat)
        f, rew, term = env.act(np.full(M.FRAMES, a))
        assert f.dtype == np.uint32 and (f < M.FRAMES).all()
        c1, r1, p1 = C.decode(f)
        assert np.array_equal(c1, c0) and np.array_equal(r1, np.minimum(r0 + repeat, 9))
        assert np.array_equal(term, r1 == 9)
        assert np.array_equal(env.ep_step, r1) and (env.ep_len == 9).all() and (env.lives == 0).all()
        free = np.maximum(r1, F) - np.maximum(r0, F)          # the elementary steps taken from rows >= F
        d = {1: -1, 2: 1}.get(a, 0)
        assert np.array_equal(p1, np.clip(p0 + d * free, 0, 7))
        landing = (r0 < 9) & term
        assert np.array_equal(rew[landing], np.where(p1 == c1, 1.0, -1.0)[landing]) and (rew[~landing] == 0).all()
        # one elementary step against Catch's own
        for s in states:
            got, want = M.step_state(s, a), C.step_state(s, a)
            if r0[s] >= F or r0[s] == 9:
                assert got == want, (s, a)
            else:
                assert C.decode(got[0])[2] == p0[s] and C.decode(got[0])[1] == r0[s] + 1 and got[1:] == want[1:], (s, a)


@pytest.mark.parametrize('repeat', [1, 3])
def test_rules_10_0_are_catch(repeat):
    env_cls, ref_cls = M.with_rules(10, 0)
    states = np.arange(M.FRAMES)
    for a in range(6):
        got = env_at(env_cls, states, repeat).act(np.full(M.FRAMES, a))
        want = env_at(C.CatchEnv, states, repeat).act(np.full(M.FRAMES, a))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), a
    a, b = env_cls(123, 300, env_id_base=17), C.CatchEnv(123, 300, env_id_base=17)
    for _ in range(3):
        a.new_random_game()
        b.new_random_game()
        assert np.array_equal(a.frame, b.frame) and np.array_equal(a.episode, b.episode)
    for f in (0, 79, 277, 639):
        assert np.array_equal(M.render(f, 10), C.render(f))
    assert issubclass(ref_cls, C.CatchEngineRef) and ref_cls.ENV is env_cls


# ------------------------------------------------------------------ reset
def test_reset_draws_a_reachable_ball():
    from oracle import philox as px
    env = M.CatchMemoryEnv(123, 300, env_id_base=17)
    k0, k1 = px.seed_key(123)
    seen = set()
    for ep in (1, 2, 3):
        env.new_random_game()
        assert (env.episode == ep).all() and (env.ep_step == 0).all() and (env.ep_len == 9).all()
        assert (env.reward == 0).all() and not env.terminal.any() and (env.lives == 0).all()
        x0, x1, _, _ = px.philox4x32(np.uint32(ep), env.ids, px.P_RESET, 0, k0, k1)
        c, r, p = (np.asarray(v, np.int64) for v in C.decode(env.frame))
        assert (r == 0).all() and np.array_equal(p, x1 % 8)
        assert (np.abs(c - p) <= 9 - F).all()
        for e in range(300):
            lo, hi = max(0, int(p[e]) - (9 - F)), min(7, int(p[e]) + (9 - F))
            assert c[e] == lo + int(x0[e]) % (hi - lo + 1)
        seen |= set(zip(c.tolist(), p.tolist()))
    assert seen <= set(M.reset_distribution()) and len(seen) > 40
    # every other frozen_rows: the same property; F <= 2 is Catch's draw
    for f in range(9):
        cls, _ = M.with_rules(1, f)
        e2 = cls(5, 200)
        e2.new_game()
        c, _, p = (np.asarray(v, np.int64) for v in C.decode(e2.frame))
        assert (np.abs(c - p) <= 9 - f).all(), f
        if f <= 2:
            cat = C.CatchEnv(5, 200)
            cat.new_game()
            assert np.array_equal(e2.frame, cat.frame)


def test_remembering_the_ball_returns_plus_one():
    """From every reachable reset state: remember c from the first frame, move towards it from row 4."""
    starts = sorted(M.reset_distribution())
    assert len(starts) == 58 and all(abs(c - p) <= 5 for c, p in starts)
    env = env_at(M.CatchMemoryEnv, [C.encode(c, 0, p) for c, p in starts])
    c0 = np.array([c for c, _ in starts])                 # the memory: read off the row-0 frame
    for e, f in enumerate(env.frame):
        ball = M.render(f)[10, 10::20, 0] == 236
        assert ball.sum() == 1 and int(np.argmax(ball)) == c0[e]
    ret = np.zeros(len(starts))
    for t in range(9):
        p = C.decode(env.frame)[2]
        _, rew, term = env.act(np.where(p > c0, 1, np.where(p < c0, 2, 0)))
        ret += rew
        assert term.all() == (t == 8)
    assert (ret == 1).all()


# ------------------------------------------------------------------ the theorem, by brute force
def paddle_of(img):
    pad = img[205, 10::20, 1] == 186
    assert pad.sum() == 1
    return int(np.argmax(pad))


def motion_policy(stack):
    d = paddle_of(stack[3]) - paddle_of(stack[2])
    return 2 if d > 0 else (1 if d < 0 else 2)            # repeat the last motion; at rest: right


def table_policy(seed):
    table = np.random.default_rng(seed).integers(0, 3, (8, 8, 8, 8))
    return lambda stack: int(table[tuple(paddle_of(s) for s in stack)])


def exact_return(policy, rules=M.RULES):
    """The exact return of a deterministic policy of the 4-frame stack (a function of the four
    rendered frames, newest last): every reset state, weighted by its exact probability."""
    frames = {}

    def img(f):
        if f not in frames:
            frames[f] = M.render(f, rules[0])
        return frames[f]

    total = Fraction(0)
    for (c, p), w in M.reset_distribution(rules[1]).items():
        f = int(C.encode(c, 0, p))
        hist = [f] * 4                                   # agent.py:37-38: four copies of the first screen
        ret = 0.0
        for _ in range(9):
            a = policy([img(g) for g in hist])
            f, rew, term = M.step_state(f, a, rules[1])
            hist = hist[1:] + [f]
            ret += rew
        assert term and ret in (-1.0, 1.0)
        total += w * int(ret)
    return total


def test_numbers():
    assert M.R_ML == Fraction(-121, 168) and abs(float(M.R_ML) - -0.7202380951) < 1e-9
    assert M.LEARNING_BAR == M.R_ML + (1 - M.R_ML) / 2 == Fraction(47, 336)
    assert abs(float(M.LEARNING_BAR) - 0.1398809524) < 1e-9
    assert sum(M.reset_distribution().values()) == 1
    lo, hi = M.ml_return_bounds()
    assert lo <= M.R_ML <= hi and hi - lo < Fraction(1, 10 ** 9)
    print('R_ML', M.R_ML, float(M.R_ML), 'with the modulo bias in', float(lo), float(hi), 'bar', float(M.LEARNING_BAR))


@pytest.mark.parametrize('name,policy', [('left', lambda s: 1), ('right', lambda s: 2), ('stay', lambda s: 0),
                                         ('motion', motion_policy), ('table1', table_policy(1)),
                                         ('table2', table_policy(2))])
def test_no_stack_policy_beats_chance(name, policy):
    got = exact_return(policy)
    lo, hi = M.ml_return_bounds()
    assert lo <= got <= hi, (name, got)
    assert abs(float(got - M.R_ML)) < 1e-9, (name, float(got))


@pytest.mark.parametrize('name,policy', [('left', lambda s: 1), ('motion', motion_policy), ('table3', table_policy(3))])
def test_no_stack_policy_beats_chance_under_rules_2_5(name, policy):
    """The rules the GPU learning test trains under: F = 5 >= V + 3 = 5."""
    got = exact_return(policy, (2, 5))
    lo, hi = M.ml_return_bounds(5)
    assert lo <= got <= hi and abs(float(got - M.memoryless_return(5))) < 1e-9, (name, float(got))
    assert M.memoryless_return(5) == Fraction(-1147, 1680)


def test_the_theorem_needs_its_premise():
    """F < V + 3 -- rules (2, 4): the stack at row 4 holds row 1, which shows the ball -- and a policy of
    the stack does better than chance."""
    def chase(stack):
        for img in stack:
            ball = img[:200, 10::20, 0].max(axis=0) == 236
            if ball.any():
                c, p = int(np.argmax(ball)), paddle_of(stack[3])
                return 1 if p > c else (2 if p < c else 0)
        return 0
    assert exact_return(chase, (2, 4)) > M.memoryless_return(4) + Fraction(1, 10)
    assert abs(float(exact_return(chase, (2, 5)) - M.memoryless_return(5))) < 1e-9


def test_a_policy_that_sees_the_ball_does_better():
    """The brute force is no tautology: under rules (10, 0) rendering, the ball is in the stack and the
    greedy policy of the newest frame returns +1 from every reset state of the same law."""
    def greedy(stack):
        ball = stack[3][:200, 10::20, 0].max(axis=0) == 236
        c, p = int(np.argmax(ball)), paddle_of(stack[3])
        return 1 if p > c else (2 if p < c else 0)
    total = Fraction(0)
    for (c, p), w in M.reset_distribution().items():
        f = int(C.encode(c, 0, p))
        ret = 0.0
        for _ in range(9):
            f, rew, _ = M.step_state(f, greedy([None, None, None, M.render(f, 10)]))
            ret += rew
        total += w * int(ret)
    assert total == 1


# ------------------------------------------------------------------ render
def test_render_hides_the_ball_below_the_first_row():
    for f in range(M.FRAMES):
        c, r, p = (int(v) for v in C.decode(f))
        img = M.render(f)
        assert img.shape == (210, 160, 3) and img.dtype == np.uint8
        pad = np.zeros((210, 160), bool)
        pad[200:210, 20 * p:20 * p + 20] = True
        assert (img[pad] == (92, 186, 92)).all()
        if r == 0:
            assert np.array_equal(img, C.render(f)) and (img[:21, 20 * c:20 * c + 20] == 236).all()
        else:
            assert (img[~pad] == 0).all()
    # the frames of a stack at rows 1..4 do not depend on c
    for p in range(8):
        for r in range(1, 5):
            assert len({M.render(C.encode(c, r, p)).tobytes() for c in range(8)}) == 1


def test_engine_ref_plays_catch_memory():
    from oracle import ref_cpu as R
    ref = M.CatchMemoryEngineRef({}, 5, 3, 3, 'a3c', 0, 640, 11, action_repeat=2)
    assert isinstance(ref.env, M.CatchMemoryEnv) and ref.env.action_repeat == 2 and ref.env.P == 640
    assert np.array_equal(ref.screen_of(333), R.screen(M.render(333)))
    assert not np.array_equal(ref.screen_of(333), R.screen(C.render(333)))
    ref.reset()
    c, r, p = (np.asarray(v, np.int64) for v in C.decode(ref.env.frame))
    assert (ref.env.episode == 1).all() and (np.abs(c - p) <= 5).all()


# ------------------------------------------------------------------ names and the command line
def test_names():
    from src import engine
    from src.environment import CATCH_RULES, GAMES, catch_rules_of, game_kind, game_spec
    assert game_spec('CatchMemory-v0') == (3, 0) and game_kind('CatchMemory-v0') == 'catch'
    assert CATCH_RULES == {'CatchMemory-v0': (1, 4)} and catch_rules_of('CatchMemory-v0') == M.RULES
    for name in ('Catch-v0', 'Pong-v0', 'Breakout-v0', 'SpaceInvaders-v0', 'Tennis-v0'):
        assert catch_rules_of(name) is None
    assert engine.GAMES == GAMES and engine.GAMES['CatchMemory-v0'] == (3, 0)


def test_flags_accept_catch_memory_like_pong():
    import main
    for extra in ([], ['--lstm', 'true'], ['--gae_lambda', '0.9'], ['--algo', 'q', '--double_q', 'true']):
        mem = main.parse_flags(['--env_name', 'CatchMemory-v0'] + extra)
        pong = main.parse_flags(['--env_name', 'Pong-v0'] + extra)
        assert main.engine_options(mem) == main.engine_options(pong)
        assert 'catch_rules' not in main.engine_options(mem)
    assert 'CatchMemory-v0' in main.__doc__


@pytest.mark.parametrize('envs_on', ['host', 'gym'])
def test_catch_memory_is_a_device_game(envs_on):
    import main
    with pytest.raises(ValueError, match='CatchMemory-v0'):
        main.engine_options(main.parse_flags(['--env_name', 'CatchMemory-v0', '--envs_on', envs_on]))
    with pytest.raises(ValueError, match='CatchMemory-v0'):      # before any config or device work
        main.main(['--mode', 'engine', '--env_name', 'CatchMemory-v0', '--envs_on', envs_on])


def test_engine_rejects_before_device_work(monkeypatch):
    from src import _lib, engine
    monkeypatch.setattr(_lib, 'require_device', lambda: (_ for _ in ()).throw(AssertionError('device asked for')))
    with pytest.raises(ValueError, match='catch_rules'):
        engine.Engine(action_size=3, catch_rules=(1, 4))                       # game synth
    for bad in ((0, 4), (11, 0), (1, -1), (1, 9)):
        with pytest.raises(ValueError, match='catch_rules'):
            engine.Engine(action_size=3, game='catch', catch_rules=bad)


# ------------------------------------------------------------------ header and the setters' checks
def test_header_declares_the_setters():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+a3c_engine_set_catch_rules\s*\((.*?)\)\s*;', src, re.S)
    assert m and [a.strip() for a in m.group(1).split(',')] == ['a3c_engine* eng', 'int visible_rows', 'int frozen_rows']
    m = re.search(r'\bint\s+a3c_env_set_catch_rules\s*\((.*?)\)\s*;', src, re.S)
    assert m and [a.strip() for a in m.group(1).split(',')] == ['a3c_env* env', 'int visible_rows', 'int frozen_rows',
                                                               'void* stream']
    from src import _lib
    i, p = _lib.c_int, _lib.c_void_p
    assert _lib.SIGNATURES['a3c_engine_set_catch_rules'] == (i, [p, i, i])
    assert _lib.SIGNATURES['a3c_env_set_catch_rules'] == (i, [p, i, i, p])
    assert ctypes.sizeof(_lib.EngineOpts) == 12 and ctypes.sizeof(_lib.EngineConfig) == 184       # neither grew


def test_setters_reject_before_they_touch_the_device():
    """The values are checked before the handle is looked at: with a NULL handle the message names the
    argument, and only valid values reach the NULL check.  No device is needed."""
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    from src import _lib
    lib = ctypes.CDLL(SO)
    lib.a3c_last_error.restype = ctypes.c_char_p
    eng, env = lib.a3c_engine_set_catch_rules, lib.a3c_env_set_catch_rules
    eng.restype = env.restype = ctypes.c_int
    eng.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    env.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for (v, f), word in (((0, 4), b'visible'), ((11, 4), b'visible'), ((-1, 99), b'visible'), ((0, 9), b'visible'),
                         ((1, -1), b'frozen'), ((1, 9), b'frozen'), ((10, 100), b'frozen'),
                         ((1, 4), b'null'), ((10, 0), b'null'), ((1, 8), b'null'), ((10, 8), b'null')):
        assert eng(None, v, f) == _lib.ERR_INVALID and word in lib.a3c_last_error(), (v, f, lib.a3c_last_error())
        assert b'a3c_engine_set_catch_rules' in lib.a3c_last_error()
        assert env(None, v, f, None) == _lib.ERR_INVALID and word in lib.a3c_last_error(), (v, f, lib.a3c_last_error())
        assert b'a3c_env_set_catch_rules' in lib.a3c_last_error()
