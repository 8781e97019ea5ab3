"""Catch (Catch-v0) without a GPU: the rules as tests/_catch_ref.py restates them
(exhaustively: 640 states), the numbers the GPU tests measure against (the optimal and the random
policy's return), the command line, the header and the ctypes mirror."""
import os
import re

import numpy as np
import pytest

import _catch_ref as C

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'a3c_hip.h')


def env_at(frames, action_repeat=1):
    env = C.CatchEnv(7, len(frames), action_repeat=action_repeat)
    env.new_game()
    env.frame[:] = np.asarray(frames, np.uint32)
    env.ep_step[:] = C.decode(env.frame)[1]
    return env


# ------------------------------------------------------------------ the rules, exhaustively
@pytest.mark.parametrize('repeat', [1, 3])
def test_every_state_and_action_stays_in_bounds(repeat):
    """All 640 states x actions 0..5 (3, 4, 5 mean stay): the next frame index is in [0, 640) -- the
    property that keeps the pool read in bounds --, the terminal is r' == 9, the ball's column never
    changes, the reward is non-zero only at a landing, and a landed state is a fixed point with
    reward 0, terminal 1."""
    states = np.arange(C.FRAMES)
    c0, r0, p0 = C.decode(states)
    for a in range(6):
        env = env_at(states, repeat)
        f, rew, term = env.act(np.full(C.FRAMES, a))
        assert f.dtype == np.uint32 and (f < C.FRAMES).all()
        c1, r1, p1 = C.decode(f)
        assert np.array_equal(c1, c0)
        assert np.array_equal(r1, np.minimum(r0 + repeat, C.ROWS - 1))
        assert np.array_equal(term, r1 == C.ROWS - 1)
        assert np.array_equal(env.ep_step, r1) and (env.ep_len == C.ROWS - 1).all() and (env.lives == 0).all()
        moves = r1 - r0                                   # raw steps actually taken
        d = {1: -1, 2: 1}.get(a, 0)
        assert np.array_equal(p1, np.clip(p0 + d * moves, 0, C.COLS - 1))
        landed = r0 == C.ROWS - 1
        assert np.array_equal(f[landed], states[landed]) and (rew[landed] == 0).all() and term[landed].all()
        landing = ~landed & term
        assert np.array_equal(rew[landing], np.where(p1 == c1, 1.0, -1.0)[landing])
        assert (rew[~landing] == 0).all()
        if a >= 3:                                        # any other value means stay
            stay = env_at(states, repeat)
            f0, rew0, term0 = stay.act(np.zeros(C.FRAMES, np.int64))
            assert np.array_equal(f, f0) and np.array_equal(rew, rew0) and np.array_equal(term, term0)


def test_simple_act_is_one_raw_step():
    states = np.arange(C.FRAMES)
    for a in range(3):
        env = env_at(states, action_repeat=3)
        f, rew, term = env.simple_act(np.full(C.FRAMES, a))
        want = [C.step_state(s, a) for s in states]
        assert np.array_equal(f, [w[0] for w in want])
        assert np.array_equal(rew, np.array([w[1] for w in want], np.float32))
        assert np.array_equal(term, [w[2] for w in want])


def test_reset_is_the_new_game_and_draws_ball_and_paddle():
    from oracle import philox as px
    env = C.CatchEnv(123, 300, env_id_base=17)
    env.new_random_game()
    assert (env.episode == 1).all() and (env.ep_step == 0).all() and (env.ep_len == 9).all()
    assert (env.reward == 0).all() and not env.terminal.any() and (env.lives == 0).all()
    k0, k1 = px.seed_key(123)
    x0, x1, _, _ = px.philox4x32(np.uint32(1), env.ids, px.P_RESET, 0, k0, k1)
    c, r, p = C.decode(env.frame)
    assert np.array_equal(c, x0 % 8) and np.array_equal(p, x1 % 8) and (r == 0).all()
    assert len(set(env.frame.tolist())) > 40          # 300 draws over 64 reset states
    # a masked new game touches the masked envs only, and resets them mid-episode too
    env.act(np.zeros(300, np.int64))
    before = env.frame.copy()
    m = np.arange(300) % 3 == 0
    env.new_game(m)
    assert np.array_equal(env.frame[~m], before[~m]) and (env.episode[m] == 2).all() and (env.episode[~m] == 1).all()
    assert (C.decode(env.frame[m])[1] == 0).all()


def test_greedy_policy_returns_plus_one_in_nine_steps():
    """From every one of the 64 reset states the paddle reaches the ball: 9 moves cover a distance of
    at most 7.  Every episode lasts exactly 9 steps."""
    starts = C.encode(np.repeat(np.arange(8), 8), 0, np.tile(np.arange(8), 8))
    assert len(starts) == 64
    env = env_at(starts)
    ret = np.zeros(64)
    for t in range(C.ROWS - 1):
        c, _, p = C.decode(env.frame)
        a = np.where(p > c, 1, np.where(p < c, 2, 0))
        _, rew, term = env.act(a)
        ret += rew
        assert term.all() == (t == C.ROWS - 2) and term.any() == (t == C.ROWS - 2)
    assert (ret == 1).all()
    # and running to the far wall loses from every reset state
    env = env_at(starts)
    ret = np.zeros(64)
    for t in range(C.ROWS - 1):
        c, _, p = C.decode(env.frame)
        ret += env.act(np.where(c >= 4, 1, 2))[1]
    assert (ret == -1).all()


def test_random_policy_return_is_exact_and_below_the_bar():
    R = C.random_policy_return()
    assert (3 ** 9 * 64) % R.denominator == 0          # 3^9 action sequences x 64 reset states
    assert -1 < R < 0                                  # the random paddle misses more often than not
    assert C.R_RAND == float(R)
    assert C.LEARNING_BAR == C.R_RAND + 0.5 * (1 - C.R_RAND) and C.R_RAND < C.LEARNING_BAR < 1
    # Monte Carlo on the restatement, uniformly random actions over resets: within 5 standard
    # errors of a +-1 variable (sd <= 1) at 20000 episodes
    rng = np.random.default_rng(5)
    n = 20000
    c = rng.integers(0, 8, n)
    p = rng.integers(0, 8, n)
    for _ in range(9):
        p = np.clip(p + rng.integers(-1, 2, n), 0, 7)
    mc = float(np.where(p == c, 1.0, -1.0).mean())
    assert abs(mc - C.R_RAND) < 5 / np.sqrt(n), (mc, C.R_RAND)
    print('R_rand =', R, '=', C.R_RAND, 'bar =', C.LEARNING_BAR, 'monte carlo', mc)


def test_render():
    for f in (0, 79, 80 * 3 + 8 * 4 + 5, 639):
        c, r, p = (int(v) for v in C.decode(f))
        img = C.render(f)
        assert img.shape == (210, 160, 3) and img.dtype == np.uint8
        ball = np.zeros((210, 160), bool)
        ball[21 * r:21 * r + 21, 20 * c:20 * c + 20] = True
        pad = np.zeros((210, 160), bool)
        pad[200:210, 20 * p:20 * p + 20] = True
        assert (img[pad] == (92, 186, 92)).all()
        assert (img[ball & ~pad] == 236).all()
        assert (img[~ball & ~pad] == 0).all()
    assert len({C.render(f).tobytes() for f in range(C.FRAMES)}) == C.FRAMES    # the frame shows the whole state


def test_engine_ref_plays_catch():
    from oracle import ref_cpu as R
    ref = C.CatchEngineRef({}, 5, 3, 3, 'a3c', 0, 640, 11, action_repeat=2)
    assert isinstance(ref.env, C.CatchEnv) and ref.env.action_repeat == 2 and ref.env.P == 640
    assert np.array_equal(ref.screen_of(333), R.screen(C.render(333)))
    ref.reset()
    assert (ref.env.episode == 1).all()
    assert np.array_equal(ref.ring[2, 3], ref.screen_of(ref.env.frame[2]))


# ------------------------------------------------------------------ names and the command line
def test_game_spec_and_kind():
    from src.environment import GAMES, game_kind, game_spec
    assert game_spec('Catch-v0') == (3, 0)
    assert game_kind('Catch-v0') == 'catch'
    for name in ('Pong-v0', 'Breakout-v0', 'SpaceInvaders-v0'):
        assert game_kind(name) == 'synth' and len(game_spec(name)) == 2
    assert all(len(v) == 2 for v in GAMES.values())
    with pytest.raises(ValueError):
        game_kind('Tennis-v0')


def test_flags_accept_catch_like_pong():
    import main
    for extra in ([], ['--lstm', 'true'], ['--gae_lambda', '0.9'], ['--algo', 'q', '--double_q', 'true'],
                  ['--dqn_type', 'nature']):
        catch = main.parse_flags(['--env_name', 'Catch-v0'] + extra)
        pong = main.parse_flags(['--env_name', 'Pong-v0'] + extra)
        assert catch.env_name == 'Catch-v0'
        assert main.engine_options(catch) == main.engine_options(pong)
        d1, d2 = dict(vars(catch)), dict(vars(pong))
        d1.pop('env_name'), d2.pop('env_name')
        assert d1 == d2
    play = main.parse_flags(['--env_name', 'Catch-v0', '--is_train', 'false', '--play_refill', 'true'])
    assert main.play_options(play, world=1) == main.play_options(
        main.parse_flags(['--env_name', 'Pong-v0', '--is_train', 'false', '--play_refill', 'true']), world=1)


@pytest.mark.parametrize('envs_on', ['host', 'gym'])
def test_catch_is_a_device_game(envs_on):
    import main
    with pytest.raises(ValueError, match='Catch-v0'):
        main.engine_options(main.parse_flags(['--env_name', 'Catch-v0', '--envs_on', envs_on]))
    with pytest.raises(ValueError, match='Catch-v0'):      # before any config or device work
        main.main(['--mode', 'engine', '--env_name', 'Catch-v0', '--envs_on', envs_on])
    main.engine_options(main.parse_flags(['--env_name', 'Pong-v0', '--envs_on', envs_on]))     # as before


def test_existing_rejections_stay_for_catch():
    import main
    for argv in (['--dueling', 'true'], ['--dqn_type', 'nature', '--algo', 'q'], ['--gae_lambda', '0.9', '--algo', 'q']):
        with pytest.raises(ValueError):
            main.engine_options(main.parse_flags(['--env_name', 'Catch-v0'] + argv))


# ------------------------------------------------------------------ header and bindings
def test_header_declares_catch():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'#define\s+A3C_GAME_SYNTH\s+0\b', src)
    assert re.search(r'#define\s+A3C_GAME_CATCH\s+1\b', src)
    m = re.search(r'\bint\s+a3c_env_create_ex\s*\((.*?)\)\s*;', src, re.S)
    old = re.search(r'\bint\s+a3c_env_create\s*\((.*?)\)\s*;', src, re.S)
    assert m and old
    args, old_args = [a.strip() for a in m.group(1).split(',')], [a.strip() for a in old.group(1).split(',')]
    assert args == old_args[:-1] + ['int game', old_args[-1]]          # the old entry's signature stays pinned
    m = re.search(r'\bint\s+a3c_engine_create_ex\s*\((.*?)\)\s*;', src, re.S)
    assert m and [a.strip() for a in m.group(1).split(',')] == ['const a3c_engine_config* cfg', 'int game',
                                                               'a3c_engine** out']


def test_ctypes_mirror_binds_catch():
    from src import _lib
    assert (_lib.A3C_GAME_SYNTH, _lib.A3C_GAME_CATCH) == (0, 1)
    res, args = _lib.SIGNATURES['a3c_env_create_ex']
    old = _lib.SIGNATURES['a3c_env_create'][1]
    assert res is _lib.c_int and args == old[:-1] + [_lib.c_int] + old[-1:]
    res, args = _lib.SIGNATURES['a3c_engine_create_ex']
    assert res is _lib.c_int and len(args) == 3 and args[1] is _lib.c_int
    from src.engine import GAME_IDS
    assert GAME_IDS == {'synth': 0, 'catch': 1}
