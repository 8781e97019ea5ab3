"""Play with refill (a3c_engine_play_ex refill = 1): the parts that need no GPU.  In the synthetic
env the terminals depend only on (ep_step, env id, episode) Philox words, not on actions, so the
schedule of any configuration is computed here with forward=False: the conditions the GPU tests'
shapes were chosen for, the step bound, main.py's play_options and the header."""
import os
import re

import numpy as np
import pytest

from _play_ref import make_ref, play_ref
from _play_refill_ref import play_refill_ref, schedule_facts, step_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')


def schedule(E, n_episode, n_step, seed, lives=1, action_repeat=4, algo='a3c', **kw):
    ref = make_ref({}, E, 6, algo, lives, frames=48, seed=seed, action_repeat=action_repeat, **kw)
    ref.screen_of = lambda f: 0                 # only the schedule is wanted: no screens
    zeros = np.zeros((step_bound(n_episode, n_step, E), E), np.int32)
    return play_refill_ref(ref, n_episode, n_step, forced_actions=zeros, forward=False)


# ------------------------------------------------------------------ 1. the GPU tests' schedules
def test_schedule_of_the_a3c_and_q_cases():
    """tests 1 and 2 of test_gpu_play_refill.py: E = 6, lives = 1, action_repeat = 4, 20 episodes of
    at most 40 steps, seed 1 (the schedule does not depend on the algorithm or the actions)."""
    r = schedule(6, 20, 40, seed=1)
    f = schedule_facts(r)
    assert f['refill_terminal'] >= 5 and f['refill_cap'] >= 1, f
    assert f['max_together'] >= 2 and f['idle_early'] >= 1, f
    # the first-generation envs that reach the cap do so in the same step
    first_caps = [t for t, e, kind, _ in r['events'] if kind == 'cap' and t == 39]
    assert len(first_caps) >= 2
    assert r['terminated'].sum() == f['refill_terminal'] + sum(1 for *_, k, n in r['events'] if k == 'terminal' and n < 0)
    f7 = schedule_facts(schedule(7, 16, 40, seed=1, algo='q'))
    assert f7['refill_terminal'] >= 1 and f7['refill_cap'] >= 1, f7


@pytest.mark.parametrize('E,n_episode,n_step,seed,kw', [(1, 3, 12, 1, {}), (37, 60, 10, 1, {}),
                                                        (6, 11, 12, 2, dict(frame84=True)), (6, 11, 12, 2, {}),
                                                        (8, 14, 12, 1, dict(dqn_type='nature')),
                                                        (8, 14, 12, 1, dict(lstm=True))])
def test_schedule_of_the_small_nature_and_lstm_cases(E, n_episode, n_step, seed, kw):
    r = schedule(E, n_episode, n_step, seed, **kw)
    f = schedule_facts(r)
    assert f['refill_terminal'] + f['refill_cap'] >= 1, f
    if E == 8:
        assert f['refill_terminal'] >= 1 and f['refill_cap'] >= 1, f
        assert sum(1 for i in range(E, n_episode) if r['lengths'][i] >= 3) >= 3      # (the LSTM state matters)
    if E == 37:
        assert f['max_together'] > n_episode - E, f            # more ends in one step than episodes left


# ------------------------------------------------------------------ 2. the rules themselves
def test_schedule_is_in_order_and_gapless():
    r = schedule(6, 20, 40, seed=1)
    E = 6
    assert r['episode_env'][:E].tolist() == list(range(E)) and (r['episode_tau0'][:E] == 3).all()
    assert np.all(np.diff(r['episode_tau0']) >= 0)             # indices are handed out in time order ...
    for t in set(r['episode_tau0'][E:].tolist()):              # ... and within a step in env-id order
        envs = r['episode_env'][r['episode_tau0'] == t]
        assert np.all(np.diff(envs) > 0)
    for e in range(E):                                         # an env's episodes are back to back
        mine = np.flatnonzero(r['episode_env'] == e)
        for a, b in zip(mine[:-1], mine[1:]):
            assert r['episode_tau0'][b] == r['episode_tau0'][a] + r['lengths'][a]
    live = r['live']
    assert live.sum() == r['lengths'].sum()                    # every live slot belongs to an episode
    assert (r['lengths'] <= 40).all() and (r['lengths'][~r['terminated']] == 40).all()
    assert not live[r['steps']:].any() and live[r['steps'] - 1].any()


def test_refill_equals_waves_when_no_env_is_refilled():
    """n_episode <= E: one wave."""
    a = make_ref({}, 6, 6, 'a3c', 1, frames=48, seed=1, action_repeat=4)
    b = make_ref({}, 6, 6, 'a3c', 1, frames=48, seed=1, action_repeat=4)
    zeros = np.zeros((40, 6), np.int32)
    w = play_ref(a, 5, 40, forced_actions=zeros[None], forward=False)
    r = play_refill_ref(b, 5, 40, forced_actions=zeros, forward=False)
    for k in ('returns', 'lengths', 'terminated'):
        assert np.array_equal(w[k], r[k]), k
    assert np.array_equal(w['live'][0], r['live'])
    for f in ('episode', 'ep_step', 'ep_len', 'lives', 'frame'):
        assert np.array_equal(getattr(a.env, f), getattr(b.env, f)), f


def test_step_bound_over_seeds_and_shapes():
    """ceil(n_episode / E) * n_step run steps always suffice (play_refill_ref asserts that every
    episode has finished within the bound); it is reached when every episode hits the cap."""
    for seed in range(1, 9):
        for E, n_episode, n_step, lives, rep in ((1, 4, 9, 1, 4), (3, 10, 17, 1, 4), (6, 20, 40, 1, 4), (5, 5, 30, 1, 8),
                                                 (4, 13, 25, 3, 8), (7, 50, 12, 1, 16), (37, 90, 6, 0, 1)):
            r = schedule(E, n_episode, n_step, seed, lives=lives, action_repeat=rep)
            assert r['steps'] <= step_bound(n_episode, n_step, E), (seed, E, n_episode, n_step)
            assert r['lengths'].min() >= 1
    r = schedule(4, 10, 8, seed=3, lives=0, action_repeat=1)      # Pong: ep_len >= 200, every episode capped
    assert not r['terminated'].any() and r['steps'] == step_bound(10, 8, 4) == 24


def test_utilisation_exceeds_waves():
    """Live slots / run slots of both modes on one configuration: refill never runs more steps."""
    a = make_ref({}, 6, 6, 'a3c', 1, frames=48, seed=1, action_repeat=4)
    zeros = np.zeros((4, 40, 6), np.int32)
    w = play_ref(a, 20, 40, forced_actions=zeros, forward=False)
    wave_steps = sum(int(w['lengths'][i * 6:(i + 1) * 6].max()) for i in range(4))
    r = schedule(6, 20, 40, seed=1)
    assert r['steps'] < wave_steps
    assert r['lengths'].sum() / (r['steps'] * 6) > w['lengths'].sum() / (wave_steps * 6)


# ------------------------------------------------------------------ 3. main.py play_options
def _flags(*argv):
    import main
    return main, main.parse_flags(list(argv))


def test_play_options_with_and_without_the_flag():
    main, f = _flags('--mode', 'engine', '--is_train', 'false')
    assert main.play_options(f, world=1) == dict(n_episode=100, n_step=10000, test_ep=None, greedy=False)
    main, f = _flags('--mode', 'engine', '--is_train', 'false', '--play_refill', 'false')
    assert 'refill' not in main.play_options(f, world=1)
    main, f = _flags('--mode', 'engine', '--is_train', 'false', '--play_refill', 'true', '--n_episode', '7')
    assert main.play_options(f, world=1) == dict(n_episode=7, n_step=10000, test_ep=None, greedy=False, refill=True)
    main, f = _flags('--mode', 'engine', '--play_refill', 'true')
    assert main.play_options(f, world=1) is None               # training: the flag has no effect


# ------------------------------------------------------------------ 4. the header and the binding
def test_header_declares_refill_and_the_schedule():
    sys_path = os.path.join(ROOT, 'async-rl-tensorflow_amd')
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    from src import _lib
    text = open(HEADER).read()
    m = re.search(r'int a3c_engine_play_ex\(([^;]*)\);', text)
    assert m and re.search(r'const a3c_play_config\* cfg, int refill,', m.group(1))
    m = re.search(r'int a3c_engine_play_schedule\(([^;]*)\);', text)
    assert m and 'int32_t* episode_env' in m.group(1) and 'int64_t* episode_tau0' in m.group(1)
    assert re.search(r'int32_t\* episode_idx;[^}]*int32_t\* sched;[^}]*\} a3c_play_buffers;', text)
    for name in ('a3c_engine_play_ex', 'a3c_engine_play_schedule'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['a3c_engine_play_ex'][1]) == len(_lib.SIGNATURES['a3c_engine_play'][1]) + 1
    assert [f for f, _ in _lib.PlayBuffers._fields_][-2:] == ['episode_idx', 'sched']
    import inspect
    from src.engine import Engine
    assert inspect.signature(Engine.play).parameters['refill'].default is False
