"""Batched evaluation (a3c_engine_play, Agent.play agent.py:351-391): the parts that need no GPU --
the CPU restatement's own batching rule, main.py's play_options, and the a3c_play_config layout."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from _play_ref import make_ref, play_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')


# ------------------------------------------------------------------ 1. the restatement's batching
def test_play_ref_batched_equals_single_envs():
    """Episode w*E + e of the batched restatement is episode w of env e played alone (env ids are
    global, frozen envs do not advance): E = 4, 8 episodes against four E = 1 runs of 2."""
    n_step, lives, seed = 400, 1, 11
    zeros = np.zeros((2, n_step, 4), np.int32)
    ref = make_ref({}, 4, 6, 'a3c', lives, frames=16, seed=seed)
    got = play_ref(ref, 8, n_step, forced_actions=zeros, forward=False)
    assert got['terminated'].any() and not got['terminated'].all()     # both ends of an episode occur
    for e in range(4):
        one = make_ref({}, 1, 6, 'a3c', lives, frames=16, seed=seed, env_id_base=e)
        alone = play_ref(one, 2, n_step, forced_actions=zeros[:, :, :1], forward=False)
        for w in range(2):
            for k in ('returns', 'lengths', 'terminated'):
                assert got[k][w * 4 + e] == alone[k][w], (k, e, w)
    # a second call goes on with the emulators where the first left them, the taus start again
    again = play_ref(ref, 8, n_step, forced_actions=zeros, forward=False)
    assert not np.array_equal(again['lengths'], got['lengths'])


def test_play_ref_partial_last_wave_and_best():
    ref = make_ref({}, 4, 6, 'a3c', 0, frames=16, seed=5)
    out = play_ref(ref, 6, 32, forced_actions=np.zeros((2, 32, 4), np.int32), forward=False)
    assert out['waves'] == 2 and out['returns'].shape == (6,)
    assert not out['live'][1, :, 2:].any() and out['live'][1, :, :2].all()
    assert (out['lengths'] == 32).all() and not out['terminated'].any()      # Pong: ep_len >= 200
    best = (0.0, 0)
    for i, r in enumerate(out['returns']):
        if r > best[0]:
            best = (float(r), i)
    assert (out['best_reward'], out['best_idx']) == best


# ------------------------------------------------------------------ 2. main.py play_options
def _flags(*argv):
    import main
    return main, main.parse_flags(list(argv))


def test_play_options_accepts():
    main, f = _flags('--mode', 'engine', '--is_train', 'false')
    assert main.play_options(f, world=1) == dict(n_episode=100, n_step=10000, test_ep=None, greedy=False)
    main, f = _flags('--mode', 'engine', '--is_train', 'false', '--n_episode', '7', '--play_steps', '50',
                     '--test_ep', '0.05', '--algo', 'q', '--update', 'sync')
    assert main.play_options(f, world=1) == dict(n_episode=7, n_step=50, test_ep=0.05, greedy=False)
    main, f = _flags('--mode', 'engine', '--is_train', 'false', '--greedy', '--test_ep', '0')
    assert main.play_options(f, world=1) == dict(n_episode=100, n_step=10000, test_ep=0.0, greedy=True)
    main, f = _flags('--mode', 'engine', '--is_train', 'false', '--lstm', 'true')
    assert main.play_options(f, world=1)['n_episode'] == 100 and main.engine_options(f) == dict(lstm=True)


@pytest.mark.parametrize('argv', [('--envs_on', 'host'), ('--envs_on', 'gym'), ('--update', 'hogwild'),
                                  ('--n_episode', '0'), ('--play_steps', '0'), ('--test_ep', '-0.5'),
                                  ('--greedy', '--algo', 'q')])
def test_play_options_rejects(argv):
    main, f = _flags('--mode', 'engine', '--is_train', 'false', *argv)
    with pytest.raises(ValueError):
        main.play_options(f, world=1)


def test_play_options_rejects_several_ranks(monkeypatch):
    main, f = _flags('--mode', 'engine', '--is_train', 'false')
    with pytest.raises(ValueError):
        main.play_options(f, world=2)
    monkeypatch.setenv('WORLD_SIZE', '4')
    with pytest.raises(ValueError):
        main.play_options(f)
    monkeypatch.setenv('WORLD_SIZE', '1')
    assert main.play_options(f) is not None


@pytest.mark.parametrize('argv', [(), ('--lstm', 'true'), ('--algo', 'q', '--double_q', 'true'),
                                  ('--dqn_type', 'nature'), ('--envs_on', 'host'), ('--update', 'hogwild')])
def test_training_flags_are_unchanged(argv):
    """--is_train true: play_options stays out of the way and engine_options gives what it gave."""
    main, f = _flags('--mode', 'engine', *argv)
    assert main.play_options(f, world=8) is None
    want = dict(lstm='--lstm' in argv)
    if '--double_q' in argv:
        want['double_q'] = True
    if '--dqn_type' in argv:
        want['dqn_type'] = 'nature'
    assert main.engine_options(f) == want


@pytest.mark.parametrize('argv', [('--dueling', 'true'), ('--dqn_type', 'nature', '--algo', 'q'),
                                  ('--double_q', 'true'), ('--lstm', 'true', '--algo', 'q')])
def test_engine_options_rejections_stay(argv):
    for train in ('true', 'false'):
        main, f = _flags('--mode', 'engine', '--is_train', train, *argv)
        with pytest.raises(ValueError):
            main.engine_options(f)


# ------------------------------------------------------------------ 3. a3c_play_config layout
C_PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "a3c_hip.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
int main(void) {
  printf("a3c_play_config %zu\n", sizeof(a3c_play_config));
  printf("a3c_play_buffers %zu\n", sizeof(a3c_play_buffers));
  F(a3c_play_config, n_episode) F(a3c_play_config, n_step) F(a3c_play_config, greedy)
  F(a3c_play_config, test_ep) F(a3c_play_config, poll_every)
  F(a3c_play_buffers, frame_ring) F(a3c_play_buffers, ring_slots) F(a3c_play_buffers, tau)
  F(a3c_play_buffers, env_frame) F(a3c_play_buffers, env_len) F(a3c_play_buffers, returns)
  F(a3c_play_buffers, frozen) F(a3c_play_buffers, lstm_h) F(a3c_play_buffers, lstm_c)
  return 0;
}
'''


def test_play_struct_layout_matches_gcc(tmp_path):
    src = tmp_path / 'probe.c'
    src.write_text(C_PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    got = dict(line.rsplit(' ', 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))
    from src import _lib
    cls = {'a3c_play_config': _lib.PlayConfig, 'a3c_play_buffers': _lib.PlayBuffers}
    for name, c in cls.items():
        assert int(got[name]) == ctypes.sizeof(c), name
    seen = 0
    for key, val in got.items():
        if '.' in key:
            st, field = key.split('.')
            assert getattr(cls[st], field).offset == int(val), key
            seen += 1
    assert seen == 14
    assert [f for f, _ in _lib.PlayConfig._fields_] == ['n_episode', 'n_step', 'greedy', 'test_ep', 'poll_every']
