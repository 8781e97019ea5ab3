"""Play with refill on the engine (a3c_engine_play_ex refill = 1, Engine.play(refill=True), main.py
--play_refill) against the CPU restatement tests/_play_refill_ref.py.

The engine's traced actions are replayed on the restatement, then: returns, lengths, terminated,
the best episode, the schedule (episode_env, episode_tau0) and the live step count are exactly
equal; the traced head rows of every live (run step, env) match the restatement's independent
forward at the project's rtol 1e-4; every draw is explained; trace entries of idle envs and of steps
not run keep their fill; the env state is bit-identical in both parity copies; for envs whose last
episode was capped the HIST newest ring planes are bit-identical.  The shapes' schedules are chosen
on the CPU (tests/test_play_refill_cpu.py asserts the same conditions without a GPU)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from _engine_parity import assert_draws_explained, assert_z, build  # noqa: E402
from _play_ref import make_ref  # noqa: E402
from _play_refill_ref import play_refill_ref, schedule_facts, step_bound  # noqa: E402

ENV_KEYS = ('frame', 'lives', 'episode', 'ep_step', 'ep_len')


def check_refill(eng, pref, n_episode, n_step, test_ep=None, greedy=False, tag='', **play_kw):
    """One Engine.play(refill=True) call against the restatement pref (both keep their play state)."""
    A, algo, E = eng.A, eng.algo, eng.E
    bound = step_bound(n_episode, n_step, E)
    out = eng.play(n_episode=n_episode, n_step=n_step, test_ep=test_ep, greedy=greedy, trace=True, refill=True,
                   **play_kw)
    acts = out['actions'].cpu().numpy()
    z = out['z'].cpu().numpy()
    assert acts.shape == (bound, E) and z.shape == (bound, E, eng.zs), tag
    r = play_refill_ref(pref, n_episode, n_step, forced_actions=acts, test_ep=test_ep, greedy=greedy)
    print(tag, 'returns', out['returns'].tolist(), 'lengths', out['lengths'].tolist(), 'steps', out['steps'],
          'of', bound, schedule_facts(r))
    for k in ('returns', 'lengths', 'terminated', 'episode_env', 'episode_tau0'):
        assert np.array_equal(out[k], r[k]), (tag, k, out[k], r[k])
    assert (out['best_reward'], out['best_idx']) == (r['best_reward'], r['best_idx']), tag
    assert out['steps'] == r['steps'] <= bound, tag
    live = r['live']
    assert live.any()
    # idle envs and steps that were not run: the trace keeps its fill
    assert (acts[~live] == -1).all(), tag
    assert np.isnan(z[~live]).all(), tag
    assert ((acts[live] >= 0) & (acts[live] < A)).all(), tag
    zw = A + 1 if algo == 'a3c' else A
    assert_z(z[live], r['z'][live], zw, tag)
    mode1 = algo == 'q' or greedy
    sub = dict(sampled=r['sampled'][live][None], z=[r['z'][live]], u=r['u'][live][None], eps=r['eps'][live][None])
    assert_draws_explained(acts[live][None], sub, 'q' if mode1 else 'a3c', A, tag,
                           z_eng=None if mode1 else z[live][None])
    # the play context's env state: both parity copies equal the restatement's
    pb = eng.play_buffers()
    for f in ENV_KEYS:
        got = pb[f].cpu().numpy()
        want = getattr(pref.env, f).astype(np.int32)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (tag, f)
    assert pb['sched'].tolist() == [n_episode, n_episode, 0, r['steps']], tag
    # envs whose last episode was capped: the HIST newest ring planes of its last step
    ring, R = pb['ring'].cpu().numpy(), pb['ring_slots']
    capped = 0
    for e in range(E):
        mine = np.flatnonzero(r['episode_env'] == e)
        if mine.size == 0 or r['terminated'][mine[-1]]:
            continue
        tau = int(r['episode_tau0'][mine[-1]]) + int(r['lengths'][mine[-1]])
        for c in range(4):
            assert np.array_equal(ring[e, (tau - 3 + c) % R], pref.ring[e, (tau - 3 + c) % pref.R]), (tag, e, c)
        capped += 1
    return out, r, capped


def play_pair(algo, A, E, lives, seed, action_repeat=4, **kw):
    """An engine and a fresh play restatement with its configuration and parameters."""
    eng, ref, _ = build(algo, A, E, 5, lives=lives, seed=seed, action_repeat=action_repeat, **kw)
    pref = make_ref(ref.params, E, A, algo, lives, 48, seed, action_repeat=action_repeat,
                    frame84=bool(kw.get('frame84')), dqn_type=kw.get('dqn_type', 'nips'))
    return eng, pref


# ------------------------------------------------------------------ 1. A3C NIPS: every kind of event
def test_refill_a3c_terminals_caps_and_idle():
    eng, pref = play_pair('a3c', 6, 6, 1, seed=1)
    out, r, capped = check_refill(eng, pref, 20, 40, tag='a3c')
    f = schedule_facts(r)
    assert f['refill_terminal'] >= 5 and f['refill_cap'] >= 1, f
    assert f['max_together'] >= 2, f           # two or more envs ended in one step: the scan order
    assert f['idle_early'] >= 1, f             # an env left idle before the run ends
    assert capped >= 1
    # a second call goes on with the emulators where the first left them; tau starts again
    out2, _, _ = check_refill(eng, pref, 9, 24, tag='a3c again')
    assert out2['episode_tau0'][0] == 3


# ------------------------------------------------------------------ 2. Q: fixed and per-env epsilon
def test_refill_q_test_ep():
    eng, pref = play_pair('q', 6, 6, 1, seed=1)
    out, r, _ = check_refill(eng, pref, 20, 40, test_ep=0.25, tag='q 0.25')
    f = schedule_facts(r)
    assert f['refill_terminal'] >= 5 and f['refill_cap'] >= 1 and f['max_together'] >= 2, f
    assert np.all(r['eps'] == np.float32(0.25))


def test_refill_q_default_epsilon_is_the_envs_own():
    eng, pref = play_pair('q', 6, 7, 1, seed=1)
    out, r, _ = check_refill(eng, pref, 16, 40, tag='q ep_end')
    f = schedule_facts(r)
    assert f['refill_terminal'] >= 1 and f['refill_cap'] >= 1, f
    assert np.array_equal(r['eps'][0], pref.ep_end) and len(set(pref.ep_end.tolist())) > 1


# ------------------------------------------------------------------ 3. small and odd shapes
@pytest.mark.parametrize('E,n_episode,n_step,seed,kw', [(1, 3, 12, 1, {}), (37, 60, 10, 1, {}),
                                                        (6, 11, 12, 2, dict(frame84=1)), (6, 11, 12, 2, dict(A=18))])
def test_refill_small_shapes(E, n_episode, n_step, seed, kw):
    """(E = 37: 33 envs reach the cap in one step -- the scan hands out 23 indices and idles the
    rest; A = 18: the wide head_row / select_with, traced rows of stride zs = 20.)"""
    kw = dict(kw)
    eng, pref = play_pair('a3c', kw.pop('A', 4), E, 1, seed=seed, **kw)
    out, r, _ = check_refill(eng, pref, n_episode, n_step, tag=(E, n_episode, kw))
    f = schedule_facts(r)
    assert f['refill_terminal'] + f['refill_cap'] >= 1, f


# ------------------------------------------------------------------ 4. nature trunk, LSTM head
def test_refill_nature_trunk():
    eng, pref = play_pair('a3c', 6, 8, 1, seed=1, scale=2.0, dqn_type='nature')
    out, r, _ = check_refill(eng, pref, 14, 12, tag='nature')
    f = schedule_facts(r)
    assert f['refill_terminal'] >= 1 and f['refill_cap'] >= 1, f


def test_refill_lstm_head_state_is_zeroed():
    """A refilled env's h / c are zero at its new episode's first step: the restatement zeroes
    them, so an engine that carried the last episode's state fails the z comparison on every step of
    the refilled episodes (5 of them last >= 3 steps)."""
    from src.engine import Engine
    from src.initializers import flatten_host, init_params
    from src.kernels import param_names_shapes
    E, A, seed = 8, 6, 1
    eng = Engine(num_envs=E, n_step=5, action_size=A, algo='a3c', start_lives=1, num_frames=48, seed=seed, lstm=True,
                 action_repeat=4)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    p = init_params(ns, seed=seed, stddev=0.08)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), p))
    pref = make_ref(p, E, A, 'a3c', 1, 48, seed, action_repeat=4, lstm=True)
    out, r, _ = check_refill(eng, pref, 14, 12, tag='lstm')
    assert sum(1 for i in range(E, 14) if r['lengths'][i] >= 3) >= 3
    # the state the zeroing replaced was not zero already: the carried h of a live env is not
    hsum = float(eng.play_buffers()['lstm_h'].abs().sum())
    assert hsum > 0


# ------------------------------------------------------------------ 5. n_episode <= E: waves mode
def _same_outputs(a, b, keys=('returns', 'lengths', 'terminated', 'episode_env', 'episode_tau0')):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    assert (a['best_reward'], a['best_idx'], a['steps']) == (b['best_reward'], b['best_idx'], b['steps'])


def _same_traces(a, b):
    ta, tb = a['actions'].reshape(-1), b['actions'].reshape(-1)
    assert torch.equal(ta, tb)
    assert torch.equal(torch.nan_to_num(a['z'], nan=-7.0).reshape(-1), torch.nan_to_num(b['z'], nan=-7.0).reshape(-1))


def test_refill_equals_waves_when_no_env_is_refilled():
    engs = [build('a3c', 6, 6, 5, lives=1, seed=1, action_repeat=4)[0] for _ in range(2)]
    outs = [eng.play(n_episode=5, n_step=40, trace=True, refill=rf) for eng, rf in zip(engs, (False, True))]
    assert outs[0]['terminated'].any() and not outs[0]['terminated'].all()
    _same_outputs(*outs)
    _same_traces(*outs)
    pa, pb = engs[0].play_buffers(), engs[1].play_buffers()
    for k in ENV_KEYS + ('ring', 'tau', 'returns', 'lengths', 'terminated'):
        assert torch.equal(pa[k], pb[k]), k
    # the frozen flags: equal for the envs that terminated or had no episode.  A capped env is the one
    # word that differs by rule: a wave never freezes it (the wave is over), a refill run does (it got
    # no new episode and other envs may go on) -- in the copy the run's last step wrote.
    capped = torch.as_tensor(np.concatenate([~outs[0]['terminated'], [False]]), device='cuda')
    assert torch.equal(pa['frozen'][:, ~capped], pb['frozen'][:, ~capped])
    assert not pa['frozen'][:, capped].any() and pb['frozen'][0, capped].all() and not pb['frozen'][1, capped].any()


# ------------------------------------------------------------------ 6. independent of polling
def test_refill_does_not_depend_on_polling():
    engs = [build('a3c', 6, 6, 5, lives=1, seed=1, action_repeat=4)[0] for _ in range(2)]
    outs = [eng.play(n_episode=20, n_step=40, poll_every=poll, trace=True, refill=True)
            for eng, poll in zip(engs, (1, 1000))]
    assert outs[0]['steps'] < step_bound(20, 40, 6)          # the run ends early: the stop matters
    _same_outputs(*outs)
    _same_traces(*outs)
    pa, pb = engs[0].play_buffers(), engs[1].play_buffers()
    assert int(pa['tau'].item()) == 3 + outs[0]['steps']     # poll_every = 1 stops at the last live step
    for k in ENV_KEYS + ('ring', 'returns', 'lengths', 'terminated', 'episode_idx', 'sched'):
        assert torch.equal(pa[k], pb[k]), k


# ------------------------------------------------------------------ 7. training state untouched
@pytest.mark.parametrize('overlap', [False, True])
def test_refill_leaves_training_untouched(overlap):
    E = 8
    a, b = [build('a3c', 6, E, 5, lives=3, seed=31, overlap=overlap)[0] for _ in range(2)]
    for eng in (a, b):
        for _ in range(3):
            eng.iterate()
    out = a.play(n_episode=2 * E + 3, n_step=24, refill=True)
    assert out['lengths'].min() > 0 and (out['episode_tau0'] > 3).sum() == E + 3      # refills happened
    for eng in (a, b):
        for _ in range(3):
            eng.iterate()
    torch.cuda.synchronize()
    for k in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------ 8. rejections, main.py
def test_refill_rejections():
    from src import _lib
    from src.engine import Engine
    eng = Engine(num_envs=2, n_step=5, action_size=6, num_frames=16, seed=1)
    with pytest.raises(_lib.A3CError) as ei:
        eng.play(n_episode=2, n_step=4, refill=True)
    assert ei.value.rc == _lib.ERR_STATE                  # before a3c_engine_reset
    eng.reset()
    for kw in (dict(refill=2), dict(refill=-1), dict(n_episode=0), dict(n_step=0), dict(poll_every=0)):
        with pytest.raises(_lib.A3CError) as ei:
            eng.play(**{**dict(n_episode=5, n_step=4, refill=True), **kw})
        assert ei.value.rc == _lib.ERR_INVALID, kw
    out = eng.play(n_episode=5, n_step=4, refill=True)
    assert out['lengths'].tolist() == [4] * 5 and out['steps'] == 12
    assert out['episode_env'].tolist() == [0, 1, 0, 1, 0] and out['episode_tau0'].tolist() == [3, 3, 7, 7, 11]
    waves = eng.play(n_episode=5, n_step=4)               # waves mode reports idx % E and the wave's tau
    assert waves['episode_env'].tolist() == [0, 1, 0, 1, 0] and waves['episode_tau0'].tolist() == [3, 3, 11, 11, 19]
    assert waves['steps'] == 12
    ext = Engine(num_envs=2, n_step=5, action_size=6, seed=1, external_env=True)
    ext.reset()
    with pytest.raises(_lib.A3CError) as ei:
        ext.play(n_episode=2, n_step=4, refill=True)
    assert ei.value.rc == _lib.ERR_INVALID


def test_main_engine_play_refill(tmp_path, capsys):
    import main
    logdir = str(tmp_path / 'logs')
    main.main(['--mode', 'engine', '--env_name', 'Pong-v0', '--num_envs', '4', '--num_frames', '32', '--logdir', logdir,
               '--update', 'sync', '--is_train', 'false', '--n_episode', '6', '--play_steps', '8', '--play_refill',
               'true'])
    cap = capsys.readouterr()
    recs = [json.loads(x) for x in open(os.path.join(logdir, 'play.jsonl'))]
    assert len(recs) == 1 and recs[0]['mode'] == 'play' and recs[0]['refill'] is True
    assert recs[0]['n_episode'] == 6 and recs[0]['env_steps'] == 48 and recs[0]['steps'] == 16
    assert json.loads(cap.out.strip().splitlines()[-1]) == recs[0]
