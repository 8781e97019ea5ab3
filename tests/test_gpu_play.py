"""Batched evaluation on the engine: a3c_engine_play / Engine.play / main.py --is_train false, the
batched form of Agent.play (agent.py:351-391), against the CPU restatement tests/_play_ref.py.

The engine's traced actions are replayed on the restatement (as _engine_parity does), then:
returns, lengths, terminated and the best episode are exactly equal; the traced head rows of every
live (step, env) match the restatement's independent forward on its own ring states at the
project's rtol 1e-4; every draw is explained (assert_draws_explained); trace entries of frozen envs
are untouched; the env state and, for capped episodes of the last wave, the newest ring planes are
bit-identical."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from _engine_parity import assert_draws_explained, assert_z, build  # noqa: E402
from _play_ref import make_ref, play_ref, ref_like  # noqa: E402


def check_play(eng, pref, n_episode, n_step, test_ep=None, greedy=False, tag='', **play_kw):
    """One Engine.play call against the restatement pref (both keep their play state)."""
    A, algo, E = eng.A, eng.algo, eng.E
    out = eng.play(n_episode=n_episode, n_step=n_step, test_ep=test_ep, greedy=greedy, trace=True, **play_kw)
    acts = out['actions'].cpu().numpy()
    z = out['z'].cpu().numpy()
    r = play_ref(pref, n_episode, n_step, forced_actions=acts, test_ep=test_ep, greedy=greedy)
    print(tag, 'returns', out['returns'].tolist(), 'lengths', out['lengths'].tolist(),
          'terminated', int(out['terminated'].sum()), 'life losses', int(r['life_lost'].sum()))
    assert np.array_equal(out['returns'], r['returns']), (tag, out['returns'], r['returns'])
    assert np.array_equal(out['lengths'], r['lengths']), (tag, out['lengths'], r['lengths'])
    assert np.array_equal(out['terminated'], r['terminated']), tag
    assert (out['best_reward'], out['best_idx']) == (r['best_reward'], r['best_idx']), tag
    live = r['live']
    assert live.any()
    # frozen envs and steps that were not run: the trace keeps its fill
    assert (acts[~live] == -1).all(), tag
    assert np.isnan(z[~live]).all(), tag
    assert ((acts[live] >= 0) & (acts[live] < A)).all(), tag
    zw = A + 1 if algo == 'a3c' else A
    assert_z(z[live], r['z'][live], zw, tag)
    mode1 = algo == 'q' or greedy
    sub = dict(sampled=r['sampled'][live][None], z=[r['z'][live]], u=r['u'][live][None], eps=r['eps'][live][None])
    assert_draws_explained(acts[live][None], sub, 'q' if mode1 else 'a3c', A, tag,
                           z_eng=None if mode1 else z[live][None])
    # the play context's env state: nothing of a frozen env advanced, both parity copies equal
    pb = eng.play_buffers()
    for f in ('frame', 'lives', 'episode', 'ep_step', 'ep_len'):
        got = pb[f].cpu().numpy()
        want = getattr(pref.env, f).astype(np.int32)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (tag, f)
    # capped episodes of the last wave: the HIST newest ring planes
    w = r['waves'] - 1
    n_act = n_episode - w * E
    capped = [e for e in range(n_act) if not r['terminated'][w * E + e]]
    if capped:
        tau = 3 + w * (n_step + 4) + n_step
        assert int(pb['tau'].item()) == tau == int(r['last_tau'][w]), tag
        ring, R = pb['ring'].cpu().numpy(), pb['ring_slots']
        for e in capped:
            for c in range(4):
                assert np.array_equal(ring[e, (tau - 3 + c) % R], pref.ring[e, (tau - 3 + c) % pref.R]), (tag, e, c)
    return out, r


# ------------------------------------------------------------------ 4. NIPS Q: terminals and caps
def test_play_q_terminals_and_caps():
    eng, ref, _ = build('q', 6, 16, 5, lives=1, seed=3)
    pref = ref_like(ref)
    out, r = check_play(eng, pref, 24, 48, test_ep=0.25, tag='q')
    assert r['waves'] == 2 and r['live'][1, 0].sum() == 8
    term = r['terminated']
    for w, sl in enumerate((slice(0, 16), slice(16, 24))):
        assert term[sl].any() and not term[sl].all(), w          # an early end and a cap in each wave
    assert (r['returns'] > 0).any() and (r['returns'] < 0).any()
    assert int(term.sum()) == 7
    assert np.all(r['eps'] == np.float32(0.25))


# ------------------------------------------------------------------ 5. is_training=False is honoured
def test_play_life_loss_is_no_terminal():
    eng, ref, _ = build('a3c', 6, 16, 5, lives=3, seed=3, action_repeat=2)
    pref = make_ref(ref.params, 16, 6, 'a3c', 3, 48, 3, action_repeat=2)
    out, r = check_play(eng, pref, 24, 48, tag='lives')
    assert int(r['life_lost'].sum()) >= 2       # lost lives that ended no episode and cost no -1


# ------------------------------------------------------------------ 6. small and odd shapes
@pytest.mark.parametrize('E,n_episode,n_step,kw', [(6, 9, 16, {}), (6, 9, 16, dict(frame84=1)), (1, 3, 16, {}),
                                                   (37, 37, 6, {}), (6, 9, 16, dict(A=18))])
def test_play_small_shapes(E, n_episode, n_step, kw):
    """(A = 18: the play tail's head with the wide head_row and the wide select_with, traced rows of
    stride zs = 20.)"""
    kw = dict(kw)
    eng, ref, _ = build('a3c', kw.pop('A', 4), E, 5, lives=0, seed=40 + E, **kw)
    check_play(eng, ref_like(ref), n_episode, n_step, tag=(E, n_episode, kw))


def test_play_a3c_greedy_and_epsilon():
    eng, ref, _ = build('a3c', 6, 5, 5, lives=0, seed=9)
    pref = ref_like(ref)
    out, r = check_play(eng, pref, 5, 12, test_ep=0.0, greedy=True, tag='greedy')
    assert np.array_equal(out['actions'].cpu().numpy()[r['live']], r['sampled'][r['live']])
    check_play(eng, pref, 7, 12, test_ep=0.5, greedy=True, tag='eps-greedy')    # (the context persists)


def test_play_q_default_epsilon_is_the_envs_own():
    eng, ref, _ = build('q', 6, 7, 5, lives=0, seed=21)
    out, r = check_play(eng, ref_like(ref), 7, 24, tag='q ep_end')
    assert np.array_equal(r['eps'][0, 0], ref.ep_end)


# ------------------------------------------------------------------ 7. nature trunk, LSTM head
def test_play_nature_trunk():
    eng, ref, _ = build('a3c', 6, 8, 5, lives=1, seed=61, scale=2.0, dqn_type='nature')
    check_play(eng, ref_like(ref), 12, 12, tag='nature')


def test_play_lstm_head():
    from src.engine import Engine
    from src.initializers import flatten_host, init_params
    from src.kernels import param_names_shapes
    E, A, seed = 8, 6, 71
    eng = Engine(num_envs=E, n_step=5, action_size=A, algo='a3c', start_lives=1, num_frames=48, seed=seed, lstm=True)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    p = init_params(ns, seed=seed, stddev=0.08)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), p))
    pref = make_ref(p, E, A, 'a3c', 1, 48, seed, lstm=True)
    check_play(eng, pref, 12, 12, tag='lstm')


# ------------------------------------------------------------------ 8. frozen envs are isolated
def test_play_batched_equals_single_env_engines():
    n_step, lives, seed = 96, 1, 4
    eng, ref, _ = build('a3c', 6, 4, 5, lives=lives, seed=seed)
    params = eng.params.cpu().numpy()
    got = eng.play(n_episode=8, n_step=n_step, trace=True)
    acts = got['actions'].cpu().numpy()
    assert got['terminated'].any() and not got['terminated'].all()
    from src.engine import Engine
    for e in range(4):
        one = Engine(num_envs=1, n_step=5, action_size=6, algo='a3c', start_lives=lives, num_frames=48, seed=seed,
                     env_id_base=e)
        one.reset(params)
        alone = one.play(n_episode=2, n_step=n_step, trace=True)
        for w in range(2):
            for k in ('returns', 'lengths', 'terminated'):
                assert got[k][w * 4 + e] == alone[k][w], (k, e, w)
        assert np.array_equal(acts[:, :, e], alone['actions'].cpu().numpy()[:, :, 0]), e
        one.close()


# ------------------------------------------------------------------ 9. independent of polling
def _same(a, b):
    for k in ('returns', 'lengths', 'terminated'):
        assert np.array_equal(a[k], b[k]), k
    assert (a['best_reward'], a['best_idx']) == (b['best_reward'], b['best_idx'])
    assert torch.equal(a['actions'], b['actions'])
    assert torch.equal(torch.nan_to_num(a['z'], nan=-7.0), torch.nan_to_num(b['z'], nan=-7.0))


def test_play_does_not_depend_on_polling():
    engs = [build('a3c', 6, 4, 5, lives=1, seed=17)[0] for _ in range(2)]
    outs = []
    for eng, poll in zip(engs, (1, 1000)):
        outs.append([eng.play(n_episode=6, n_step=1500, poll_every=poll, trace=True) for _ in range(2)])
    assert outs[0][0]['terminated'].all()                 # every wave ends early: the stop matters
    for call in range(2):
        _same(outs[0][call], outs[1][call])
    assert not np.array_equal(outs[0][0]['lengths'], outs[0][1]['lengths'])   # the emulators went on
    pa, pb = engs[0].play_buffers(), engs[1].play_buffers()
    for k in ('frame', 'lives', 'episode', 'ep_step', 'ep_len', 'ring', 'returns', 'lengths', 'terminated'):
        assert torch.equal(pa[k], pb[k]), k


def test_play_reset_clears_the_context():
    eng, _, _ = build('q', 6, 3, 5, lives=1, seed=23)
    first = eng.play(n_episode=5, n_step=20, test_ep=0.1, trace=True)
    second = eng.play(n_episode=5, n_step=20, test_ep=0.1, trace=True)
    assert not torch.equal(first['actions'], second['actions'])
    eng.reset()
    _same(eng.play(n_episode=5, n_step=20, test_ep=0.1, trace=True), first)


# ------------------------------------------------------------------ 10. training state untouched
@pytest.mark.parametrize('overlap', [False, True])
def test_play_leaves_training_untouched(overlap):
    E = 8
    a, b = [build('a3c', 6, E, 5, lives=3, seed=31, overlap=overlap)[0] for _ in range(2)]
    for eng in (a, b):
        for _ in range(3):
            eng.iterate()
    out = a.play(n_episode=E, n_step=24)
    assert out['lengths'].min() > 0
    for eng in (a, b):
        for _ in range(3):
            eng.iterate()
    torch.cuda.synchronize()
    for k in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------ rejected cases
def test_play_rejections():
    from src import _lib
    from src.engine import Engine
    eng = Engine(num_envs=2, n_step=5, action_size=6, num_frames=16, seed=1)
    with pytest.raises(_lib.A3CError) as ei:
        eng.play(n_episode=2, n_step=4)
    assert ei.value.rc == _lib.ERR_STATE                  # before a3c_engine_reset
    eng.reset()
    for kw in (dict(n_episode=0), dict(n_step=0), dict(poll_every=0)):
        with pytest.raises(_lib.A3CError) as ei:
            eng.play(**{**dict(n_episode=2, n_step=4), **kw})
        assert ei.value.rc == _lib.ERR_INVALID, kw
    assert eng.play(n_episode=2, n_step=4)['lengths'].tolist() == [4, 4]
    ext = Engine(num_envs=2, n_step=5, action_size=6, seed=1, external_env=True)
    ext.reset()
    with pytest.raises(_lib.A3CError) as ei:
        ext.play(n_episode=2, n_step=4)
    assert ei.value.rc == _lib.ERR_INVALID


# ------------------------------------------------------------------ 11. main.py --is_train false
def test_main_engine_is_train_false(tmp_path, capsys):
    import main
    logdir = str(tmp_path / 'logs')
    common = ['--mode', 'engine', '--env_name', 'Pong-v0', '--num_envs', '4', '--num_frames', '32', '--logdir', logdir,
              '--update', 'sync']
    # without a checkpoint: a warning, the initial parameters
    main.main(common + ['--is_train', 'false', '--n_episode', '6', '--play_steps', '8'])
    cap = capsys.readouterr()
    assert 'no checkpoint' in cap.err
    recs = [json.loads(x) for x in open(os.path.join(logdir, 'play.jsonl'))]
    assert len(recs) == 1 and recs[0]['mode'] == 'play' and recs[0]['checkpoint'] is None
    assert recs[0]['n_episode'] == 6 and recs[0]['env_steps'] == 48 and recs[0]['global_step'] == 0
    assert json.loads(cap.out.strip().splitlines()[-1]) == recs[0]
    files = sorted(os.listdir(logdir))
    assert not [f for r, _, fs in os.walk(logdir) for f in fs if f != 'play.jsonl'], files   # nothing saved
    # after two training iterations: plays that checkpoint, writes none, the step stays
    main.main(common + ['--iterations', '2'])
    tree = sorted((r, f, os.path.getsize(os.path.join(r, f))) for r, _, fs in os.walk(logdir) for f in fs
                  if f not in ('play.jsonl', 'engine.jsonl'))
    assert tree
    capsys.readouterr()
    main.main(common + ['--is_train', 'false', '--n_episode', '3', '--play_steps', '8', '--greedy'])
    recs = [json.loads(x) for x in open(os.path.join(logdir, 'play.jsonl'))]
    assert len(recs) == 2 and recs[1]['checkpoint'] and recs[1]['global_step'] == 2 * 4 * 5
    assert recs[1]['n_episode'] == 3 and recs[1]['greedy'] is True
    assert tree == sorted((r, f, os.path.getsize(os.path.join(r, f))) for r, _, fs in os.walk(logdir) for f in fs
                          if f not in ('play.jsonl', 'engine.jsonl'))
