"""Catch (Catch-v0) on the GPU, against tests/_catch_ref.py: the rendered pool, the
stand-alone batched env (a3c_env_create_ex), the engine in every mode (the Catch instantiations of
the fused head kernels), play in waves and with refill, the rejections -- and that the engine
learns the game.

Bars: the project's existing ones, through the existing helpers (_engine_parity's check_* with the
oracle swapped for CatchEngineRef, test_gpu_lstm's LSTM check, test_gpu_gae's lambda-return check,
test_gpu_play's / test_gpu_play_refill's replays): env quantities and the ring exact; z, losses,
gradients and parameters at the bars those helpers assert."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

CATCH = dict(game='catch')
A, FRAMES = 3, C.FRAMES


@pytest.fixture
def catch_oracle(monkeypatch):
    """The existing parity helpers build their oracle as EngineRef(...): make that the Catch one."""
    import test_gpu_lstm
    monkeypatch.setattr(EP, 'EngineRef', C.CatchEngineRef)
    monkeypatch.setattr(test_gpu_lstm, 'EngineRef', C.CatchEngineRef)


def screens_of(frames, cache={}):
    for f in set(int(f) for f in frames):
        if f not in cache:
            cache[f] = R.screen(C.render(f))
    return np.stack([cache[int(f)] for f in frames])


def make_config(**kw):
    from test_gpu_dropin import make_config as mk
    return mk('Catch-v0', **kw)


# ------------------------------------------------------------------ the pool
def test_pool_is_rendered_byte_for_byte():
    """All 640 frames of k_pool_render_catch, read through the engine's pool buffer."""
    from src.engine import Engine
    eng = Engine(num_envs=2, n_step=2, action_size=A, num_frames=FRAMES, seed=3, **CATCH)
    eng.reset()
    torch.cuda.synchronize()
    pool = eng.frame_pool.cpu().numpy()
    assert pool.shape == (FRAMES, 210, 160, 3)
    bad = [f for f in range(FRAMES) if not np.array_equal(pool[f], C.render(f))]
    assert not bad, bad[:8]
    # a larger pool (the engine's own default): the same 640 frames in front
    big = Engine(num_envs=2, n_step=2, action_size=A, seed=3, **CATCH)
    assert big.cfg.num_frames >= FRAMES
    big.reset()
    torch.cuda.synchronize()
    assert torch.equal(big.frame_pool[:FRAMES].cpu(), torch.as_tensor(pool))


# ------------------------------------------------------------------ the stand-alone env
@pytest.mark.parametrize('repeat', [1, 2])
def test_batched_env_matches_reference(repeat):
    """E = 5, 40 acts with uniformly random actions, terminals restarted through
    new_random_game(mask): frames, rewards, terminals and the 84x84 screens bit-equal."""
    from src.environment import BatchedEnvironment
    E, seed = 5, 77
    env = BatchedEnvironment(make_config(action_repeat=repeat, random_start=30), num_envs=E, env_id_base=5, seed=seed)
    assert env.game == 'catch' and env.action_size == A and env.frame_pool.shape[0] >= FRAMES
    ref = C.CatchEnv(seed, E, action_repeat=repeat, env_id_base=5)
    scr = env.new_random_game()[0]
    ref.new_random_game()
    torch.cuda.synchronize()
    assert np.array_equal(env._frame.cpu().numpy(), ref.frame.astype(np.int32))
    assert np.array_equal(scr.cpu().numpy(), screens_of(ref.frame))
    rng = np.random.default_rng(3)
    landings = 0
    for t in range(40):
        a = rng.integers(0, A, E).astype(np.int32)
        scr, rew, term = env.act(torch.as_tensor(a), is_training=bool(t & 1))
        fr, rr, tt = ref.act(a)
        torch.cuda.synchronize()
        assert np.array_equal(env._frame.cpu().numpy(), fr.astype(np.int32)), t
        assert np.array_equal(rew.cpu().numpy(), rr), t
        assert np.array_equal(term.cpu().numpy().astype(bool), tt), t
        assert (env.lives_all.cpu().numpy() == 0).all(), t
        assert np.array_equal(scr.cpu().numpy(), screens_of(fr)), t
        landings += int(tt.sum())
        if tt.any():
            assert set(rr[tt].tolist()) <= {-1.0, 1.0}
            env.new_random_game(torch.as_tensor(tt.astype(np.uint8)).cuda())
            ref.new_random_game(tt.copy())
            torch.cuda.synchronize()
            assert np.array_equal(env._frame.cpu().numpy(), ref.frame.astype(np.int32)), t
    assert landings >= 15


@pytest.mark.parametrize('repeat', [1, 3])
def test_every_state_and_action_on_the_device(repeat):
    """The exhaustive CPU check on the kernel's own rules: env e is put in state e (all 640), every
    action 0..5 -- the next frame index stays in [0, 640), frame, reward and terminal equal the
    reference's, for act and for the raw step."""
    from src.environment import BatchedEnvironment
    env = BatchedEnvironment(make_config(action_repeat=repeat), num_envs=FRAMES, seed=1, num_frames=FRAMES)
    env.new_game()
    states = torch.arange(FRAMES, dtype=torch.int32, device='cuda')
    for simple in (False, True):
        for a in range(6):
            env._frame.copy_(states)
            ref = C.CatchEnv(1, FRAMES, action_repeat=repeat)
            ref.new_game()
            ref.frame[:] = np.arange(FRAMES, dtype=np.uint32)
            _, rew, term = env.act(torch.full((FRAMES,), a, dtype=torch.int32), simple=simple)
            fr, rr, tt = ref.simple_act(np.full(FRAMES, a)) if simple else ref.act(np.full(FRAMES, a))
            torch.cuda.synchronize()
            got = env._frame.cpu().numpy()
            assert ((got >= 0) & (got < FRAMES)).all(), (a, simple)
            assert np.array_equal(got, fr.astype(np.int32)), (a, simple)
            assert np.array_equal(rew.cpu().numpy(), rr), (a, simple)
            assert np.array_equal(term.cpu().numpy().astype(bool), tt), (a, simple)


def test_single_env_wrappers_play_catch():
    """--mode agent's drop-in Environment / GymEnvironment on Catch-v0: one episode of 9 acts."""
    from src.environment import GymEnvironment
    env = GymEnvironment(make_config(random_seed=9, action_repeat=1, display=False))
    assert env.action_size == A and env.lives == 0
    screen, _, _, terminal = env.new_random_game()
    assert not terminal and tuple(screen.shape) == (84, 84)
    ref = C.CatchEnv(9, 1)
    ref.new_random_game()
    for t in range(9):
        c, _, p = C.decode(ref.frame)
        a = int(np.where(p > c, 1, np.where(p < c, 2, 0))[0])
        screen, reward, terminal = env.act(a, is_training=True)
        fr, rr, tt = ref.act(np.array([a]))
        assert (reward, terminal) == (float(rr[0]), bool(tt[0])) and terminal == (t == 8)
        assert np.array_equal(screen.cpu().numpy(), screens_of(fr)[0])
    assert reward == 1.0


# ------------------------------------------------------------------ engine parity
def stagger(eng, ref):
    """A check's start(eng, ref) hook.  Every env starts its first episode at reset, so all of them
    would land in the same step.  Put env e's ball in row (e * action_repeat) % 9 -- in the engine
    (both parity rows of its state) and the oracle alike --, so that with E = 6, n = 5 the landings,
    and the new games behind them, fall on every step position of the rollouts: an act moves the
    ball action_repeat rows, so the six envs are 1, 2, .. acts apart (repeat 2: an episode takes 5
    acts = one rollout, and rows 0, 2, 4, 6, 8, 1 land at t = 4, 3, 2, 1, 0, 3 of every rollout)."""
    env = ref.env
    c, _, p = C.decode(env.frame)
    r = (np.arange(ref.E) * env.action_repeat) % (C.ROWS - 1)
    env.frame[:] = C.encode(c, r, p).astype(np.uint32)
    env.ep_step[:] = r
    torch.cuda.synchronize()
    for key, v in (('frame', env.frame), ('ep_step', env.ep_step)):
        row = torch.as_tensor(v.astype(np.int32)).cuda()
        for parity in range(2):
            eng._env[key][parity].copy_(row)
    torch.cuda.synchronize()


def assert_landings_everywhere(ref, n):
    cells = np.asarray(ref.episode_counts['terminal_cells'])
    assert cells.shape[1] == n and (cells.sum(axis=0) >= 1).all(), cells.tolist()
    assert cells[:, :n - 1].sum() >= 1                       # new games started mid-rollout
    assert ref.episode_counts['game_overs'] == ref.episode_counts['terminals']     # every terminal is a reset


E6, N5 = 6, 5


@pytest.mark.parametrize('algo,kw', [('a3c', {}), ('q', {}), ('q', dict(action_repeat=2)),
                                     ('a3c', dict(dqn_type='nature', scale=2.0, learning_rate=2e-3))],
                         ids=['a3c-nips-sync', 'q-sync', 'q-sync-repeat2', 'nature-sync'])
def test_engine_sync_matches_oracle(catch_oracle, algo, kw):
    """E = 6, n = 5, 4 iterations of the synchronous engine: actions, rewards, clipped rewards,
    terminals, env state (frame indices) and ring exact; z, loss, gradients, parameters at
    check_sync_vs_oracle's bars."""
    eng, ref = EP.check_sync_vs_oracle(algo, A, E6, N5, 0, iters=4, seed=611, frames=FRAMES, start=stagger,
                                       **CATCH, **kw)
    assert isinstance(ref, C.CatchEngineRef) and eng.game == 'catch'
    assert_landings_everywhere(ref, N5)


@pytest.mark.parametrize('kw', [{}, dict(dqn_type='nature', scale=2.0, learning_rate=2e-3)], ids=['nips', 'nature'])
def test_engine_unfused_head_matches_oracle(catch_oracle, monkeypatch, kw):
    """A3C_FUSED_SCREEN=0: the unfused head (head_act's Catch form in k_head_fwd / k_nat_head, the whole
    act in one lane behind the draw) and the separate screen launch."""
    monkeypatch.setenv('A3C_FUSED_SCREEN', '0')
    _, ref = EP.check_sync_vs_oracle('a3c', A, E6, N5, 0, iters=4, seed=615, frames=FRAMES, start=stagger, **CATCH, **kw)
    assert_landings_everywhere(ref, N5)


def test_engine_overlap_matches_oracle(catch_oracle):
    """The default overlapped engine (k_head_screen_conv12's Catch form): 5 rollouts, 4 backwards."""
    _, ref = EP.check_overlap_vs_oracle(A, E6, N5, 0, rollouts=5, seed=612, frames=FRAMES, learning_rate=3e-3,
                                        start=stagger, **CATCH)
    assert isinstance(ref, C.CatchEngineRef)
    assert_landings_everywhere(ref, N5)


def test_engine_lstm_matches_oracle(catch_oracle):
    from test_gpu_lstm import check_lstm_sync_vs_oracle
    _, ref = check_lstm_sync_vs_oracle(A, E6, N5, 0, iters=4, seed=613, frames=FRAMES, learning_rate=2e-3,
                                       start=stagger, **CATCH)
    assert isinstance(ref, C.CatchEngineRef)
    assert_landings_everywhere(ref, N5)


def test_engine_gae_matches_reference(catch_oracle):
    """gae_lambda = 0.9 (test_gpu_gae's check): every rollout's env quantities exact against the
    oracle's replay, its returns the lambda-return of its own rewards, terminals and V rows, its
    loss the A3C loss at that target; the first rollout's gradient against the oracle backward on
    the engine's saved activations."""
    from test_gpu_gae import LAM, check_rollout, raw_gradient
    eng, ref, ns = EP.build('a3c', A, E6, N5, 0, seed=614, frames=FRAMES, gae_lambda=LAM, **CATCH)
    stagger(eng, ref)
    cells = np.zeros(N5, np.int64)
    for k in range(4):
        Pk = EP.unflat(eng, ns, eng.params) if k == 0 else None
        eng.iterate()
        torch.cuda.synchronize()
        terms, G32 = check_rollout(eng.slot(0), eng.loss.cpu().numpy(), A, N5, E6, ('catch', k))
        out = ref.iterate(forced_actions=eng.actions.cpu().numpy(), grads=False)
        assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards'])
        assert np.array_equal(terms, out['terminals'])
        ring = eng.frame_ring.cpu().numpy()
        assert np.array_equal(ring, ref.ring), k
        if Pk is not None:
            _, g_same = EP.same_act_grads(eng, EP.rollout_planes(ref, N5), Pk, 'a3c', A, N5, E6, G32)
            G = raw_gradient(eng, ns)
            for name, _ in ns:
                assert EP.rel_l2(G[name], g_same[name]) < 1e-4, (name, EP.rel_l2(G[name], g_same[name]))
        ref.tau += N5
        EP.assert_env_state(eng, ref, k)
        cells += terms.astype(np.int64).sum(axis=1)
    assert (cells >= 1).all(), cells


# ------------------------------------------------------------------ play
def play_pair(algo, E, seed, **kw):
    eng, ref, _ = EP.build(algo, A, E, N5, 0, seed=seed, frames=FRAMES, **CATCH, **kw)
    return eng, C.CatchEngineRef(ref.params, E, 1, A, algo, 0, FRAMES, seed)


def assert_catch_episodes(out):
    assert (out['lengths'] == C.ROWS - 1).all() and out['terminated'].all()
    assert set(out['returns'].tolist()) <= {-1.0, 1.0}


def test_play_in_waves(catch_oracle):
    """E = 6, 13 episodes (3 waves, the last with one env), cap 50: test_gpu_play's replay."""
    from test_gpu_play import check_play
    eng, pref = play_pair('a3c', E6, 621)
    out, r = check_play(eng, pref, 13, 50, tag='catch waves')
    assert r['waves'] == 3
    assert_catch_episodes(out)


def test_play_with_refill(catch_oracle):
    from test_gpu_play_refill import check_refill
    eng, pref = play_pair('a3c', E6, 622)
    out, r, capped = check_refill(eng, pref, 13, 50, tag='catch refill')
    assert capped == 0 and out['steps'] == 27                # 13 episodes of 9 steps on 6 envs: 3 rounds
    assert_catch_episodes(out)
    # the envs were stepped in lock-step: every refill took the six next indices in env-id order
    assert out['episode_env'].tolist() == [0, 1, 2, 3, 4, 5] * 2 + [0]


def test_play_random_policy_return(catch_oracle):
    """test_ep = 1 on a q engine is the uniformly random policy: 1024 episodes put 4 standard errors
    of a +-1 variable (sd <= 1: 4 / 32 = 0.125) inside 0.15 of the exact R_rand."""
    eng, _ = play_pair('q', 64, 623)
    out = eng.play(n_episode=1024, n_step=50, test_ep=1.0, refill=True)
    assert_catch_episodes(out)
    mean = float(out['returns'].mean())
    print('random policy: mean return', mean, 'exact', C.R_RAND)
    assert abs(mean - C.R_RAND) <= 0.15, (mean, C.R_RAND)


# ------------------------------------------------------------------ rejections
def test_rejections():
    from src import _lib
    from src.engine import Engine
    from src.environment import BatchedEnvironment
    for kw in (dict(frame84=1), dict(external_env=True), dict(num_frames=FRAMES - 1), dict(action_size=6),
               dict(start_lives=5)):
        args = dict(num_envs=4, n_step=2, action_size=A, num_frames=FRAMES)
        args.update(kw)
        with pytest.raises(_lib.A3CError, match='Catch') as ei:
            Engine(**args, **CATCH)
        assert ei.value.rc == _lib.ERR_INVALID, kw
    with pytest.raises(ValueError):
        Engine(num_envs=4, n_step=2, action_size=A, game='pong')
    with pytest.raises(_lib.A3CError, match='Catch') as ei:
        BatchedEnvironment(make_config(), num_envs=2, num_frames=FRAMES - 1)
    assert ei.value.rc == _lib.ERR_INVALID
    import ctypes
    h = ctypes.c_void_p()
    bad = _lib.lib().a3c_env_create_ex(2, A, 0, 30, 1, FRAMES, 1, 0, 2, ctypes.byref(h))      # no such game
    assert bad == _lib.ERR_INVALID and not h.value
    cfg = _lib.EngineConfig()
    _lib.lib().a3c_engine_config_default(ctypes.byref(cfg))
    cfg.net = _lib.net_desc(A)
    assert _lib.lib().a3c_engine_create_ex(ctypes.byref(cfg), 7, ctypes.byref(h)) == _lib.ERR_INVALID and not h.value
    Engine(num_envs=4, n_step=2, action_size=A, num_frames=FRAMES, **CATCH).close()            # the least pool


# ------------------------------------------------------------------ the command line
def test_main_trains_and_plays_catch(tmp_path, capsys):
    import json
    import main
    common = ['--mode', 'engine', '--env_name', 'Catch-v0', '--num_envs', '32', '--num_frames', '640', '--logdir',
              str(tmp_path)]
    eng = main.main(common + ['--iterations', '6', '--log_every', '3'])
    torch.cuda.synchronize()
    assert eng.game == 'catch' and eng.A == A and eng.overlap and torch.isfinite(eng.params).all()
    assert len(open(tmp_path / 'engine.jsonl').read().splitlines()) == 2
    capsys.readouterr()
    eng = main.main(common + ['--is_train', 'false', '--n_episode', '40', '--play_refill', 'true'])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert eng.game == 'catch' and rec['mode'] == 'play' and rec['checkpoint'] is not None
    assert rec['n_episode'] == 40 and rec['terminated'] == 40 and rec['mean_length'] == 9.0
    assert -1.0 <= rec['mean_reward'] <= 1.0 and rec['env_steps'] == 360


# ------------------------------------------------------------------ learning
LEARN_K = 1024


def test_engine_learns_catch():
    """The reason for all of the above: the default engine (a3c, nips, overlapped, 256 envs, n = 5,
    lr 7e-4, beta 0.01, RMSProp epsilon 0.1) trained LEARN_K iterations from the reference
    initialisers, then 1024 episodes played by sampling from the policy.  The bar is halfway from
    the random policy's exact return to the optimal one, R_rand + 0.5 (1 - R_rand) = 0.125, derived
    on the CPU (tests/_catch_ref.py): the untrained parameters play below it, the trained ones at
    or above it.

    LEARN_K: mean play return against iterations, measured on one MI355X for seeds 1 / 2 / 3 (the
    engine's and the initialiser's):  0: -0.754 / -0.744 / -0.736,  64: -0.756 / -0.717 / -0.727,
    128: -0.734 / -0.764 / -0.723,  256: -0.344 / -0.494 / -0.170,  512: 0.967 / 0.977 / 0.955,
    1024: 0.992 / 0.992 / 0.996,  2048: 0.996 / 0.998 / 0.998,  16384: 1.0 / 1.0 / 1.0.  512 is the
    smallest power of two at which all three clear the bar; LEARN_K is twice that (0.28 s of
    training)."""
    import main
    from src.engine import Engine
    seed = 1
    eng = Engine(num_envs=256, n_step=5, action_size=A, overlap=True, seed=seed, num_frames=FRAMES, **CATCH)
    eng.reset(main.initial_params(eng, A, 'a3c', seed))
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    before = eng.play(n_episode=1024, n_step=50, refill=True)
    for _ in range(LEARN_K):
        eng.iterate()
    after = eng.play(n_episode=1024, n_step=50, refill=True)
    assert_catch_episodes(before)
    assert_catch_episodes(after)
    r0, r1 = float(before['returns'].mean()), float(after['returns'].mean())
    print('catch: mean play return untrained', r0, 'after', LEARN_K, 'iterations', r1, 'bar', C.LEARNING_BAR)
    assert r0 < C.LEARNING_BAR, (r0, C.LEARNING_BAR)
    assert r1 >= C.LEARNING_BAR, (r1, C.LEARNING_BAR)
