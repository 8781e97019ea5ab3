"""first_screen on the GPU, against tests/_first_screen_ref.py: at a terminal the training
rollout writes the new game's first screen into the history where the reference loop writes the
landing's.  The engine in every kernel form under CatchMemory-v0's rules (1, 4), the ring's content,
that off is the engine as it was, that play is untouched, the rejections, the command line -- and
that the named game is now learned by the head with memory and still not by the one without.

Shapes and bars are tests/test_gpu_catch_memory.py's: E = 6, n = 5, 4 iterations, 640 frames, the
`stagger` start (terminals on every rollout position), the existing helpers with the oracle swapped
for the first-screen one: env quantities and the ring exact; z, losses, gradients and parameters at
the bars those helpers assert."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _catch_memory_ref as M  # noqa: E402
import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
import _first_screen_ref as F  # noqa: E402
from test_gpu_catch import E6, N5, assert_catch_episodes, assert_landings_everywhere, stagger  # noqa: E402
from test_gpu_catch_memory import screens_of  # noqa: E402

A, FRAMES = 3, M.FRAMES
MEM = dict(game='catch', catch_rules=M.RULES)
ON = dict(MEM, first_screen=True)
ORACLE = F.FirstScreenMemoryEngineRef


@pytest.fixture
def first_screen_oracle(monkeypatch):
    """The existing parity helpers build their oracle as EngineRef(...): make that the first-screen one."""
    import test_gpu_lstm
    monkeypatch.setattr(EP, 'EngineRef', ORACLE)
    monkeypatch.setattr(test_gpu_lstm, 'EngineRef', ORACLE)


def checked(eng, ref, n=N5):
    assert isinstance(ref, F.FirstScreen) and eng.first_screen and eng.catch_rules == M.RULES
    assert_landings_everywhere(ref, n)


# ------------------------------------------------------------------ 1. parity, every kernel form
@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_engine_sync_matches_oracle(first_screen_oracle, algo):
    checked(*EP.check_sync_vs_oracle(algo, A, E6, N5, 0, iters=4, seed=811, frames=FRAMES, start=stagger, **ON))


def test_engine_unfused_head_matches_oracle(first_screen_oracle, monkeypatch):
    """A3C_FUSED_SCREEN=0: head_act's Catch form and the separate screen launch, which reads the frame
    indices the head recorded."""
    monkeypatch.setenv('A3C_FUSED_SCREEN', '0')
    checked(*EP.check_sync_vs_oracle('a3c', A, E6, N5, 0, iters=4, seed=815, frames=FRAMES, start=stagger, **ON))


def test_engine_overlap_matches_oracle(first_screen_oracle):
    """k_head_screen_conv12's Catch forms: the next state's conv1 input is the first screen."""
    checked(*EP.check_overlap_vs_oracle(A, E6, N5, 0, rollouts=5, seed=812, frames=FRAMES, learning_rate=3e-3,
                                        start=stagger, **ON))


def test_engine_lstm_matches_oracle(first_screen_oracle):
    from test_gpu_lstm import check_lstm_sync_vs_oracle
    checked(*check_lstm_sync_vs_oracle(A, E6, N5, 0, iters=4, seed=813, frames=FRAMES, learning_rate=2e-3,
                                       start=stagger, **ON))


def test_engine_lstm_overlap_matches_oracle(first_screen_oracle):
    from test_gpu_lstm import check_lstm_overlap_vs_oracle
    checked(*check_lstm_overlap_vs_oracle(A, E6, N5, 0, rollouts=5, seed=814, frames=FRAMES, learning_rate=2e-3,
                                          start=stagger, **ON))


def test_engine_nature_matches_oracle(first_screen_oracle):
    """k_head_screen_fold's Catch form (E = 6, the shape tests/test_gpu_catch.py runs the nature trunk at)."""
    checked(*EP.check_sync_vs_oracle('a3c', A, E6, N5, 0, iters=4, seed=816, frames=FRAMES, start=stagger,
                                     dqn_type='nature', scale=2.0, learning_rate=2e-3, **ON))


def test_engine_graph_matches_oracle(first_screen_oracle):
    checked(*EP.check_sync_vs_oracle('a3c', A, E6, N5, 0, iters=4, seed=817, frames=FRAMES, start=stagger,
                                     use_graph=True, **ON))


def test_engine_q_nstep_matches_oracle(monkeypatch):
    import _qn_ref as Q
    oracle = type('FirstScreenNStepQ', (F.FirstScreen, Q.NStepQ, M.CatchMemoryEngineRef), {})
    monkeypatch.setattr(EP, 'EngineRef', oracle)
    eng, ref = EP.check_sync_vs_oracle('q', A, E6, N5, 0, iters=4, seed=818, frames=FRAMES, start=stagger, q_nstep=1, **ON)
    assert type(ref) is oracle and eng.cfg.q_nstep == 1
    checked(eng, ref)


# ------------------------------------------------------------------ 2. the ring's content
def test_ring_holds_first_screens():
    """After every rollout the ring is read on the host: the slot after each terminal is the screen of
    the new game's row-0 frame, which shows the ball (it differs from the same paddle's screen without
    one).  8 iterations of E = 6, n = 5 (240 env steps, 9 to an episode) so that at least 20 are seen."""
    from src.engine import Engine
    import main
    eng = Engine(num_envs=E6, n_step=N5, action_size=A, num_frames=FRAMES, seed=41, **ON)
    eng.reset(main.initial_params(eng, A, 'a3c', 41))
    env = M.CatchMemoryEnv(41, E6)
    env.new_random_game()

    class Both:
        pass
    both = Both()
    both.env, both.E = env, E6
    stagger(eng, both)
    tau, Rs, seen = 3, eng.ring_slots, 0
    for k in range(8):
        eng.iterate()
        torch.cuda.synchronize()
        assert int(eng.counters[0].item()) == tau + N5
        acts, terms = eng.actions.cpu().numpy(), eng.terminals.cpu().numpy()
        ring = eng.frame_ring.cpu().numpy()
        for t in range(N5):
            fr, _, term = env.act(acts[t])
            assert np.array_equal(term, terms[t].astype(bool)), (k, t)
            if term.any():
                env.new_random_game(term.copy())
            want = np.where(term, env.frame, fr)          # the frame whose screen the history gets
            for e in range(E6):
                plane = ring[e, (tau + t + 1) % Rs]
                assert np.array_equal(plane, screens_of([want[e]])[0]), (k, t, e)
                if term[e]:
                    c, r, p = (int(v) for v in C.decode(int(env.frame[e])))
                    assert r == 0
                    assert not np.array_equal(plane, screens_of([C.encode(c, 1, p)])[0]), (k, t, e)     # no ball there
                    seen += 1
        assert np.array_equal(eng.env_frame.cpu().numpy(), env.frame.astype(np.int32)), k
        tau += N5
    assert seen >= 20, seen


# ------------------------------------------------------------------ 3. off is off
def run4(**kw):
    from src.engine import Engine
    import main
    eng = Engine(num_envs=E6, n_step=N5, action_size=A, num_frames=FRAMES, seed=31, **MEM, **kw)
    eng.reset(main.initial_params(eng, A, 'a3c', 31))
    for _ in range(4):
        eng.iterate()
    torch.cuda.synchronize()
    return eng


def test_off_is_the_engine_as_it_was():
    from src.engine import Engine
    a, b, on = run4(), run4(first_screen=False), run4(first_screen=True)
    assert not a.first_screen and not b.first_screen and on.first_screen
    assert torch.equal(a.params, b.params) and torch.equal(a.frame_ring, b.frame_ring)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.env_frame, b.env_frame)
    assert not torch.equal(a.frame_ring, on.frame_ring)
    # not in the state blob: the sizes are equal, and an on-engine's blob loads into a plain engine
    blob = on.save_state()
    assert blob.size == a.save_state().size == b.save_state().size
    c = Engine(num_envs=E6, n_step=N5, action_size=A, num_frames=FRAMES, seed=31, **MEM)
    c.reset()
    c.load_state(blob)
    torch.cuda.synchronize()
    assert torch.equal(c.params, on.params) and torch.equal(c.frame_ring, on.frame_ring) and not c.first_screen


# ------------------------------------------------------------------ 4. play unchanged
@pytest.mark.parametrize('refill', [False, True], ids=['waves', 'refill'])
def test_play_is_unchanged(refill):
    from src.engine import Engine
    import main
    outs = []
    for kw in ({}, dict(first_screen=True)):
        eng = Engine(num_envs=E6, n_step=N5, action_size=A, num_frames=FRAMES, seed=722, **MEM, **kw)
        eng.reset(main.initial_params(eng, A, 'a3c', 722))
        outs.append(eng.play(n_episode=13, n_step=50, refill=refill))
        assert_catch_episodes(outs[-1])
    off, on = outs
    assert np.array_equal(off['returns'], on['returns']) and np.array_equal(off['lengths'], on['lengths'])
    if refill:
        assert off['steps'] == on['steps'] == 27


# ------------------------------------------------------------------ 5. rejections
def test_rejections_and_the_setter_mid_run():
    from src import _lib
    from src.engine import Engine
    import main
    with pytest.raises(ValueError, match='first_screen'):
        Engine(num_envs=4, n_step=2, action_size=A, first_screen=True)
    L = _lib.lib()
    synth = Engine(num_envs=4, n_step=2, action_size=A, num_frames=48)
    assert L.a3c_engine_set_first_screen(synth._h, 1) == _lib.ERR_INVALID and b'Catch' in L.a3c_last_error()
    eng = Engine(num_envs=E6, n_step=N5, action_size=A, num_frames=FRAMES, seed=51, **MEM)
    assert L.a3c_engine_set_first_screen(eng._h, 2) == _lib.ERR_INVALID and b'on must be' in L.a3c_last_error()
    eng.reset(main.initial_params(eng, A, 'a3c', 51))
    eng.rollout_grad()                            # a gradient computed and not applied
    assert L.a3c_engine_set_first_screen(eng._h, 1) == _lib.ERR_STATE and b'pending' in L.a3c_last_error()
    eng.apply()
    torch.cuda.synchronize()
    # mid-run, nothing pending: no reset is asked for, and the next terminal follows it.  All six envs
    # started at the reset, so they land together at env step 9: rollout 2's t = 3.
    slot = (3 + 9) % eng.ring_slots
    eng.set_first_screen(True)
    eng.iterate()
    torch.cuda.synchronize()
    assert eng.terminals.cpu().numpy()[3].all() and eng.first_screen
    frames = eng.env_frame.cpu().numpy()
    c, r, p = C.decode(frames)
    assert (r == 1).all()                         # one act into the new games, the paddle still frozen
    ring = eng.frame_ring.cpu().numpy()
    for e in range(E6):
        assert np.array_equal(ring[e, slot], screens_of([C.encode(c[e], 0, p[e])])[0]), e      # row 0: the ball
        assert not np.array_equal(ring[e, slot], screens_of([C.encode(c[e], 1, p[e])])[0]), e


# ------------------------------------------------------------------ 6. the command line
def test_main_trains_and_plays_with_first_screen(tmp_path, capsys):
    import json
    import main
    common = ['--mode', 'engine', '--env_name', 'CatchMemory-v0', '--lstm', 'true', '--first_screen', 'true',
              '--num_envs', '32', '--num_frames', '640', '--logdir', str(tmp_path)]
    eng = main.main(common + ['--iterations', '6', '--log_every', '3'])
    torch.cuda.synchronize()
    assert eng.first_screen and eng.game == 'catch' and eng.catch_rules == (1, 4) and eng.lstm and eng.overlap
    assert torch.isfinite(eng.params).all()
    capsys.readouterr()
    eng = main.main(common + ['--is_train', 'false', '--n_episode', '40', '--play_refill', 'true'])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert eng.first_screen and rec['mode'] == 'play' and rec['checkpoint'] is not None
    assert rec['n_episode'] == 40 and rec['terminated'] == 40 and rec['mean_length'] == 9.0
    assert -1.0 <= rec['mean_reward'] <= 1.0


# ------------------------------------------------------------------ 7, 8. learning
LEARN_K = 4096       # from the table in test_learning_with_memory_on_the_named_game's docstring
LEARN_N = 9
EPISODES = 4096
FOUR_SE = 4.0 / np.sqrt(EPISODES)         # |return| = 1: sd <= 1, 4 standard errors = 0.0625


def trained(lstm, first_screen, seed=1):
    import main
    from src.engine import Engine
    kw = dict(first_screen=True) if first_screen else {}
    eng = Engine(num_envs=256, n_step=LEARN_N, action_size=A, overlap=True, seed=seed, num_frames=FRAMES, lstm=lstm,
                 **MEM, **kw)
    eng.reset(main.initial_params(eng, A, 'a3c', seed))
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    before = eng.play(n_episode=EPISODES, n_step=50, refill=True)
    for _ in range(LEARN_K):
        eng.iterate()
    after = eng.play(n_episode=EPISODES, n_step=50, refill=True)
    assert_catch_episodes(before)
    assert_catch_episodes(after)
    return float(before['returns'].mean()), float(after['returns'].mean())


def test_learning_with_memory_on_the_named_game():
    """The LSTM engine on CatchMemory-v0 itself -- rules (1, 4), 256 envs, overlapped, n = 9, reference
    initialisers, default hyperparameters (RMSProp), seed 1 -- with first_screen: untrained below the bar,
    after LEARN_K iterations at or above it; the same engine without first_screen after the same LEARN_K
    stays below it (DESIGN §4k's finding).  The bar is the project's own, M.LEARNING_BAR = 47/336 =
    0.1399: halfway from R_ML to the optimal +1.  Mean return of 4096 episodes played by sampling
    (play, refill).

    LEARN_K from tools/catch_memory_learning.py --first_screen true --heads lstm, one MI355X, seeds
    1 / 2 / 3:
      n = 9, RMSProp:  0: -0.7192 / -0.7134 / -0.7139,  64: -0.7168 / -0.7300 / -0.7251,  128: -0.7173 /
        -0.7354 / -0.7295,  256: -0.7163 / -0.7124 / -0.7148,  512: -0.7222 / -0.7217 / -0.7261,  1024: 0.0786 /
        0.3647 / 0.3979,  2048: 0.9526 / 0.9956 / 0.8740,  4096: 0.9956 / 0.9976 / 0.9937,  8192: 0.9932 / 0.9990 /
        0.9966,  16384: 0.9883 / 0.9976 / 0.9922
      n = 5, RMSProp:  0: -0.7192 / -0.7134 / -0.7139,  64: -0.7104 / -0.7324 / -0.7280,  128: -0.7251 /
        -0.7280 / -0.7256,  256: -0.7109 / -0.7046 / -0.7148,  512: -0.7251 / -0.7183 / -0.7319,  1024: -0.7285 /
        -0.7134 / -0.7251,  2048: -0.7207 / -0.7217 / -0.7217,  4096: -0.7061 / -0.7231 / -0.7007,  8192: -0.6650 /
        -0.6313 / -0.6084,  16384: -0.6777 / -0.0986 / -0.5728      (no power of two clears: as under rules
        (2, 5), a 5-step rollout's BPTT does not span the 9-step episode)
    At n = 9, 2048 is the smallest power of two at which all three seeds clear the bar; LEARN_K is twice
    that (2.9 s of training; 16384 iterations took 11.4 s).  RMSProp clears, so Adam was not needed.  The
    feed-forward head with first_screen, seed 1, n = 9, stays at -0.7012 .. -0.7422 throughout (0: -0.7192,
    4096: -0.7183, 16384: -0.7012).  Without first_screen: DESIGN §4k's tables, -0.70 .. -0.74 to 16384.
    """
    bar = float(M.LEARNING_BAR)
    assert abs(bar - 47 / 336) < 1e-12
    r0, r1 = trained(True, True)
    print('first_screen lstm: mean play return untrained', r0, 'after', LEARN_K, 'iterations', r1, 'bar', bar)
    assert r0 < bar, (r0, bar)
    assert r1 >= bar, (r1, bar)
    _, r_off = trained(True, False)
    print('reference loop lstm: after', LEARN_K, 'iterations', r_off)
    assert r_off < bar, (r_off, bar)


def test_no_learning_without_memory():
    """The feed-forward engine under the same setup stays within 4 standard errors (0.0625) of R_ML =
    -121/168, untrained and trained: §4k's theorem is about play and any parameters, and play starts an
    episode from four copies of the first screen whatever training saw -- play was not touched."""
    assert FOUR_SE == 0.0625
    r_ml = float(M.R_ML)
    r0, r1 = trained(False, True)
    print('first_screen feed-forward: mean play return untrained', r0, 'after', LEARN_K, 'iterations', r1, 'R_ML', r_ml)
    assert abs(r0 - r_ml) <= FOUR_SE, (r0, r_ml)
    assert abs(r1 - r_ml) <= FOUR_SE, (r1, r_ml)
