"""Every device form of Environment.screen on the painted pool (tests/_painted.py): the reference's
24 golden frames and 24 saturated, flat and hard-edged ones, in place of the hashed pool's white noise
(whose screens stay within bytes 54..197).

Ring tests (bit-exact).  The engine runs with num_frames = 48 and the painted pool; the oracle's env is
replayed with the engine's own actions, which names the frame of every step (no network pass); every
ring plane the rollouts wrote must equal the oracle's screen of that frame, and all 48 frames must
have entered the ring (tests/test_painted_cpu.py holds the seeds to that on the CPU).  E = 16, n = 5,
6 rollouts: every screen kernel is one workgroup (or one band set) per env.

The instantiations that inline atari::screen_frame<NT>, atari::copy_frame84<NT>, atari::screen_band or
a3c_preprocess_part, from a3c_forward_launch / a3c_nat_forward_launch (csrc/net_fwd.hip), enqueue_step
(csrc/engine.hip) and csrc/env.hip, and the case that reaches each (sync: the step owns the GPU, 1024
threads; overlap: LaunchMode::shared_gpu, 512):

  kernel                                      reached by                                case
  k_head_screen_conv12<true,  false>          NIPS conv fusion, steps 0..n-2, l2 re-read a3c-overlap-l2bits0, q-overlap,
                                                                                        a3c-sync-fused, q-sync-fused
  k_head_screen_conv12<true,  true>           the same with the ReLU bits (A3C_L2BITS=1) a3c-overlap-l2bits1
  k_head_screen_conv12<false, false>          a3c: the last step (conv of s_n, nothing   every a3c conv-fusion case
                                              saved); q runs no conv of s_n
  k_head_screen_conv12<false, true>           no default build: the last step saves no l2 bits (only the
                                              measurement build -DA3C_ABL_NOL1 pairs them) -- skipped
  k_head_screen_conv12, LSTM head on h        lstm=True, overlap                        lstm-overlap
  k_head_screen<1024, 256>                    NIPS sync (A3C_FUSE_CONV off: its default) a3c-sync, lstm-sync (h of the cell)
  k_head_screen<512, 256>                     NIPS overlap with A3C_FUSE_CONV=0         a3c-overlap-unfused
  k_head_screen<1024, 512>, <512, 512>        nature sync, overlap                      nature-sync, nature-overlap
  k_env_screen (screen_band)                  A3C_FUSED_SCREEN=0; ext_observe           unfused-screen, host-env
  copy_frame84<512> in k_head_screen_conv12   frame84 = 1, NIPS overlap                 frame84-overlap
  copy_frame84<1024> in k_head_screen<.,512>  frame84 = 1, nature sync                  frame84-nature-sync
  k_head_screen_conv12<., ., A3C_GAME_CATCH>  game catch, overlap                       catch-overlap
  k_head_screen_play<1024, 256>, <512, 256>   Engine.play, NIPS sync / overlap engine   play-nips, play-nips-overlap
  k_head_screen_play<1024, 512>               Engine.play, nature                       play-nature
  k_play_begin_screens (a3c_preprocess_part)  the first screens of every play wave      the play cases
  k_play_observe_refill (screen_frame<512>)   Engine.play(refill=True)                  play-refill
  k_env_init_screens (a3c_preprocess_part)    a3c_engine_ext_begin                      host-env
  a3c_env_screen (k_env_screen)               BatchedEnvironment.screens                batched-env
  k_head_screen_fold<., 512>                  only with the A/B knob A3C_NAT_FOLD_HEAD of a -DA3C_KNOBS build -- skipped
  k_screen_atari, k_preprocess                the standalone entry points               tests/test_gpu_kernels.py

(The Catch forms of k_head_screen / k_head_screen_play and the device reset's k_env_init_screens see their
own pools only: one Catch engine is painted, and a reset fills the pool by hash again.)  Play episodes are
capped at a few steps so that every plane of the play ring is known; the bar there is 40 of the 48 frames.

Full parity on painted frames: the parity checks of tests/_engine_parity.py and tests/test_gpu_lstm.py,
their bars unchanged, with start = paint -- conv1's u8 operand (k_head_screen_conv12's bf16 hand-off,
k_conv12_fwd<.., U8>, k_nat_conv1_bf, the conv1 weight gradient) and everything above it on inputs over
0..254.  The largest independent rel-L2 (bar 2e-2) each case saw on an MI355X is noted beside it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
import _painted as P  # noqa: E402
from _play_ref import play_ref, ref_like  # noqa: E402
from _play_refill_ref import play_refill_ref  # noqa: E402
from oracle.engine_ref import EngineRef  # noqa: E402
from oracle.synthetic_env import SyntheticAtari  # noqa: E402

E, N, ITERS = P.RING_E, P.RING_N, P.RING_ITERS
ALL = set(range(P.N_FRAMES))
HOOKS = dict(paint=P.paint, paint84=P.paint84, paint_catch=P.paint_catch)


def describe(got, want):
    d = got != want
    ys, xs = np.nonzero(d)
    return f'{int(d.sum())} px differ, rows {ys.min()}..{ys.max()} cols {xs.min()}..{xs.max()}'


class Tally:
    """Planes compared, frames seen, and the planes that differ (env, step, frame, where)."""

    def __init__(self, label):
        self.label, self.planes, self.seen, self.bad = label, 0, set(), []

    def plane(self, got, f, env, step):
        want = P.painted_screens()[int(f) % P.N_FRAMES]
        self.planes += 1
        self.seen.add(int(f) % P.N_FRAMES)
        if not np.array_equal(got, want):
            self.bad.append(f'env {env} step {step} frame {int(f)}: {describe(got, want)}')

    def finish(self, at_least=P.N_FRAMES):
        print(f'painted ring {self.label}: {self.planes} planes compared, {len(self.seen)} distinct frames')
        for line in self.bad[:16]:
            print('  ', line)
        assert not self.bad, (self.label, len(self.bad), self.bad[:4])
        assert len(self.seen) >= at_least, (self.label, 'frames seen', sorted(self.seen), 'missing', sorted(ALL - self.seen))


def make(case, monkeypatch):
    """The engine and the oracle of a ring case, learning rate 0 (the ring does not depend on it)."""
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    kw = dict(case['kw'], learning_rate=0.0)
    if case['lstm']:
        from test_gpu_lstm import build
        return build(case['A'], E, N, case['lives'], case['seed'], **kw)[:2]
    frames = P.N_FRAMES
    if case['game'] == 'catch':
        monkeypatch.setattr(EP, 'EngineRef', C.CatchEngineRef)
        kw['game'], frames = 'catch', C.FRAMES
    if kw.get('dqn_type') == 'nature':
        kw['scale'] = 2.0
    return EP.build(case['algo'], case['A'], E, N, case['lives'], case['seed'], frames=frames, **kw)[:2]


def rollouts(eng, ref, tally, iterate, tau=3):
    """ITERS rollouts: every plane they write against the screen of the frame the replayed env names."""
    R = eng.ring_slots
    for k in range(ITERS):
        iterate()
        torch.cuda.synchronize()
        acts = eng.slot(k & 1 if eng.overlap else 0)['actions'].cpu().numpy()
        frames = P.step_frames(ref, acts)
        ring = eng.frame_ring.cpu().numpy()
        for t in range(N):
            for e in range(E):
                tally.plane(ring[e, (tau + t + 1) % R], frames[t, e], e, k * N + t)
        tau += N
        if not eng.external_env:     # the replay is in lock-step with the device env
            assert np.array_equal(eng._env['frame'][tau & 1].cpu().numpy(), ref.env.frame.astype(np.int32)), k


DEVICE_CASES = sorted(k for k, c in P.RING_CASES.items() if not c['kw'].get('external_env'))


@pytest.mark.parametrize('name', DEVICE_CASES)
def test_ring_on_painted_frames(name, monkeypatch):
    case = P.RING_CASES[name]
    eng, ref = make(case, monkeypatch)
    HOOKS[case['hook']](eng, ref)
    tally = Tally(name)
    rollouts(eng, ref, tally, eng.iterate)
    tally.finish()


class HostPaintedEnv:
    """One synthetic env stepped on the host whose frames are the painted ones (HostEnvPool's interface)."""

    def __init__(self, seed, e, A, lives):
        self.env = SyntheticAtari(seed, 1, P.N_FRAMES, A, lives, env_id_base=e)

    def _rgb(self):
        return P.painted_frames()[int(self.env.frame[0])]

    def new_random_game(self):
        self.env.new_random_game()
        return self._rgb(), 0, 0, bool(self.env.terminal[0])

    def act(self, action, is_training=True):
        _, r, t = self.env.act(np.array([action]), is_training=is_training)
        return self._rgb(), float(r[0]), bool(t[0])


def test_host_env_ring_on_painted_frames(monkeypatch):
    """a3c_engine_ext_begin -> k_env_init_screens (the four begin planes), then ext_observe -> k_env_screen."""
    from src.host_env import HostEnvPool
    case = P.RING_CASES['host-env']
    eng, built = make(case, monkeypatch)
    ref = EngineRef(built.params, E, N, case['A'], case['algo'], case['lives'], P.N_FRAMES, case['seed'],
                    learning_rate=0.0)
    P.tell(ref, lambda f: P.painted_screens()[int(f)])       # before its reset: the begin planes are painted too
    ref.reset()
    pool = HostEnvPool([HostPaintedEnv(case['seed'], e, case['A'], case['lives']) for e in range(E)], threads=1)
    tally = Tally('host-env')
    try:
        eng.begin_host(pool)
        torch.cuda.synchronize()
        ring = eng.frame_ring.cpu().numpy()
        for e in range(E):
            for c in range(4):
                tally.plane(ring[e, c % eng.ring_slots], ref.env.frame[e], e, f'begin {c}')
        rollouts(eng, ref, tally, lambda: eng.iterate_host(pool))
    finally:
        pool.close()
    tally.finish()


def test_batched_environment_on_painted_frames():
    """BatchedEnvironment with a painted frame_pool: a3c_env_screen after new_random_game and every act."""
    from src.environment import BatchedEnvironment
    from test_gpu_dropin import make_config
    c = P.BATCHED_ENV_CASE
    env = BatchedEnvironment(make_config('Pong-v0', action_repeat=1, random_start=30), num_envs=c['E'], seed=c['seed'],
                             num_frames=P.N_FRAMES)
    ref = SyntheticAtari(c['seed'], c['E'], P.N_FRAMES, c['A'], 0, 30, 1, 0)
    P.to_pool(env, P.painted_frames())
    tally = Tally('batched-env')
    rng = np.random.default_rng(c['seed'])
    screens = env.new_random_game()[0].cpu().numpy()
    ref.new_random_game()
    for t in range(c['steps'] + 1):
        for e in range(c['E']):
            tally.plane(screens[e], ref.frame[e], e, t)
        a = rng.integers(0, c['A'], c['E']).astype(np.int32)
        screens = env.act(a)[0].cpu().numpy()
        ref.act(a)
    tally.finish()


# ---------------------------------------------------------------------------------- play
def play_pair(seed, hook=P.paint, **kw):
    """An engine, the play restatement told the painted screens, and its twin told planes that name
    their frame (the same replay on both says which frame every slot of the play ring holds)."""
    if kw.get('dqn_type') == 'nature':
        kw['scale'] = 2.0
    eng, ref, _ = EP.build('a3c', 6, E, N, 0, seed, **kw)
    pref, ids = ref_like(ref), ref_like(ref)
    hook(eng, pref)
    P.tell(ids, P.id_plane)
    return eng, pref, ids


def compare_play_ring(eng, pref, ids, tally, call, only=None):
    """The whole play ring of every env against the restatement's; only(e, slot): count the plane."""
    pb = eng.play_buffers()
    ring, R = pb['ring'].cpu().numpy(), pb['ring_slots']
    assert R == pref.R == ids.R
    for e in range(E):
        for s in range(R):
            f = int(ids.ring[e, s, 0, 0])
            assert np.array_equal(pref.ring[e, s], P.painted_screens()[f])
            if only is None or only(e, s):
                tally.plane(ring[e, s], f, e, f'call {call} slot {s}')
            else:
                assert np.array_equal(ring[e, s], pref.ring[e, s]), (call, e, s, describe(ring[e, s], pref.ring[e, s]))


@pytest.mark.parametrize('name,seed,kw', [('play-nips', 721, {}), ('play-nips-overlap', 722, dict(overlap=True)),
                                          ('play-nature', 723, dict(dqn_type='nature'))],
                         ids=['play-nips', 'play-nips-overlap', 'play-nature'])
def test_play_ring_on_painted_frames(name, seed, kw):
    """Waves of E episodes capped at 4 steps, 6 calls: the ring's 5 slots then hold the wave's first
    screen (k_play_begin_screens) and its 4 steps' (k_head_screen_play), all of which are compared."""
    eng, pref, ids = play_pair(seed, **kw)
    tally = Tally(name)
    for call in range(6):
        out = eng.play(n_episode=E, n_step=4, trace=True)
        acts = out['actions'].cpu().numpy()
        for r in (pref, ids):
            res = play_ref(r, E, 4, forced_actions=acts, forward=False)
        assert not out['terminated'].any() and not res['terminated'].any()     # every env took its 4 steps
        assert np.array_equal(out['lengths'], res['lengths'])
        compare_play_ring(eng, pref, ids, tally, call)
    tally.finish(at_least=40)


def test_play_refill_ring_on_painted_frames():
    """Play with refill, 2 E episodes capped at 1 step, 10 calls: at the cap every env takes a new
    episode, whose first screen k_play_observe_refill writes into the four newest slots; the last slot
    holds the second episode's step (k_head_screen_play).  The refilled planes alone must show 40 frames."""
    eng, pref, ids = play_pair(724)
    tally, refilled = Tally('play-refill'), Tally('play-refill, the planes k_play_observe_refill wrote')
    for call in range(10):
        out = eng.play(n_episode=2 * E, n_step=1, trace=True, refill=True)
        acts = out['actions'].cpu().numpy()
        for r in (pref, ids):
            res = play_refill_ref(r, 2 * E, 1, forced_actions=acts, forward=False)
        assert not out['terminated'].any() and np.array_equal(out['episode_tau0'], res['episode_tau0'])
        R = pref.R
        begun = {(int(res['episode_env'][i]), (int(res['episode_tau0'][i]) - 3 + c) % R)
                 for i in range(E, 2 * E) for c in range(4)}
        stepped = {(int(res['episode_env'][i]), (int(res['episode_tau0'][i]) + 1) % R) for i in range(E, 2 * E)}
        assert len(begun) == 4 * E and not begun & stepped
        compare_play_ring(eng, pref, ids, tally, call)
        compare_play_ring(eng, pref, ids, refilled, call, only=lambda e, s: (e, s) in begun)
    refilled.finish(at_least=40)
    tally.finish(at_least=40)


# ---------------------------------------------------------------------------------- full parity
PE, PN = 8, 3
NAT = dict(dqn_type='nature', scale=2.0, learning_rate=2e-3)


def saw_the_byte_range(ref):
    """The oracle's ring at the end of a check (the engine's, bit for bit) holds bytes 0 and 254: the
    states the last rollouts ran on were painted ones, not the hashed pool's 54..197."""
    assert ref.ring.min() == 0 and ref.ring.max() == 254, (int(ref.ring.min()), int(ref.ring.max()))


def test_parity_sync_a3c_on_painted_frames():
    """Largest independent rel-L2 seen: 2.0e-06."""
    saw_the_byte_range(EP.check_sync_vs_oracle('a3c', 6, PE, PN, 3, iters=3, seed=731, start=P.paint)[1])


@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_parity_overlap_on_painted_frames(algo):
    """Largest independent rel-L2 seen: a3c 1.7e-06, q 7.2e-07."""
    saw_the_byte_range(EP.check_overlap_vs_oracle(6, PE, PN, 0, rollouts=4, seed=732, learning_rate=3e-3, algo=algo,
                                                  start=P.paint)[1])


def test_parity_nature_sync_on_painted_frames():
    """Largest independent rel-L2 seen: 1.1e-06."""
    saw_the_byte_range(EP.check_sync_vs_oracle('a3c', 6, PE, PN, 0, iters=3, seed=733, start=P.paint, **NAT)[1])


def test_parity_nature_overlap_on_painted_frames():
    """Largest independent rel-L2 seen: 1.0e-06."""
    saw_the_byte_range(EP.check_overlap_vs_oracle(6, PE, PN, 0, rollouts=4, seed=734, start=P.paint, **NAT)[1])


def test_parity_lstm_sync_on_painted_frames():
    """(check_lstm_sync_vs_oracle asserts its 2e-2 independent bound per tensor and reports no maximum.)"""
    from test_gpu_lstm import check_lstm_sync_vs_oracle
    saw_the_byte_range(check_lstm_sync_vs_oracle(6, PE, PN, 3, iters=3, seed=735, learning_rate=2e-3,
                                                 start=P.paint)[1])
