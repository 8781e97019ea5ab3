"""first_screen without a GPU: the restated rule against the reference loop (what changes
in the ring, and that nothing else does), the masking argument on the targets, the flags, and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import _catch_memory_ref as M
import _catch_ref as C
import _first_screen_ref as F
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')
E, N, A, SEED = 4, 5, 3, 17
ROWS0 = [4, 4, 4, 6]          # three envs land at the rollout's last step, the fourth at t = 2
CASES = {'a3c': ('a3c', {}), 'q': ('q', {}), 'double_q': ('q', dict(double_q=True))}


def pair(algo, kw):
    """The reference-loop oracle and the first-screen oracle from the same parameters, at ROWS0."""
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    p = init_params(param_names_shapes(A, algo), seed=SEED, stddev=0.08)
    refs = []
    for cls in (M.CatchMemoryEngineRef, F.FirstScreenMemoryEngineRef):
        ref = cls(p, E, N, A, algo, 0, M.FRAMES, SEED, **kw)
        ref.reset()
        c, _, pc = C.decode(ref.env.frame)
        ref.env.frame[:] = C.encode(c, ROWS0, pc).astype(np.uint32)
        ref.env.ep_step[:] = ROWS0
        refs.append(ref)
    return refs


@pytest.fixture(scope='module')
def runs():
    """One rollout of both oracles under the same forced actions, per case: computed once, not changed."""
    rng = np.random.default_rng(5)
    forced = rng.integers(0, A, (N, E)).astype(np.int32)
    out = {}
    for name, (algo, kw) in CASES.items():
        plain, first = pair(algo, kw)
        out[name] = (plain, first, plain.iterate(forced, grads=False), first.iterate(forced, grads=False))
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_trajectories_and_ring(runs, name):
    plain, first, a, b = runs[name]
    assert isinstance(first, F.FirstScreen) and not isinstance(plain, F.FirstScreen)
    for k in ('actions', 'rewards', 'rewards_raw', 'terminals', 'game_overs'):
        assert np.array_equal(a[k], b[k]), k
    for f in ('frame', 'episode', 'ep_step', 'ep_len', 'lives'):
        assert np.array_equal(getattr(plain.env, f), getattr(first.env, f)), f
    terms = a['terminals'].astype(bool)
    want = np.zeros((N, E), bool)
    want[4, :3] = want[2, 3] = True
    assert np.array_equal(terms, want)
    differ = {(e, s) for e in range(E) for s in range(plain.R) if not np.array_equal(plain.ring[e, s], first.ring[e, s])}
    assert differ == {(e, (plain.tau + t + 1) % plain.R) for t, e in np.argwhere(terms)} and len(differ) == 4
    for t, e in np.argwhere(terms):
        f = int(b['frames'][t, e])
        c, r, p = (int(v) for v in C.decode(f))
        assert r == 0 and f != int(a['frames'][t, e]) and C.decode(int(a['frames'][t, e]))[1] == C.ROWS - 1
        plane = first.ring[e, (first.tau + t + 1) % first.R]
        assert np.array_equal(plane, R.screen(M.render(f)))
        assert not np.array_equal(plane, R.screen(M.render(C.encode(c, 1, p))))       # the ball is in it
    # env 3's new game: its frame record outside the terminal is the reference loop's
    assert np.array_equal(a['frames'][~terms], b['frames'][~terms])
    assert [t for t, _ in b['first_screens']] == [2, 4]


@pytest.mark.parametrize('name', sorted(CASES))
def test_landing_screen_reaches_no_target(runs, name):
    """The state that holds the landing screen as its newest plane is the s_{t+1} of a terminal
    transition, which every target multiplies by (1 - terminal): the envs whose only terminal is the
    rollout's last step have bit-equal targets.  The fourth env's later states hold the first screen."""
    _, _, a, b = runs[name]
    assert a['target'].dtype == np.float32
    assert np.array_equal(a['target'][:, :3], b['target'][:, :3])
    assert not np.array_equal(a['target'][:, 3], b['target'][:, 3])
    assert np.array_equal(a['target'][:3, 3], b['target'][:3, 3])       # up to its terminal at t = 2: masked too


# ------------------------------------------------------------------ flags
def test_flags():
    import main
    off = main.parse_flags(['--env_name', 'CatchMemory-v0', '--lstm', 'true'])
    on = main.parse_flags(['--env_name', 'CatchMemory-v0', '--lstm', 'true', '--first_screen', 'true'])
    assert off.first_screen is False and on.first_screen is True
    assert 'first_screen' not in main.engine_options(off)
    assert main.engine_options(on) == dict(main.engine_options(off), first_screen=True)
    assert main.engine_options(main.parse_flags(['--env_name', 'Catch-v0', '--first_screen', 'true']))['first_screen'] is True
    # the name does not switch it on: the options of the name stay Pong's
    assert main.engine_options(off) == main.engine_options(main.parse_flags(['--env_name', 'Pong-v0', '--lstm', 'true']))
    assert '--first_screen true' in main.__doc__


@pytest.mark.parametrize('argv', [['--mode', 'agent', '--env_name', 'CatchMemory-v0'],
                                  ['--mode', 'engine', '--env_name', 'Pong-v0'],
                                  ['--mode', 'engine', '--env_name', 'CatchMemory-v0', '--envs_on', 'host'],
                                  ['--mode', 'engine', '--env_name', 'Pong-v0', '--envs_on', 'gym']],
                         ids=['agent', 'pong', 'host', 'gym'])
def test_flag_rejections_before_device_work(monkeypatch, argv):
    import main
    from src import _lib
    monkeypatch.setattr(_lib, 'require_device', lambda: (_ for _ in ()).throw(AssertionError('device asked for')))
    with pytest.raises(ValueError, match='first_screen|device game'):
        main.main(argv + ['--first_screen', 'true'])
    if argv[1] == 'engine':
        with pytest.raises(ValueError, match='first_screen|device game'):
            main.engine_options(main.parse_flags(argv + ['--first_screen', 'true']))


def test_engine_rejects_before_device_work(monkeypatch):
    from src import _lib, engine
    monkeypatch.setattr(_lib, 'require_device', lambda: (_ for _ in ()).throw(AssertionError('device asked for')))
    for on in (True, False):
        with pytest.raises(ValueError, match='first_screen'):
            engine.Engine(action_size=3, first_screen=on)                      # game synth


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_setter():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+a3c_engine_set_first_screen\s*\((.*?)\)\s*;', src, re.S)
    assert m and [a.strip() for a in m.group(1).split(',')] == ['a3c_engine* eng', 'int on']
    text = open(HEADER).read()
    doc = text[text.index('first_screen (DESIGN 4l)'):text.index('int a3c_engine_set_first_screen')]
    assert 'agent.py:66-67' in doc and 'agent.py:366-367' in doc
    from src import _lib
    assert _lib.SIGNATURES['a3c_engine_set_first_screen'] == (_lib.c_int, [_lib.c_void_p, _lib.c_int])
    assert 'a3c_engine_set_first_screen' in _lib.OPTIONAL_IN_OLD_BUILDS
    assert ctypes.sizeof(_lib.EngineOpts) == 12 and ctypes.sizeof(_lib.EngineConfig) == 184       # neither grew


def test_setter_rejects_before_it_touches_the_device():
    """`on` is checked before the handle is looked at: with a NULL handle the message names the
    argument, and only 0 and 1 reach the NULL check.  No device is needed."""
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    from src import _lib
    lib = ctypes.CDLL(SO)
    lib.a3c_last_error.restype = ctypes.c_char_p
    fn = lib.a3c_engine_set_first_screen
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    for on, word in ((2, b'on must be'), (-1, b'on must be'), (0, b'null'), (1, b'null')):
        assert fn(None, on) == _lib.ERR_INVALID and word in lib.a3c_last_error(), (on, lib.a3c_last_error())
        assert b'a3c_engine_set_first_screen' in lib.a3c_last_error()
