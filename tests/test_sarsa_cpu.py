"""Asynchronous Sarsa (Engine(algo='q', sarsa=1)) without a GPU: the restatement the GPU tests
compare against (tests/_sarsa_ref.py) held to a brute-force definition, to its n = 1 identity and, with argmax
actions, to the max oracles; what the data sets and the engine-parity cases of tests/test_gpu_sarsa.py cover,
proved here so that no GPU case can pass without it -- the parity cases' seeds included: replayed by the oracle
alone, no draw at s_n is a near-tie, so the GPU check's near-tie allowance excuses nothing; the command line
(--sarsa); the options struct and the new symbols.

PARITY is the one table of both files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _catch_ref as C  # noqa: E402
import _qn_ref as Q  # noqa: E402
import _sarsa_ref as S  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_episode_ends_cpu import backprop, simulate  # noqa: E402
from test_q_nstep_cpu import catch_terminals  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')
DISCOUNT = 0.99

# the engine-parity cases of test_gpu_sarsa.py: the shapes of test_q_nstep_cpu.PARITY (check: the
# _engine_parity check that runs it; the overlap pipeline's last rollout has no backward), each env and each
# check with the one-step form and with q_nstep; lr: the learning rate the case runs with (default: the
# engine's).  ep_end_t: epsilon passes through (0, 1) inside the run, so
# the draws at s_n take both branches.
PARITY = {
    'sync': dict(check='sync', algo='q', A=6, E=8, n=3, rollouts=3, lives=5, seed=3501, q_nstep=0),
    'sync-nstep': dict(check='sync', algo='q', A=18, E=13, n=5, rollouts=3, lives=0, seed=3502, q_nstep=1),
    'overlap': dict(check='overlap', algo='q', A=6, E=16, n=5, rollouts=4, lives=0, seed=3503, q_nstep=0, lr=3e-3),
    'overlap-nstep': dict(check='overlap', algo='q', A=6, E=8, n=4, rollouts=4, lives=0, seed=3504, q_nstep=1, lr=3e-3),
    'host': dict(check='sync', algo='q', A=6, E=6, n=3, rollouts=3, lives=0, seed=3505, frames=40, host=True,
                 q_nstep=0, lr=2e-3),
    'catch-sync': dict(check='sync', algo='q', A=3, E=6, n=3, rollouts=4, lives=0, seed=3506, catch=True,
                       opts=dict(action_repeat=2), q_nstep=0),
    'catch-sync-nstep': dict(check='sync', algo='q', A=3, E=6, n=3, rollouts=4, lives=0, seed=3508, catch=True,
                             opts=dict(action_repeat=2), q_nstep=1),
    'catch-overlap': dict(check='overlap', algo='q', A=3, E=6, n=3, rollouts=5, lives=0, seed=3507, catch=True,
                          opts=dict(action_repeat=2), q_nstep=0, lr=3e-3),
    'catch-overlap-nstep': dict(check='overlap', algo='q', A=3, E=6, n=3, rollouts=5, lives=0, seed=3509, catch=True,
                                opts=dict(action_repeat=2), q_nstep=1, lr=3e-3),
}
# every case: epsilon from 1 down to the env's ep_end over 24 env steps, from the first step
EPS = dict(ep_end_t=24, learn_start=0)
TIE_MARGIN = 1e-4         # ten times assert_draws_explained's near-tie allowance


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize('n,E,A', [(1, 3, 2), (2, 5, 3), (5, 37, 6), (64, 9, 18)])
@pytest.mark.parametrize('nstep', [0, 1])
def test_restatement_equals_the_definition(n, E, A, nstep):
    """One-step: the same products, 1e-12 is generous; n-step: the recursion against the explicit sum of
    discounted rewards up to the first terminal -- the two round differently."""
    for normal in (False, True):
        for bad in (False, True):
            for d in S.op_cases(n, E, A, A + 2, normal_rewards=normal, bad_words=bad):
                rows = S.rows_of(d, nstep, n, E)
                args = (d['rewards'], d['terms'], d['actions'], d['boot'], rows, A, DISCOUNT, nstep)
                got = S.sarsa_target_ref(*args)
                r64 = S.sarsa_target_ref(*args, out_dtype=np.float64)
                want = S.sarsa_target_brute(*args)
                assert got.dtype == np.float32 and got.shape == (n, E) and np.isfinite(got).all()
                np.testing.assert_allclose(r64, want, rtol=1e-12, atol=1e-12)
                assert np.array_equal(r64.astype(np.float32), got)       # float32 is the last step only


@pytest.mark.parametrize('E,A', [(1, 1), (37, 6), (300, 18)])
def test_one_step_rollouts_have_one_form(E, A):
    """n = 1: the one-step and the n-step form are the same float64 operations."""
    for normal in (False, True):
        for d in S.op_cases(1, E, A, A + 2, normal_rewards=normal):
            one = S.sarsa_target_ref(d['rewards'], d['terms'], d['actions'], d['boot'], d['q'], A, DISCOUNT, 0)
            many = S.sarsa_target_ref(d['rewards'], d['terms'], d['actions'], d['boot'], d['q'], A, DISCOUNT, 1)
            assert np.array_equal(one, many)


@pytest.mark.parametrize('n,E,A', [(1, 5, 3), (5, 37, 6), (64, 9, 18), (2, 300, 1)])
def test_argmax_actions_give_the_max_targets(n, E, A):
    """With a' the first argmax of the same target rows, Sarsa is Q-learning: oracle.ref_cpu.td_target
    (one-step) and _qn_ref.nstep_q_target_ref (n-step), to the last bit."""
    for normal in (False, True):
        for d in S.op_cases(n, E, A, A + 2, normal_rewards=normal):
            acts, boot = S.argmax_actions(d['q'], n, E, A)
            one = S.sarsa_target_ref(d['rewards'], d['terms'], acts, boot, d['q'], A, DISCOUNT, 0)
            want = R.td_target(d['rewards'].reshape(-1), d['terms'].reshape(-1), d['q'][:, :A], DISCOUNT)
            assert np.array_equal(one, want.astype(np.float32).reshape(n, E))
            rows = S.rows_of(d, 1, n, E)
            many = S.sarsa_target_ref(d['rewards'], d['terms'], acts, boot, rows, A, DISCOUNT, 1)
            assert np.array_equal(many, Q.nstep_q_target_ref(d['rewards'], d['terms'], rows[:, :A], None, DISCOUNT))


def test_column_reduction():
    assert S.column(np.array([-1, 6, 2 ** 31 - 1, 5, 0], np.int32), 6).tolist() == [
        (2 ** 32 - 1) % 6, 0, (2 ** 31 - 1) % 6, 5, 0]
    assert S.column(np.array([-1, 7], np.int32), 1).tolist() == [0, 0]


# ------------------------------------------------------------------ 2. coverage of the op data
@pytest.mark.parametrize('E', S.OP_E)
@pytest.mark.parametrize('n', [n for n in S.OP_N if n >= 5])
def test_op_data_distinguishes_sarsa(n, E):
    """Every (n >= 5, E) of the GPU test, over the data sets it runs there: some targets differ from the max
    targets (both forms, A > 1); an env without a terminal (the bootstrap at full depth); terminals at i = 0,
    at an interior step, at i = n-1, two in a row; NaN outside the live columns; the out-of-range words are
    where the forms read them."""
    for A, zs in S.OP_AZS:
        for normal in (False, True):
            sets = S.op_cases(n, E, A, zs, normal_rewards=normal)
            terms = [d['terms'] for d in sets]
            assert any(t[0].any() for t in terms)
            assert any(t[1:n - 1].any() for t in terms)
            assert any(t[n - 1].any() for t in terms)
            assert any((t[:-1] & t[1:]).any() for t in terms)
            assert any((t.sum(axis=0) == 0).any() for t in terms)
            differs = [False, False]
            for d in sets:
                assert np.isnan(d['q'][:, A:]).all() and np.isfinite(d['q'][:, :A]).all()
                assert ((d['actions'] >= 0) & (d['actions'] < A)).all() and ((d['boot'] >= 0) & (d['boot'] < A)).all()
                if normal:
                    assert not set(np.unique(d['rewards'])) <= {-2.0, -1.0, 0.0, 1.0}
                else:
                    assert set(np.unique(d['rewards'])) <= {-2.0, -1.0, 0.0, 1.0}
                one = S.sarsa_target_ref(d['rewards'], d['terms'], d['actions'], d['boot'], d['q'], A, DISCOUNT, 0)
                mx = R.td_target(d['rewards'].reshape(-1), d['terms'].reshape(-1), d['q'][:, :A], DISCOUNT)
                differs[0] |= bool((one != mx.astype(np.float32).reshape(n, E)).any())
                rows = S.rows_of(d, 1, n, E)
                many = S.sarsa_target_ref(d['rewards'], d['terms'], d['actions'], d['boot'], rows, A, DISCOUNT, 1)
                mxn = Q.nstep_q_target_ref(d['rewards'], d['terms'], rows[:, :A], None, DISCOUNT)
                differs[1] |= bool((many != mxn).any())
                free = d['terms'].sum(axis=0) == 0
                if A > 1 and free.any():          # the boot action reaches step 0 of an env without a terminal
                    assert (many[0, free] != mxn[0, free]).any()
            assert differs == [A > 1, A > 1]
            bad = S.op_cases(n, E, A, zs, normal_rewards=normal, bad_words=True)
            words = {-1, A, 2 ** 31 - 1}
            assert all(set(d['boot'].tolist()) & words and set(d['actions'][1:].reshape(-1).tolist()) & words for d in bad)
            assert words <= set().union(*[set(d['boot'].tolist()) | set(d['actions'].reshape(-1).tolist()) for d in bad])


@pytest.mark.parametrize('E', S.OP_E)
def test_boot_data_takes_both_branches(E):
    """Every data set of the draw's GPU test: over its eps rows (all 0, all 1, mixed) both branches occur, the
    rows hold NaN outside the live columns; the tie set's maxima occur twice, so a last-maximum or any-maximum
    rule would differ from the first-maximum one somewhere."""
    for A, zs in S.OP_AZS:
        q, mixed = S.boot_cases(E, A, zs)
        assert np.isnan(q[:, A:]).all() and np.isfinite(q[:, :A]).all()
        assert ((mixed > 0) & (mixed < 1)).any() or E == 1
        took = set()
        for eps in (np.zeros(E, np.float32), np.ones(E, np.float32), mixed):
            for tau in S.BOOT_TAUS:
                a, random = S.boot_action_ref(q, eps, A, tau, env_id_base=3, seed=S.BOOT_SEED)
                assert ((a >= 0) & (a < A)).all()
                took |= set(random.tolist())
        assert took == {False, True}
        if A >= 2:
            qt, _ = S.boot_cases(E, A, zs, ties=True)
            top = qt[:, :A].max(axis=1, keepdims=True)
            assert ((qt[:, :A] == top).sum(axis=1) >= 2).all()
            first = np.argmax(qt[:, :A], axis=1)
            last = A - 1 - np.argmax(qt[:, :A][:, ::-1], axis=1)
            assert (first != last).all()
            a, _ = S.boot_action_ref(qt, np.zeros(E, np.float32), A, 5, seed=S.BOOT_SEED)
            assert np.array_equal(a, first)


def test_large_tau_uses_both_counter_words():
    """tau past 2^32 changes the draw through the counter's high word."""
    q, _ = S.boot_cases(300, 18, 20)
    eps = np.ones(300, np.float32)
    lo, _ = S.boot_action_ref(q, eps, 18, 7, seed=S.BOOT_SEED)
    hi, _ = S.boot_action_ref(q, eps, 18, 7 + 2 ** 32, seed=S.BOOT_SEED)
    assert not np.array_equal(lo, hi)
    assert 7 + 2 ** 32 in S.BOOT_TAUS


# ------------------------------------------------------------------ 3. the oracle and its adapter
@pytest.mark.parametrize('q_nstep', [0, 1])
def test_oracle_subclass_and_late_target_adapter_agree(q_nstep):
    """The two ways the GPU checks take the oracle's Sarsa target -- Sarsa.iterate (synchronous checks) and
    SarsaRc on the next states' rows (the overlap check's late targets, one rollout later) -- are one rule:
    equal while the target network has not moved, and not the max target."""
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    from oracle.engine_ref import EngineRef
    A, E, n, seed = 4, 3, 3, 3001
    p = init_params(param_names_shapes(A, 'q'), seed=seed, stddev=0.08)
    cls = S.NStepSarsaEngineRef if q_nstep else S.SarsaEngineRef
    ref = cls(p, E, n, A, 'q', 0, 16, seed, ep_end_t=24, learn_start=0)
    assert S.Sarsa.last is ref
    mx = (Q.NStepQEngineRef if q_nstep else EngineRef)(p, E, n, A, 'q', 0, 16, seed, ep_end_t=24, learn_start=0)
    for r in (ref, mx):
        r.reset()
        r.env.ep_len[:] = r.env.ep_step + np.array([1, 2, 50], np.uint32)      # terminals at t = 0 and t = 1
    acts = np.array([[0, 1, 2], [3, 0, 1], [2, 3, 0]], np.int32)
    out = ref.iterate(acts)
    old = mx.iterate(acts)
    assert out['terminals'][0, 0] and out['terminals'][1, 1] and not out['terminals'][:, 2].any()
    assert set(old) - {'q_boot'} <= set(out) and set(out['grads']) == set(old['grads'])
    nxt = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
    ref.tau += n
    ref.iterate(acts, grads=False)                    # the overlap check replays rollout k before the late targets of k-1
    rc = S.SarsaRc(n, E, A, q_nstep)
    qn = R.forward(ref.tparams, nxt, 'q', keep=False)['z'].astype(np.float32)
    late = rc.td_target(out['rewards'].reshape(-1), out['terminals'].reshape(-1), qn, DISCOUNT)
    assert np.array_equal(late.reshape(n, E), out['target'])
    assert rc.clip_by_norm is R.clip_by_norm                       # everything else is oracle.ref_cpu
    a_n = out['boot']['sampled'][0]
    assert np.array_equal(ref.boot_hist[0]['sampled'][0], a_n) and len(ref.boot_hist) == 2
    rows = qn[(n - 1) * E:] if q_nstep else qn
    assert np.array_equal(out['target'], S.sarsa_target_ref(out['rewards'], out['terminals'], acts, a_n, rows, A,
                                                            DISCOUNT, q_nstep))
    assert np.abs(out['target'] - old['target']).max() > 1e-6
    loss, _ = R.q_loss_and_dz(out['z_batch'], acts.reshape(-1), out['target'].reshape(-1).astype(np.float64))
    assert loss == out['losses']['loss'] and out['losses']['loss'] != old['losses']['loss']


# ------------------------------------------------------------------ 4. the parity cases
@pytest.mark.parametrize('name', list(PARITY))
def test_parity_case_covers_the_terminal_positions(name):
    """Every engine-parity case, from the env alone: among its back-propagated rollouts there are terminals at
    t = 0, at an interior t and at t = n-1, and a rollout in which some env has none."""
    case = PARITY[name]
    K, n, E = backprop(case), case['n'], case['E']
    if case.get('catch'):
        cells = catch_terminals(case)[:K].sum(axis=2)
    else:
        cells = simulate(case)['terms'][:K]
    assert cells[:, 0].sum() >= 1 and cells[:, n - 1].sum() >= 1 and cells[:, 1:n - 1].sum() >= 1, cells.tolist()
    assert (cells.sum(axis=1) < E).any(), cells.tolist()


@pytest.mark.parametrize('name', list(PARITY))
def test_parity_seed_has_no_near_tie_at_the_bootstrap_state(name):
    """The case replayed by the oracle alone, in the order its check replays it (S.oracle_alone): at every
    back-propagated rollout's s_n both branches of the draw are well apart -- |u - eps| and, on the greedy
    branch, the gap between the two largest Q values exceed TIE_MARGIN, ten times the allowance of
    assert_draws_explained -- and over the case both branches occur and some target differs from the max
    target by more than 1e-3."""
    case = PARITY[name]
    boots, differ = S.oracle_alone(case, EPS)
    assert len(boots) == case['rollouts']
    random = greedy = 0
    for k, b in enumerate(boots[:backprop(case)]):
        u, eps, z = b['u'][0], b['eps'][0], b['z'][0][:, :case['A']]
        assert (np.abs(u - eps) > TIE_MARGIN).all(), (name, k)
        g = u >= eps
        top2 = np.sort(z, axis=1)[:, -2:]
        gap = (top2[:, 1] - top2[:, 0]) / np.maximum(1.0, np.abs(z).max(axis=1))
        assert (gap[g] > TIE_MARGIN).all(), (name, k, gap[g].min())
        random += int((~g).sum())
        greedy += int(g.sum())
    print(name, 'draws at s_n: random', random, 'greedy', greedy, 'max |sarsa - max target|', differ)
    assert random >= 1 and greedy >= 1
    assert differ > 1e-3


# ------------------------------------------------------------------ 5. the command line
def test_sarsa_flag_reaches_the_engine_options():
    import main
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--sarsa', 'true'])) == dict(lstm=False, sarsa=1)
    kw = main.engine_options(main.parse_flags(['--algo', 'q', '--sarsa', 'true', '--q_nstep', 'true']))
    assert kw == dict(lstm=False, q_nstep=1, sarsa=1)
    for argv in (['--algo', 'q'], ['--algo', 'q', '--sarsa', 'false'], []):
        assert 'sarsa' not in main.engine_options(main.parse_flags(argv))
    # the dicts the existing tests expect are what they were
    assert main.engine_options(main.parse_flags([])) == dict(lstm=False)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'true'])) == dict(lstm=False, q_nstep=1)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--double_q', 'true'])) == dict(lstm=False,
                                                                                              double_q=True)
    f = main.parse_flags(['--mode', 'engine', '--algo', 'q', '--sarsa', 'true', '--n_step', '5', '--env_name', 'Catch-v0'])
    assert main.engine_options(f) == dict(lstm=False, sarsa=1)


def test_sarsa_flag_rejections():
    import main
    with pytest.raises(ValueError, match='--sarsa is a Q-learning option'):
        main.engine_options(main.parse_flags(['--sarsa', 'true']))
    with pytest.raises(ValueError, match='--sarsa with --double_q'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--sarsa', 'true', '--double_q', 'true']))
    with pytest.raises(ValueError, match='--sarsa is an engine option'):
        main.main(['--mode', 'agent', '--algo', 'q', '--sarsa', 'true'])
    # the existing rejections keep their text
    with pytest.raises(ValueError, match='--q_nstep is a Q-learning option'):
        main.engine_options(main.parse_flags(['--q_nstep', 'true']))
    with pytest.raises(ValueError, match='algo q has one-step TD targets'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--gae_lambda', '0.9']))


# ------------------------------------------------------------------ 6. the C structs and symbols
C_PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "a3c_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(a3c_engine_opts), offsetof(a3c_engine_opts, size),
         offsetof(a3c_engine_opts, game), offsetof(a3c_engine_opts, sarsa), sizeof(a3c_engine_config),
         offsetof(a3c_engine_config, gae_lambda));
  return 0;
}
'''


def test_opts_struct_matches_gcc(tmp_path):
    """a3c_engine_opts as gcc lays the header out against the ctypes mirror; a3c_engine_config is as large as
    it was (184 bytes, gae_lambda last)."""
    from src import _lib
    src = tmp_path / 'probe.c'
    src.write_text(C_PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    size, o_size, o_game, o_sarsa, cfg_size, lam = (int(v) for v in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.split())
    o = _lib.EngineOpts
    assert size == ctypes.sizeof(o) == 12
    assert (o_size, o_game, o_sarsa) == (o.size.offset, o.game.offset, o.sarsa.offset) == (0, 4, 8)
    assert [f[0] for f in o._fields_] == ['size', 'game', 'sarsa']
    assert cfg_size == ctypes.sizeof(_lib.EngineConfig) == 184 and lam == _lib.EngineConfig.gae_lambda.offset == 180
    assert _lib.EngineConfig._fields_[-1][0] == 'gae_lambda' and not hasattr(_lib.EngineConfig, 'sarsa')


NEW_SYMBOLS = ('a3c_engine_opts_default', 'a3c_engine_create_opts', 'a3c_engine_slot_boot_actions', 'a3c_boot_action',
               'a3c_sarsa_target')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    import torch  # noqa: F401  (share torch's HIP runtime, as the package does)
    return ctypes.CDLL(SO)


def test_new_symbols_and_default_options(lib):
    from src import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name + '(' in header, name
    o = _lib.EngineOpts(size=-1, game=9, sarsa=9)
    lib.a3c_engine_opts_default.restype = None
    lib.a3c_engine_opts_default.argtypes = [ctypes.POINTER(_lib.EngineOpts)]
    lib.a3c_engine_opts_default(ctypes.byref(o))
    assert (o.size, o.game, o.sarsa) == (ctypes.sizeof(_lib.EngineOpts), 0, 0)


def test_create_opts_rejects_before_it_allocates(lib):
    """The cases a3c_engine_create_opts rejects return A3C_ERR_INVALID from the argument checks, which run
    before anything touches the device: they do so on a machine without one."""
    from src import _lib
    lib.a3c_engine_config_default.restype = None
    lib.a3c_engine_config_default.argtypes = [ctypes.POINTER(_lib.EngineConfig)]
    lib.a3c_engine_opts_default.restype = None
    lib.a3c_engine_opts_default.argtypes = [ctypes.POINTER(_lib.EngineOpts)]
    lib.a3c_engine_create_opts.restype = ctypes.c_int
    lib.a3c_engine_create_opts.argtypes = [ctypes.POINTER(_lib.EngineConfig), ctypes.POINTER(_lib.EngineOpts),
                                           ctypes.POINTER(ctypes.c_void_p)]
    lib.a3c_last_error.restype = ctypes.c_char_p

    def create(algo='q', double_q=0, null_opts=False, **okw):
        cfg = _lib.EngineConfig()
        lib.a3c_engine_config_default(ctypes.byref(cfg))
        cfg.net = _lib.net_desc(6, algo, False, 'nips')
        cfg.num_envs, cfg.n_step, cfg.num_frames, cfg.double_q = 4, 2, 8, double_q
        o = _lib.EngineOpts()
        lib.a3c_engine_opts_default(ctypes.byref(o))
        for k, v in okw.items():
            setattr(o, k, v)
        h = ctypes.c_void_p(1)
        rc = lib.a3c_engine_create_opts(ctypes.byref(cfg), None if null_opts else ctypes.byref(o), ctypes.byref(h))
        assert h.value is None
        return rc, lib.a3c_last_error()

    for kw, word in ((dict(sarsa=2), b'sarsa must be 0 or 1'), (dict(sarsa=-1), b'sarsa must be 0 or 1'),
                     (dict(sarsa=1, algo='a3c'), b'sarsa is a Q-learning option'),
                     (dict(sarsa=1, double_q=1), b'sarsa with double_q'),
                     (dict(size=8), b'size'), (dict(size=0), b'size'), (dict(null_opts=True), b'opts'),
                     (dict(game=7), b'unknown game')):
        rc, msg = create(**kw)
        assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
