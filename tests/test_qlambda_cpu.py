"""lambda-return targets of the Q engine (Engine(algo='q', q_lambda=...)) without a GPU: the
restatement the GPU tests compare against (tests/_qlambda_ref.py) held to the brute-force definition and, at
lambda = 0 and lambda = 1, to the one-step and n-step restatements bit for bit; what the engine-parity cases of
tests/test_gpu_qlambda.py cover, proved here on the oracle alone so that no GPU case can pass without it -- the
cases' seeds included: no draw of theirs is a near-tie, so the GPU checks' near-tie allowance excuses nothing;
the command line (--q_lambda); the header's new symbols and the two pinned struct sizes.

PARITY is the one table of both files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _qlambda_ref as L  # noqa: E402
import _qn_ref as Q  # noqa: E402
import _sarsa_ref as S  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_episode_ends_cpu import backprop, simulate  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')
DISCOUNT = 0.99
LAM = 0.7

# the engine-parity cases of test_gpu_qlambda.py (check: the _engine_parity check that runs it; the overlap
# pipeline's last rollout has no backward): sync at E = 8 and overlap at E = 16, n = 5 and one case at n = 1,
# the three forms, lambda = 0.7, lives = 5 (Breakout's; the scheduled game overs put terminals inside the
# rollouts); lr: the learning rate the case runs with (default: the engine's).
PARITY = {
    'sync-q': dict(check='sync', form='q', A=6, E=8, n=5, rollouts=3, lives=5, seed=4101, lam=LAM),
    'sync-double': dict(check='sync', form='double', A=6, E=8, n=5, rollouts=3, lives=5, seed=4102, lam=LAM),
    'sync-sarsa': dict(check='sync', form='sarsa', A=6, E=8, n=5, rollouts=3, lives=5, seed=4103, lam=LAM),
    'sync-sarsa-n1': dict(check='sync', form='sarsa', A=6, E=8, n=1, rollouts=6, lives=5, seed=4104, lam=LAM),
    'overlap-q': dict(check='overlap', form='q', A=6, E=16, n=5, rollouts=4, lives=5, seed=4105, lam=LAM, lr=3e-3),
    'overlap-double': dict(check='overlap', form='double', A=6, E=16, n=5, rollouts=4, lives=5, seed=4106, lam=LAM,
                           lr=3e-3),
    'overlap-sarsa': dict(check='overlap', form='sarsa', A=6, E=16, n=5, rollouts=4, lives=5, seed=4127, lam=LAM,
                          lr=3e-3),
}
# every case: epsilon from 1 down to the env's ep_end over 24 env steps, from the first step
EPS = dict(ep_end_t=24, learn_start=0)
TIE_MARGIN = 1e-4         # ten times assert_draws_explained's near-tie allowance

SHAPES = [(n, E) for n in L.OP_N for E in L.OP_E]


def covers(cells, n, E):
    """The coverage condition on the terminals per (rollout, t) cell [backprop, n]: a terminal in the first
    cell, in the last cell, in a middle cell (where n has one), and a rollout in which not every env ends."""
    cells = np.asarray(cells)
    middle = cells[:, 1:n - 1].sum() >= 1 if n >= 3 else True
    return bool(cells[:, 0].sum() >= 1 and cells[:, n - 1].sum() >= 1 and middle and (cells.sum(axis=1) < E).any())


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize('n,E', SHAPES)
def test_recursion_equals_the_definition(n, E):
    """lambda_q_target_ref against lambda_q_target_brute, 1e-12 relative in float64: every (A, zs), the three
    forms, lambda in (0, 0.3, 0.95, 1), clipped and standard-normal rewards (E = 300: the clipped set), in-range
    actions and out-of-range words.  The float32 result is the float64 one rounded, nothing else."""
    for A, zs in L.OP_AZS:
        for normal in ((False,) if E >= 300 else (False, True)):
            for d in L.op_cases(n, E, A, zs, normal_rewards=normal, bad_words=True):
                for form in L.FORMS:
                    for lam in L.OP_LAMBDAS:
                        args = (d['rewards'], d['terms'], d['q'], A, DISCOUNT, lam)
                        kw = L.form_args(d, form)
                        r64 = L.lambda_q_target_ref(*args, out_dtype=np.float64, **kw)
                        want = L.lambda_q_target_brute(*args, **kw)
                        assert r64.shape == (n, E) and np.isfinite(r64).all() and np.abs(r64).max() < 1e6
                        np.testing.assert_allclose(r64, want, rtol=1e-12, atol=1e-12)
                        got = L.lambda_q_target_ref(*args, **kw)
                        assert got.dtype == np.float32 and np.array_equal(r64.astype(np.float32), got)


@pytest.mark.parametrize('n,E', SHAPES)
def test_endpoints_are_the_existing_rules_bit_for_bit(n, E):
    """On the same data lambda = 0 is ref_cpu.td_target / td_target_double / sarsa_target_ref(nstep = 0) and
    lambda = 1 is nstep_q_target_ref / sarsa_target_ref(nstep = 1) on the rows of s_n, array_equal; lambda = 0.5
    differs from both wherever the two ends differ at all (n >= 2, A >= 2)."""
    for A, zs in L.OP_AZS:
        for normal in (False, True):
            for d in L.op_cases(n, E, A, zs, normal_rewards=normal):
                r, t, q = d['rewards'], d['terms'], d['q']
                live, last = q[:, :A], q[(n - 1) * E:]
                ends = dict(
                    q=(R.td_target(r.reshape(-1), t.reshape(-1), live, DISCOUNT),
                       Q.nstep_q_target_ref(r, t, last[:, :A], None, DISCOUNT)),
                    double=(R.td_target_double(r.reshape(-1), t.reshape(-1), live, d['q_sel'][:, :A], DISCOUNT),
                            Q.nstep_q_target_ref(r, t, last[:, :A], d['q_sel'][(n - 1) * E:, :A], DISCOUNT)),
                    sarsa=(S.sarsa_target_ref(r, t, d['actions'], d['boot'], q, A, DISCOUNT, 0),
                           S.sarsa_target_ref(r, t, d['actions'], d['boot'], last, A, DISCOUNT, 1)))
                for form in L.FORMS:
                    kw = L.form_args(d, form)
                    one, many = (np.asarray(v).astype(np.float32).reshape(n, E) for v in ends[form])
                    got0 = L.lambda_q_target_ref(r, t, q, A, DISCOUNT, 0.0, **kw)
                    got1 = L.lambda_q_target_ref(r, t, q, A, DISCOUNT, 1.0, **kw)
                    assert np.array_equal(got0, one), (A, zs, form, normal)
                    assert np.array_equal(got1, many), (A, zs, form, normal)
                    half = L.lambda_q_target_ref(r, t, q, A, DISCOUNT, 0.5, **kw)
                    if n == 1:
                        assert np.array_equal(one, many) and np.array_equal(half, one)
                    elif A >= 2 and E >= 5:
                        assert (one != many).any()
                        assert (half != one).any() and (half != many).any(), (A, zs, form, normal)


def test_forms_differ_and_padding_is_never_read():
    """The three forms give different targets on the op data (A >= 2), and the columns >= A change nothing."""
    n, E = 5, 37
    for A, zs in L.OP_AZS:
        d, = L.op_cases(n, E, A, zs)
        nan, = L.op_cases(n, E, A, zs, pad=np.nan)
        got = {}
        for form in L.FORMS:
            got[form] = L.lambda_q_target_ref(d['rewards'], d['terms'], d['q'], A, DISCOUNT, LAM, **L.form_args(d, form))
            other = L.lambda_q_target_ref(nan['rewards'], nan['terms'], nan['q'], A, DISCOUNT, LAM,
                                          **L.form_args(nan, form))
            assert np.array_equal(got[form], other)
        if zs > A:
            assert (d['q'][:, A:] == L.PAD).all() and (d['q_sel'][:, A:] == L.PAD).all()
        if A >= 2:
            assert (got['q'] != got['double']).any() and (got['q'] != got['sarsa']).any()
            assert (got['double'] != got['sarsa']).any()


def test_op_data_holds_every_bad_word_where_it_is_read():
    for n, E in ((2, 1), (5, 37), (64, 300)):
        for A, zs in L.OP_AZS:
            sets = L.op_cases(n, E, A, zs, bad_words=True)
            words = {-1, A, 2 ** 31 - 1, -2 ** 31}
            seen = set()
            for d in sets:
                seen |= set(d['boot'].tolist()) | set(d['actions'][1:].reshape(-1).tolist())
            assert words <= seen or E == 1, (n, E, A, sorted(seen & words))
            assert seen & words


# ------------------------------------------------------------------ 2. the oracle and its adapter
@pytest.mark.parametrize('form', L.FORMS)
def test_oracle_subclass_and_late_target_adapter_agree(form):
    """The two ways the GPU checks take the oracle's lambda target -- QLambda.iterate (synchronous checks) and
    QLambdaRc on the next states' rows (the overlap check's late targets, one rollout later) -- are one rule:
    equal while the target network has not moved, and neither the one-step nor the n-step target."""
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    A, E, n, seed = 4, 3, 3, 3001
    p = init_params(param_names_shapes(A, 'q'), seed=seed, stddev=0.08)
    kw = dict(ep_end_t=24, learn_start=0, **(dict(double_q=1) if form == 'double' else {}))
    ref = L.oracle_class(LAM, sarsa=form == 'sarsa')(p, E, n, A, 'q', 0, 16, seed, **kw)
    assert L.QLambda.last is ref and ref.lam == LAM
    ref.reset()
    ref.env.ep_len[:] = ref.env.ep_step + np.array([1, 2, 50], np.uint32)      # terminals at t = 0 and t = 1
    acts = np.array([[0, 1, 2], [3, 0, 1], [2, 3, 0]], np.int32)
    Pp = {k: v.copy() for k, v in ref.params.items()}
    out = ref.iterate(acts)
    assert out['terminals'][0, 0] and out['terminals'][1, 1] and not out['terminals'][:, 2].any()
    nxt = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
    ref.tau += n
    ref.iterate(acts, grads=False)            # the overlap check replays rollout k before the late targets of k-1
    rc = L.QLambdaRc(n, E, A, LAM, sarsa=form == 'sarsa')
    qn = R.forward(ref.tparams, nxt, 'q', keep=False)['z'].astype(np.float32)
    flat = (out['rewards'].reshape(-1), out['terminals'].reshape(-1))
    if form == 'double':
        qo = R.forward(Pp, nxt, 'q', keep=False)['z'][:, :A].astype(np.float32)
        late = rc.td_target_double(*flat, qn, qo, DISCOUNT)
    else:
        late = rc.td_target(*flat, qn, DISCOUNT)
    assert np.array_equal(late.reshape(n, E), out['target'])
    assert rc.clip_by_norm is R.clip_by_norm                       # everything else is oracle.ref_cpu
    assert np.abs(out['target'] - out['one_step_target']).max() > 1e-6
    loss, _ = R.q_loss_and_dz(out['z_batch'], acts.reshape(-1), out['target'].reshape(-1).astype(np.float64))
    assert loss == out['losses']['loss']


# ------------------------------------------------------------------ 3. the parity cases
def test_parity_table_holds_the_cases_the_engine_is_checked_at():
    keys = {(c['check'], c['E']) for c in PARITY.values()}
    assert keys == {('sync', 8), ('overlap', 16)}
    assert {c['form'] for c in PARITY.values() if c['check'] == 'sync' and c['n'] == 5} == set(L.FORMS)
    assert {c['form'] for c in PARITY.values() if c['check'] == 'overlap' and c['n'] == 5} == set(L.FORMS)
    assert sorted({c['n'] for c in PARITY.values()}) == [1, 5]
    assert all(c['lam'] == 0.7 and c['lives'] == 5 for c in PARITY.values())


@pytest.mark.parametrize('name', list(PARITY))
def test_parity_case_covers_the_terminal_positions(name):
    """Every engine-parity case, from the env alone: among its back-propagated rollouts there are terminals in
    the first cell, in a middle cell (n = 1 has none) and in the last cell, and a rollout in which some env has
    none."""
    case = PARITY[name]
    K, n, E = backprop(case), case['n'], case['E']
    sim = simulate(case)
    cells = sim['terms'][:K]
    assert covers(cells, n, E), cells.tolist()


@pytest.mark.parametrize('name', list(PARITY))
def test_parity_seed_has_no_near_tie(name):
    """The case replayed by the oracle alone, in the order its check replays it (L.oracle_alone): every draw of
    every rollout -- and, Sarsa, every back-propagated rollout's draw at s_n -- is well apart from both of its
    boundaries: |u - eps| and, on the greedy branch, the gap between the two largest Q values exceed
    TIE_MARGIN, ten times the allowance of assert_draws_explained.  Over the case both branches occur, the
    oracle's own terminals cover the cells, and the lambda targets differ from the one-step and from the n-step
    targets of the same rows by more than 1e-3 somewhere (n = 1: they are the one-step targets)."""
    case = PARITY[name]
    A, E, n = case['A'], case['E'], case['n']
    outs, ref = L.oracle_alone(case, EPS)
    K = backprop(case)
    assert len(outs) == case['rollouts'] and ref.lam == case['lam']
    random = greedy = 0

    def margins(u, eps, z, tag):
        nonlocal random, greedy
        assert (np.abs(u - eps) > TIE_MARGIN).all(), (name, tag)
        g = u >= eps
        top2 = np.sort(z[:, :A], axis=1)[:, -2:]
        gap = (top2[:, 1] - top2[:, 0]) / np.maximum(1.0, np.abs(z[:, :A]).max(axis=1))
        assert (gap[g] > TIE_MARGIN).all(), (name, tag, gap[g].min())
        random += int((~g).sum())
        greedy += int(g.sum())

    differ0 = differ1 = 0.0
    for k, out in enumerate(outs):
        for t in range(n):
            margins(out['u'][t], out['eps'][t], out['z'][t], (k, t))
        if k >= K:
            continue
        form = {}
        if case['form'] == 'sarsa':
            b = ref.boot_hist[k]
            margins(b['u'][0], b['eps'][0], b['z'][0], (k, 'boot'))
            form = dict(actions=out['actions'], boot_actions=b['sampled'][0])
        tgt = out['late'] if case['check'] == 'overlap' else out['target']
        rows = (out['late_rows'] if case['check'] == 'overlap' else out['q_target_rows'])[:, :A].astype(np.float32)
        if case['form'] == 'double':
            continue                    # (its q_sel rows are the check's own; the two other forms show the rule)
        for lam, key in ((0.0, 0), (1.0, 1)):
            end = L.lambda_q_target_ref(out['rewards'], out['terminals'], rows, A, DISCOUNT, lam, **form)
            gap = float(np.abs(tgt - end).max())
            if key == 0:
                differ0 = max(differ0, gap)
            else:
                differ1 = max(differ1, gap)
    cells = np.array([o['terminals'].astype(np.int64).sum(axis=1) for o in outs[:K]])
    print(name, 'draws: random', random, 'greedy', greedy, 'max |lambda - one-step|', differ0, 'max |lambda - n-step|',
          differ1, 'terminal cells', cells.tolist())
    assert random >= 1 and greedy >= 1
    assert covers(cells, n, E), cells.tolist()
    if case['form'] != 'double':
        if n == 1:
            assert differ0 == 0.0 and differ1 == 0.0
        else:
            assert differ0 > 1e-3 and differ1 > 1e-3


# ------------------------------------------------------------------ 4. the command line
BASE = ['--mode', 'engine', '--algo', 'q', '--n_step', '5', '--env_name', 'Catch-v0']


def test_q_lambda_flag_reaches_the_engine_options():
    import main
    assert main.engine_options(main.parse_flags(BASE + ['--q_lambda', '0.8'])) == dict(lstm=False, q_lambda=0.8)
    assert main.engine_options(main.parse_flags(BASE + ['--q_lambda', '0.8', '--sarsa', 'true'])) == dict(
        lstm=False, sarsa=1, q_lambda=0.8)
    assert main.engine_options(main.parse_flags(BASE + ['--q_lambda', '0.8', '--double_q', 'true'])) == dict(
        lstm=False, double_q=True, q_lambda=0.8)
    for value in ('0', '1', '0.0', '1.0'):             # the ends are lambdas like any other: 0 is not "unset"
        kw = main.engine_options(main.parse_flags(BASE + ['--q_lambda', value]))
        assert kw == dict(lstm=False, q_lambda=float(value)) and isinstance(kw['q_lambda'], float)
    for argv in (BASE, ['--algo', 'q'], []):
        flags = main.parse_flags(argv)
        assert flags.q_lambda is None and 'q_lambda' not in main.engine_options(flags)
    # the dicts the existing tests expect are what they were
    assert main.engine_options(main.parse_flags([])) == dict(lstm=False)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'true'])) == dict(lstm=False, q_nstep=1)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--sarsa', 'true'])) == dict(lstm=False, sarsa=1)


def test_q_lambda_flag_rejections():
    import main
    with pytest.raises(ValueError, match='--q_lambda is a Q-learning option'):
        main.engine_options(main.parse_flags(['--q_lambda', '0.8']))
    with pytest.raises(ValueError, match='--q_lambda is a Q-learning option'):
        main.engine_options(main.parse_flags(['--algo', 'a3c', '--q_lambda', '0']))
    with pytest.raises(ValueError, match='--q_lambda with --q_nstep'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'true', '--q_lambda', '0.8']))
    for bad in ('-0.1', '1.5', 'nan'):
        with pytest.raises(ValueError, match=r'--q_lambda must be in \[0, 1\]'):
            main.engine_options(main.parse_flags(['--algo', 'q', '--q_lambda', bad]))
    with pytest.raises(ValueError, match='--q_lambda is an engine option'):
        main.main(['--mode', 'agent', '--algo', 'q', '--q_lambda', '0.8'])
    # the existing rejections keep their text
    with pytest.raises(ValueError, match='algo q has one-step TD targets'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--gae_lambda', '0.9']))
    with pytest.raises(ValueError, match='--q_nstep is a Q-learning option'):
        main.engine_options(main.parse_flags(['--q_nstep', 'true']))
    with pytest.raises(ValueError, match='--sarsa with --double_q'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--sarsa', 'true', '--double_q', 'true']))


def test_engine_keyword_is_checked_before_the_device():
    """Engine._check_q_lambda, the rule Engine(q_lambda=...) and Engine.set_q_lambda share."""
    from src.engine import Engine
    chk = Engine._check_q_lambda
    assert chk(None, 'a3c', 1) is None and chk(0, 'q', 0) == 0.0 and chk(1, 'q', 0) == 1.0 and chk(0.7, 'q', 0) == 0.7
    for args, word in (((0.5, 'a3c', 0), 'Q-learning option'), ((0.5, 'q', 1), 'q_lambda with q_nstep'),
                       ((-0.1, 'q', 0), 'must be in'), ((1.01, 'q', 0), 'must be in'),
                       ((float('nan'), 'q', 0), 'must be in')):
        with pytest.raises(ValueError, match=word):
            chk(*args)


# ------------------------------------------------------------------ 5. the C structs and symbols
C_PROBE = r'''
#include <stdio.h>
#include "a3c_hip.h"
int main(void) {
  int (*op)(const float*, const uint8_t*, const int32_t*, const int32_t*, const float*, const float*, int, int64_t,
            int, int, double, double, float*, void*) = a3c_lambda_q_target;
  int (*set)(a3c_engine*, int, double) = a3c_engine_set_q_lambda;
  printf("%zu %zu %d\n", sizeof(a3c_engine_config), sizeof(a3c_engine_opts), op != 0 && set != 0);
  return 0;
}
'''
NEW_SYMBOLS = ('a3c_lambda_q_target', 'a3c_engine_set_q_lambda')


def test_header_declares_the_symbols_and_the_structs_did_not_grow(tmp_path):
    """The header as gcc reads it: both prototypes with the signatures the ctypes table has, and
    a3c_engine_config / a3c_engine_opts as large as they were (184 and 12 bytes)."""
    from src import _lib
    src = tmp_path / 'probe.c'
    src.write_text(C_PROBE)
    obj = tmp_path / 'probe.o'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), '-c', str(src), '-o', str(obj)],
                   check=True)
    assert ctypes.sizeof(_lib.EngineConfig) == 184 and ctypes.sizeof(_lib.EngineOpts) == 12
    assert [f[0] for f in _lib.EngineOpts._fields_] == ['size', 'game', 'sarsa']
    assert not hasattr(_lib.EngineConfig, 'q_lambda') and not hasattr(_lib.EngineOpts, 'q_lambda')
    header = open(HEADER).read()
    assert 'typedef struct a3c_engine_opts { int size; int game; int sarsa; } a3c_engine_opts;' in header
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['a3c_lambda_q_target'][1]) == 14
    assert _lib.SIGNATURES['a3c_engine_set_q_lambda'][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    assert 'lambda = 0' in header and 'lambda = 1' in header and 'to the last bit' in header


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    import torch  # noqa: F401  (share torch's HIP runtime, as the package does)
    return ctypes.CDLL(SO)


def test_library_exports_the_symbols_and_rejects_before_the_device(lib):
    """The argument checks of both entry points run before anything touches the device: they answer
    A3C_ERR_INVALID on a machine without one."""
    from src import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    lib.a3c_last_error.restype = ctypes.c_char_p
    res, args = _lib.SIGNATURES['a3c_lambda_q_target']
    lib.a3c_lambda_q_target.restype, lib.a3c_lambda_q_target.argtypes = res, args
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def call(r=one, t=one, a=null, b=null, q=one, qs=null, n=2, E=5, A=3, zs=4, lam=0.5, out=one):
        return lib.a3c_lambda_q_target(r, t, a, b, q, qs, n, E, A, zs, DISCOUNT, lam, out, null)
    for kw in (dict(r=null), dict(t=null), dict(q=null), dict(out=null), dict(a=one), dict(b=one),
               dict(a=one, b=one, qs=one), dict(lam=-0.1), dict(lam=1.1), dict(lam=float('nan')), dict(n=0), dict(E=0),
               dict(A=0), dict(A=5, zs=4)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert b'a3c_lambda_q_target' in lib.a3c_last_error(), kw
    res, args = _lib.SIGNATURES['a3c_engine_set_q_lambda']
    lib.a3c_engine_set_q_lambda.restype, lib.a3c_engine_set_q_lambda.argtypes = res, args
    for on, lam, word in ((2, 0.5, b'on must be 0 or 1'), (-1, 0.5, b'on must be 0 or 1'), (1, 1.5, b'lambda must be'),
                          (1, float('nan'), b'lambda must be'), (1, 0.5, b'null')):
        assert lib.a3c_engine_set_q_lambda(null, on, lam) == _lib.ERR_INVALID
        assert word in lib.a3c_last_error(), (on, lam)
