"""Asynchronous n-step Q-learning (q_nstep) without a GPU: the restatement the GPU
tests compare against (tests/_qn_ref.py) held to a brute-force definition and, at n = 1, to the
one-step oracle; the coverage of every data set and every engine-parity case of
tests/test_gpu_q_nstep.py, proved here so that no GPU case can pass without it; the command line
(--q_nstep); the C struct and its default.

PARITY is the one table of both files (as test_episode_ends_cpu.CASES is)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _catch_ref as C  # noqa: E402
import _qn_ref as Q  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_episode_ends_cpu import backprop, simulate  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')

# the engine-parity cases of test_gpu_q_nstep.py (check: the _engine_parity check that runs it; the
# overlap pipeline's last rollout has no backward).  Synthetic env: terminals by _engine_parity.schedule
# over the back-propagated rollouts; Catch: the balls staggered as tests/test_gpu_catch.py staggers them.
PARITY = {
    'sync': dict(check='sync', algo='q', A=6, E=8, n=3, rollouts=3, lives=5, seed=3101),
    'sync-double-18': dict(check='sync', algo='q', A=18, E=13, n=5, rollouts=3, lives=0, seed=3102,
                           opts=dict(double_q=1)),
    'overlap': dict(check='overlap', algo='q', A=6, E=16, n=5, rollouts=4, lives=0, seed=3103),
    'overlap-double': dict(check='overlap', algo='q', A=6, E=8, n=4, rollouts=4, lives=0, seed=3104,
                           opts=dict(double_q=1)),
    'host': dict(check='sync', algo='q', A=6, E=6, n=3, rollouts=3, lives=0, seed=3105, frames=40, host=True),
    'catch-sync': dict(check='sync', algo='q', A=3, E=6, n=3, rollouts=4, lives=0, seed=3106, catch=True,
                       opts=dict(action_repeat=2)),
    'catch-overlap': dict(check='overlap', algo='q', A=3, E=6, n=3, rollouts=5, lives=0, seed=3107, catch=True,
                          opts=dict(action_repeat=2)),
}


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize('n,E,A', [(1, 3, 2), (2, 5, 3), (5, 37, 6), (64, 9, 18)])
@pytest.mark.parametrize('double', [False, True])
def test_restatement_equals_the_definition(n, E, A, double):
    """The recursion against the explicit sum of discounted rewards up to the first terminal (plus
    discount^(n-i) B_e when there is none): 1e-12 relative -- the two round differently."""
    for normal in (False, True):
        for d in Q.op_cases(n, E, A, A + 2, normal_rewards=normal):
            qsel = d['q_sel'][:, :A] if double else None
            got = Q.nstep_q_target_ref(d['rewards'], d['terms'], d['q_boot'][:, :A], qsel, 0.99)
            want = Q.nstep_q_target_brute(d['rewards'], d['terms'], d['q_boot'][:, :A], qsel, 0.99)
            assert got.dtype == np.float32 and got.shape == (n, E)
            r64 = Q.nstep_q_target_ref(d['rewards'], d['terms'], d['q_boot'][:, :A], qsel, 0.99, out_dtype=np.float64)
            np.testing.assert_allclose(r64, want, rtol=1e-12, atol=1e-12)
            assert np.array_equal(r64.astype(np.float32), got)       # float32 is the last step only


@pytest.mark.parametrize('E,A', [(1, 1), (37, 6), (300, 18)])
def test_one_step_is_the_td_target(E, A):
    """n = 1: the restatement is oracle.ref_cpu.td_target / td_target_double to the last bit."""
    for normal in (False, True):
        for d in Q.op_cases(1, E, A, A + 2, normal_rewards=normal):
            r, t, qb, qs = d['rewards'], d['terms'], d['q_boot'][:, :A], d['q_sel'][:, :A]
            assert np.array_equal(Q.nstep_q_target_ref(r, t, qb, None, 0.99)[0],
                                  R.td_target(r[0], t[0], qb, 0.99).astype(np.float32))
            assert np.array_equal(Q.nstep_q_target_ref(r, t, qb, qs, 0.99)[0],
                                  R.td_target_double(r[0], t[0], qb, qs, 0.99).astype(np.float32))


@pytest.mark.parametrize('double_q', [False, True])
def test_oracle_subclass_and_late_target_adapter_agree(double_q):
    """The two ways the GPU checks take the oracle's n-step target -- NStepQ.iterate (synchronous
    checks) and NStepRc on the next states' rows (the overlap check's late targets) -- are one rule:
    equal while the target network has not moved, and not the one-step target.  With grads the
    subclass returns what EngineRef.iterate returns for algo q."""
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    from oracle.engine_ref import EngineRef
    A, E, n, seed = 4, 3, 3, 3001
    p = init_params(param_names_shapes(A, 'q'), seed=seed, stddev=0.08)
    ref = Q.NStepQEngineRef(p, E, n, A, 'q', 0, 16, seed, double_q=double_q)
    one = EngineRef(p, E, n, A, 'q', 0, 16, seed, double_q=double_q)
    for r in (ref, one):
        r.reset()
        r.env.ep_len[:] = r.env.ep_step + np.array([1, 2, 50], np.uint32)      # terminals at t = 0 and t = 1
    acts = np.zeros((n, E), np.int32)
    out = ref.iterate(acts)
    old = one.iterate(acts)
    assert out['terminals'].tolist() == old['terminals'].tolist() and out['terminals'][0, 0] and out['terminals'][1, 1]
    assert not out['terminals'][:, 2].any()
    assert set(old) | {'q_boot'} <= set(out) and set(out['grads']) == set(old['grads'])
    nxt = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
    rc = Q.NStepRc(n, E, A)
    qn = R.forward(ref.tparams, nxt, 'q', keep=False)['z'].astype(np.float32)
    if double_q:
        qo = R.forward(ref.params, nxt, 'q', keep=False)['z'][:, :A].astype(np.float32)
        late = rc.td_target_double(out['rewards'].reshape(-1), out['terminals'].reshape(-1), qn, qo, 0.99)
    else:
        late = rc.td_target(out['rewards'].reshape(-1), out['terminals'].reshape(-1), qn, 0.99)
    assert np.array_equal(late.reshape(n, E), out['target'])
    assert rc.clip_by_norm is R.clip_by_norm                       # everything else is oracle.ref_cpu
    # env 2 has no terminal: its first target is r0 + g r1 + g^2 r2 + g^3 B, not r0 + g max Q(s_1)
    assert abs(out['target'][0, 2] - old['target'][0, 2]) > 1e-6
    want = Q.nstep_q_target_ref(out['rewards'], out['terminals'], out['q_boot'][:, :A].astype(np.float32),
                                out['q_boot_online'][:, :A].astype(np.float32) if double_q else None, 0.99)
    assert np.array_equal(want, out['target'])
    loss, _ = R.q_loss_and_dz(out['z_batch'], acts.reshape(-1), out['target'].reshape(-1).astype(np.float64))
    assert loss == out['losses']['loss'] and out['losses']['loss'] != old['losses']['loss']


# ------------------------------------------------------------------ 2. coverage
@pytest.mark.parametrize('E', Q.OP_E)
@pytest.mark.parametrize('n', [n for n in Q.OP_N if n >= 5])
def test_op_data_covers_the_terminal_patterns(n, E):
    """Every (n >= 5, E) of the GPU test, over the data sets it runs there: a terminal at i = 0, at
    an interior step, at i = n-1 (the bootstrap cut), two in a row, and an env without any (the
    bootstrap at full depth); double Q changes the targets."""
    for A, zs in Q.OP_AZS:
        for normal in (False, True):
            sets = Q.op_cases(n, E, A, zs, normal_rewards=normal)
            terms = [d['terms'] for d in sets]
            assert any(t[0].any() for t in terms)
            assert any(t[1:n - 1].any() for t in terms)
            assert any(t[n - 1].any() for t in terms)
            assert any((t[:-1] & t[1:]).any() for t in terms)
            assert any((t.sum(axis=0) == 0).any() for t in terms)
            changed = False
            for d in sets:
                assert np.isnan(d['q_boot'][:, A:]).all() and np.isnan(d['q_sel'][:, A:]).all()
                assert np.isfinite(d['q_boot'][:, :A]).all() and np.isfinite(d['q_sel'][:, :A]).all()
                if normal:
                    assert not set(np.unique(d['rewards'])) <= {-2.0, -1.0, 0.0, 1.0}
                else:
                    assert set(np.unique(d['rewards'])) <= {-2.0, -1.0, 0.0, 1.0}
                differ = np.argmax(d['q_sel'][:, :A], axis=1) != np.argmax(d['q_boot'][:, :A], axis=1)
                plain = Q.nstep_q_target_ref(d['rewards'], d['terms'], d['q_boot'][:, :A], None, 0.99)
                double = Q.nstep_q_target_ref(d['rewards'], d['terms'], d['q_boot'][:, :A], d['q_sel'][:, :A], 0.99)
                if A > 1 and (d['terms'].sum(axis=0) == 0).any():
                    assert differ.any()
                    assert not np.array_equal(plain, double)
                    changed = True
                if A == 1:
                    assert np.array_equal(plain, double)
            assert changed == (A > 1)


def catch_terminals(case):
    """Terminals [rollouts, n, E] of a Catch case from CatchEnv alone: landings depend on no action."""
    E, n, r = case['E'], case['n'], case['opts']['action_repeat']
    env = C.CatchEnv(case['seed'], E, action_repeat=r)
    env.new_random_game()
    c, _, p = C.decode(env.frame)
    rows = (np.arange(E) * r) % (C.ROWS - 1)                 # tests/test_gpu_catch.py stagger()
    env.frame[:] = C.encode(c, rows, p).astype(np.uint32)
    env.ep_step[:] = rows
    out = np.zeros((case['rollouts'], n, E), np.int64)
    for k in range(case['rollouts']):
        for t in range(n):
            _, _, term = env.act(np.zeros(E, np.int32))
            out[k, t] = term
            if term.any():
                env.new_random_game(term)
    return out


@pytest.mark.parametrize('name', list(PARITY))
def test_parity_case_covers_the_terminal_positions(name):
    """Every engine-parity case, from the env alone: among its back-propagated rollouts there are
    terminals at t = 0, at an interior t and at t = n-1, and a rollout in which some env has none
    (fewer terminals in the rollout than envs)."""
    case = PARITY[name]
    K, n, E = backprop(case), case['n'], case['E']
    if case.get('catch'):
        cells = catch_terminals(case)[:K].sum(axis=2)
    else:
        cells = simulate(case)['terms'][:K]
    print(name, 'terminals per (rollout, t):', cells.tolist())
    assert cells[:, 0].sum() >= 1 and cells[:, n - 1].sum() >= 1 and cells[:, 1:n - 1].sum() >= 1, cells.tolist()
    assert (cells.sum(axis=1) < E).any(), cells.tolist()


# ------------------------------------------------------------------ 3. the command line
def test_q_nstep_flag_reaches_the_engine_options():
    import main
    kw = main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'true']))
    assert kw == dict(lstm=False, q_nstep=1)
    kw = main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'true', '--double_q', 'true']))
    assert kw == dict(lstm=False, q_nstep=1, double_q=True)
    assert 'q_nstep' not in main.engine_options(main.parse_flags(['--algo', 'q']))
    assert 'q_nstep' not in main.engine_options(main.parse_flags(['--algo', 'q', '--q_nstep', 'false']))
    assert 'q_nstep' not in main.engine_options(main.parse_flags([]))
    f = main.parse_flags(['--mode', 'engine', '--algo', 'q', '--q_nstep', 'true', '--n_step', '5', '--env_name',
                          'Catch-v0'])
    assert main.engine_options(f) == dict(lstm=False, q_nstep=1)


def test_q_nstep_flag_rejections():
    import main
    with pytest.raises(ValueError, match='q_nstep'):
        main.engine_options(main.parse_flags(['--q_nstep', 'true']))
    with pytest.raises(ValueError, match='q_nstep'):
        main.main(['--mode', 'agent', '--q_nstep', 'true'])
    # the gae_lambda rejections keep their text
    with pytest.raises(ValueError, match='algo q has one-step TD targets'):
        main.engine_options(main.parse_flags(['--algo', 'q', '--gae_lambda', '0.9']))


# ------------------------------------------------------------------ 4. the C struct
C_PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "a3c_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(a3c_engine_config), offsetof(a3c_engine_config, q_nstep),
         offsetof(a3c_engine_config, ep_end), offsetof(a3c_engine_config, ep_end_t),
         offsetof(a3c_engine_config, gae_lambda));
  return 0;
}
'''


def test_config_struct_matches_gcc(tmp_path):
    """sizeof and the new field's place as gcc lays the header out; q_nstep sits in the 4 bytes that
    aligned ep_end_t, so the struct is as large as it was (184 bytes) and gae_lambda is still last."""
    from src import _lib
    src = tmp_path / 'probe.c'
    src.write_text(C_PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    size, off, ep_end, ep_end_t, lam = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                       check=True).stdout.split())
    cfg = _lib.EngineConfig
    assert size == ctypes.sizeof(cfg) == 184
    assert off == cfg.q_nstep.offset == ep_end + 4 == ep_end_t - 4
    assert ep_end == cfg.ep_end.offset and ep_end_t == cfg.ep_end_t.offset and lam == cfg.gae_lambda.offset == 180
    assert cfg._fields_[-1][0] == 'gae_lambda'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    import torch  # noqa: F401  (share torch's HIP runtime, as the package does)
    return ctypes.CDLL(SO)


def test_default_config_is_one_step(lib):
    from src import _lib
    cfg = _lib.EngineConfig()
    cfg.q_nstep = 7
    lib.a3c_engine_config_default.restype = None
    lib.a3c_engine_config_default.argtypes = [ctypes.POINTER(_lib.EngineConfig)]
    lib.a3c_engine_config_default(ctypes.byref(cfg))
    assert cfg.q_nstep == 0 and cfg.double_q == 0 and cfg.gae_lambda == 1.0
    assert hasattr(lib, 'a3c_nstep_q_target') and 'a3c_nstep_q_target' in _lib.SIGNATURES
