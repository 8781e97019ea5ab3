"""GAE(lambda) in the A3C engine, the parts that need no GPU: the numpy reference the GPU tests
compare against (gae_ref, checked here at its two closed forms), the command line (--gae_lambda
reaches the Engine or is rejected) and the C header.

The recursion (include/a3c_hip.h K7b, DESIGN "GAE(lambda)"), for i = n-1 .. 0 with V_n = boot:
    nt = 1 - terminal_i;  delta_i = r_i + gamma nt V_{i+1} - V_i;
    A_i = delta_i + gamma lambda nt A_{i+1}  (A_n = 0);  G_i = A_i + V_i."""
import os
import re

import numpy as np
import pytest

from oracle import ref_cpu as Rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')


def gae_ref(rewards, terms, values, boot, gamma, lam):
    """fp64 GAE over [n][E]: returns (G, A), the lambda-returns and the advantages."""
    r = np.asarray(rewards, np.float64)
    v = np.asarray(values, np.float64)
    nt = 1.0 - (np.asarray(terms) != 0).astype(np.float64)
    n = r.shape[0]
    vn = np.asarray(boot, np.float64).copy()
    a = np.zeros(r.shape[1], np.float64)
    G = np.zeros(r.shape, np.float64)
    A = np.zeros(r.shape, np.float64)
    for i in range(n - 1, -1, -1):
        delta = r[i] + gamma * nt[i] * vn - v[i]
        a = delta + gamma * lam * nt[i] * a
        A[i] = a
        G[i] = a + v[i]
        vn = v[i]
    return G, A


def rollout_data(n, E, seed):
    """Random [n][E] rewards / values / bootstrap with terminals at interior steps and at n-1."""
    rng = np.random.default_rng(seed)
    rewards = rng.standard_normal((n, E)).astype(np.float32)
    values = rng.standard_normal((n, E)).astype(np.float32)
    boot = rng.standard_normal(E).astype(np.float32)
    terms = (rng.random((n, E)) < 0.15).astype(np.uint8)
    terms[n - 1, ::3] = 1
    if n > 2:
        terms[n // 2, 1::3] = 1
    return rewards, terms, values, boot


@pytest.mark.parametrize('n,E', [(1, 5), (2, 7), (5, 37), (64, 11)])
def test_gae_ref_lambda_one_is_the_nstep_return(n, E):
    rewards, terms, values, boot = rollout_data(n, E, 10 * n + E)
    assert terms[n - 1].any() and (n < 3 or terms[1:n - 1].any())
    G, A = gae_ref(rewards, terms, values, boot, 0.99, 1.0)
    want = Rc.nstep_returns(rewards, terms, boot, 0.99)
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(A, want - values.astype(np.float64), rtol=0, atol=1e-12)


@pytest.mark.parametrize('n,E', [(1, 5), (2, 7), (5, 37), (64, 11)])
def test_gae_ref_lambda_zero_is_the_one_step_target(n, E):
    rewards, terms, values, boot = rollout_data(n, E, 20 * n + E)
    G, A = gae_ref(rewards, terms, values, boot, 0.99, 0.0)
    v_next = np.concatenate([values[1:], boot[None]]).astype(np.float64)
    want = rewards.astype(np.float64) + 0.99 * (1.0 - terms) * v_next
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-12)


def test_gae_ref_between_the_two():
    """lambda in (0, 1): the exponentially weighted sum of the k-step advantages, written out
    for one env without terminals."""
    rng = np.random.default_rng(3)
    n, g, lam = 4, 0.9, 0.7
    r, v, boot = rng.standard_normal((n, 1)), rng.standard_normal((n, 1)), rng.standard_normal(1)
    G, A = gae_ref(r, np.zeros((n, 1), np.uint8), v, boot, g, lam)
    vv = np.concatenate([v[:, 0], boot])
    delta = r[:, 0] + g * vv[1:] - vv[:-1]
    for t in range(n):
        want = sum((g * lam) ** k * delta[t + k] for k in range(n - t))
        assert abs(A[t, 0] - want) < 1e-12


# ------------------------------------------------------------------ command line
def _main():
    import main
    return main


def test_default_flags_give_todays_options():
    main = _main()
    f = main.parse_flags([])
    assert f.gae_lambda == 1.0
    assert main.engine_options(f) == dict(lstm=False)
    assert main.engine_options(main.parse_flags(['--lstm', 'true'])) == dict(lstm=True)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--double_q', 'true'])) == dict(lstm=False,
                                                                                                 double_q=True)
    assert main.engine_options(main.parse_flags(['--dqn_type', 'nature'])) == dict(lstm=False, dqn_type='nature')
    # 1 spelled out is still the default: nothing is added
    assert main.engine_options(main.parse_flags(['--gae_lambda', '1'])) == dict(lstm=False)
    assert main.engine_options(main.parse_flags(['--algo', 'q', '--gae_lambda', '1.0'])) == dict(lstm=False)


def test_gae_lambda_reaches_the_engine_options():
    main = _main()
    kw = main.engine_options(main.parse_flags(['--gae_lambda', '0.95']))
    assert kw == dict(lstm=False, gae_lambda=0.95)
    kw = main.engine_options(main.parse_flags(['--gae_lambda', '0', '--lstm', 'true']))
    assert kw == dict(lstm=True, gae_lambda=0.0)
    kw = main.engine_options(main.parse_flags(['--gae_lambda', '0.5', '--dqn_type', 'nature']))
    assert kw == dict(lstm=False, gae_lambda=0.5, dqn_type='nature')


@pytest.mark.parametrize('argv', [['--algo', 'q', '--gae_lambda', '0.9'], ['--gae_lambda', '1.5'],
                                  ['--gae_lambda', '-0.1'], ['--gae_lambda', 'nan']])
def test_gae_lambda_rejections(argv):
    main = _main()
    with pytest.raises(ValueError, match='gae_lambda'):
        main.engine_options(main.parse_flags(argv))


def test_mode_agent_rejects_gae_lambda():
    """--mode agent is the per-step Q-learning loop: rejected before any config or device work."""
    main = _main()
    with pytest.raises(ValueError, match='gae_lambda'):
        main.main(['--mode', 'agent', '--gae_lambda', '0.9'])


# ------------------------------------------------------------------ header and bindings
def test_header_declares_gae():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+a3c_gae_returns\s*\(', src)
    cfg = re.search(r'typedef struct a3c_engine_config \{(.*?)\} a3c_engine_config;', src, re.S).group(1)
    fields = re.findall(r'\b(\w+)\s*[;,]', cfg)
    assert fields[-1] == 'gae_lambda', fields[-3:]           # appended: earlier offsets are unchanged
    assert re.search(r'\bfloat\s+gae_lambda\s*;', cfg)


def test_ctypes_mirror_has_gae():
    from src import _lib
    assert _lib.EngineConfig._fields_[-1] == ('gae_lambda', _lib.c_float)
    res, args = _lib.SIGNATURES['a3c_gae_returns']
    assert res is _lib.c_int and len(args) == 12
    assert args[3] is _lib.c_i64 and args[7] is _lib.c_double and args[8] is _lib.c_double
