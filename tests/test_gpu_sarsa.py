"""Asynchronous one-step and n-step Sarsa (Engine(algo='q', sarsa=1)) on the GPU: the two
stand-alone kernels bit for bit against tests/_sarsa_ref.py; the engine's draw at the bootstrap state against
the next rollout's own first draw; the engine in every mode against the oracle under the Sarsa rule (the
existing _engine_parity checks and their bars, with the oracle swapped for _sarsa_ref's and the engine's a_n
held to the oracle's draw); graph against eager, resume, sarsa = 0, the rejections, learning on Catch.

What each data set and each parity case covers, and that no parity seed has a near-tie at s_n, is proved
without a GPU in tests/test_sarsa_cpu.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
import _qn_ref as Q  # noqa: E402
import _sarsa_ref as S  # noqa: E402
from test_episode_ends_cpu import backprop  # noqa: E402
from test_sarsa_cpu import EPS, PARITY  # noqa: E402

DISCOUNT = 0.99


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. a3c_sarsa_target
@pytest.mark.parametrize('E', S.OP_E)
@pytest.mark.parametrize('n', S.OP_N)
def test_target_op_equals_the_restatement_bit_for_bit(n, E):
    """a3c_sarsa_target against sarsa_target_ref, array_equal: the same float64 operations in the same order
    with contraction off.  Every (A, zs), both forms, clipped and standard-normal rewards, in-range actions
    and a few out-of-range words (-1, A, 2^31 - 1: they complete and read the column the restatement's
    reduction names, inside the row -- everything outside the live columns is NaN, so a read outside them
    shows).  n = 1: the two forms are torch.equal."""
    from src.kernels import sarsa_target
    for A, zs in S.OP_AZS:
        for normal in (False, True):
            for bad in (False, True):
                for d in S.op_cases(n, E, A, zs, normal_rewards=normal, bad_words=bad):
                    r, t, a, b = dev(d['rewards']), dev(d['terms']), dev(d['actions']), dev(d['boot'])
                    got = {}
                    for nstep in (0, 1):
                        rows = S.rows_of(d, nstep, n, E)
                        got[nstep] = sarsa_target(r, t, a, b, dev(rows), A, DISCOUNT, nstep=bool(nstep))
                        g = got[nstep].cpu().numpy()
                        want = S.sarsa_target_ref(d['rewards'], d['terms'], d['actions'], d['boot'], rows, A, DISCOUNT,
                                                  nstep)
                        assert g.shape == (n, E) and np.isfinite(g).all(), (A, zs, normal, bad, nstep)
                        miss = np.argwhere(g != want)
                        assert miss.size == 0, (A, zs, normal, bad, nstep, len(miss), miss[:4].tolist(),
                                                [(float(g[i, e]), float(want[i, e])) for i, e in miss[:4]])
                    if n == 1:
                        assert torch.equal(got[0], got[1]), (A, zs, normal, bad)


@pytest.mark.parametrize('n,E', [(1, 300), (5, 37), (64, 300), (2, 1)])
def test_target_op_with_argmax_actions_is_the_max_target(n, E):
    """a' = the first argmax of the same target rows: torch.equal to a3c_td_target (one-step) and to
    a3c_nstep_q_target (n-step)."""
    from src.kernels import nstep_q_target, sarsa_target, td_target
    for A, zs in S.OP_AZS:
        for d in S.op_cases(n, E, A, zs) + S.op_cases(n, E, A, zs, normal_rewards=True):
            acts, boot = S.argmax_actions(d['q'], n, E, A)
            r, t, a, b, q = dev(d['rewards']), dev(d['terms']), dev(acts), dev(boot), dev(d['q'])
            one = sarsa_target(r, t, a, b, q, A, DISCOUNT)
            assert torch.equal(one.reshape(-1), td_target(r.reshape(-1), t.reshape(-1), q, A, DISCOUNT)), (A, zs)
            rows = dev(S.rows_of(d, 1, n, E))
            assert torch.equal(sarsa_target(r, t, a, b, rows, A, DISCOUNT, nstep=True),
                               nstep_q_target(r, t, rows, A, DISCOUNT)), (A, zs)


def test_target_op_rejects_invalid_arguments():
    from src import _lib
    lib = _lib.lib()
    d = S.op_cases(2, 5, 3, 4)[0]
    r, t, a, b, q = dev(d['rewards']), dev(d['terms']), dev(d['actions']), dev(d['boot']), dev(d['q'])
    out = torch.empty((2, 5), device='cuda')
    p, s, null = _lib.ptr, _lib.stream_handle(), ctypes.c_void_p(0)

    def call(r_=p(r), t_=p(t), a_=p(a), b_=p(b), q_=p(q), out_=p(out), nstep=0, n=2, E=5, A=3, zs=4):
        return lib.a3c_sarsa_target(r_, t_, a_, b_, q_, nstep, n, E, A, zs, DISCOUNT, out_, s)
    assert call() == 0 and call(nstep=1) == 0
    for kw in (dict(r_=null), dict(t_=null), dict(a_=null), dict(b_=null), dict(q_=null), dict(out_=null),
               dict(nstep=2), dict(nstep=-1), dict(n=0), dict(E=0), dict(A=0), dict(A=5, zs=4)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert b'a3c_sarsa_target' in lib.a3c_last_error(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. a3c_boot_action
@pytest.mark.parametrize('E', S.OP_E)
def test_boot_action_op_equals_the_numpy_draw(E):
    """a3c_boot_action against oracle.philox + the first argmax, array_equal: every (A, zs), eps rows of 0, of 1
    and mixed, taus on both sides of 2^32, a non-zero env_id_base, a seed with both key words set.  Both
    branches occur on every data set (asserted); the tie set must give the first maximum."""
    from src.kernels import boot_action
    for A, zs in S.OP_AZS:
        sets = [S.boot_cases(E, A, zs)] + ([S.boot_cases(E, A, zs, ties=True)] if A >= 2 else [])
        for ties, (q, mixed) in enumerate(sets):
            took = set()
            for eps in (np.zeros(E, np.float32), np.ones(E, np.float32), mixed):
                for tau in S.BOOT_TAUS:
                    got = boot_action(dev(q), dev(eps), A, tau, env_id_base=3, seed=S.BOOT_SEED).cpu().numpy()
                    want, random = S.boot_action_ref(q, eps, A, tau, env_id_base=3, seed=S.BOOT_SEED)
                    assert got.dtype == np.int32 and np.array_equal(got, want), (A, zs, ties, tau, got[:8], want[:8])
                    took |= set(random.tolist())
            assert took == {False, True}, (A, zs, ties)
            if ties:
                got = boot_action(dev(q), dev(np.zeros(E, np.float32)), A, 5, seed=S.BOOT_SEED).cpu().numpy()
                assert np.array_equal(got, np.argmax(q[:, :A], axis=1))


def test_boot_action_op_rejects_invalid_arguments():
    from src import _lib
    lib = _lib.lib()
    q, eps = (dev(v) for v in S.boot_cases(5, 3, 4))
    out = torch.empty((5,), dtype=torch.int32, device='cuda')
    p, s, null = _lib.ptr, _lib.stream_handle(), ctypes.c_void_p(0)

    def call(q_=p(q), eps_=p(eps), out_=p(out), E=5, A=3, zs=4):
        return lib.a3c_boot_action(q_, eps_, E, A, zs, 7, 0, 123, out_, s)
    assert call() == 0
    for kw in (dict(q_=null), dict(eps_=null), dict(out_=null), dict(E=0), dict(A=0), dict(A=5, zs=4)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert b'a3c_boot_action' in lib.a3c_last_error(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the draw is the rollout's draw
ITERS = 6
ANNEAL = dict(ep_end_t=12, learn_start=0)       # epsilon from 1 to the env's ep_end over 12 env steps


def boots_and_firsts(eng, overlap):
    """Run ITERS iterations; returns (a_n of rollout k, actions[0] of rollout k+1) for every k that has both."""
    boots, firsts = {}, {}
    for k in range(ITERS):
        eng.iterate()
        torch.cuda.synchronize()
        if overlap:               # iterate k: rollout k into slot k & 1, the gradient of rollout k-1 beside it
            firsts[k] = eng.slot(k & 1)['actions'][0].cpu().numpy().copy()
            if k >= 1:
                boots[k - 1] = eng.slot((k - 1) & 1)['boot_actions'].cpu().numpy().copy()
        else:
            firsts[k] = eng.slot(0)['actions'][0].cpu().numpy().copy()
            boots[k] = eng.slot(0)['boot_actions'].cpu().numpy().copy()
    pairs = [(k, boots[k], firsts[k + 1]) for k in sorted(boots) if k + 1 in firsts]
    assert len(pairs) == ITERS - 1
    return pairs


@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)], ids=['sync', 'overlap'])
def test_boot_action_is_the_next_rollouts_first_action(E, overlap, n):
    """learning_rate = 0: the parameters never change, so a_n of rollout k is actions[0] of rollout k+1,
    array_equal -- the same key, step, epsilon and Q row, by another kernel.  The default learning rate: the
    same on every env on the random branch (u < eps at that step), which reads no Q; both branches occur."""
    A = 6
    kw = dict(overlap=overlap, sarsa=1, target_q_update_step=40, **ANNEAL)
    eng, ref, _ = EP.build('q', A, E, n, 0, seed=3601 + E + n, learning_rate=0.0, **kw)
    for k, boot, first in boots_and_firsts(eng, overlap):
        assert ((boot >= 0) & (boot < A)).all() and np.array_equal(boot, first), (k, boot, first)
    eng, ref, _ = EP.build('q', A, E, n, 0, seed=3601 + E + n, **kw)
    p0 = eng.params.clone()
    random = greedy = 0
    for k, boot, first in boots_and_firsts(eng, overlap):
        ref.tau = 3 + k * n                                   # rollout k starts there; its step n is s_n's draw
        u, eps = ref.draw_words(n)[0], ref.eps(n)
        m = u < eps
        assert np.array_equal(boot[m], first[m]), (k, boot, first, m)
        random += int(m.sum())
        greedy += int((~m).sum())
    assert random >= 1 and greedy >= 1, (random, greedy)
    assert not torch.equal(eng.params, p0)                     # (the parameters did change under these draws)


# ------------------------------------------------------------------ 4. engine parity
def assert_coverage(name, ref):
    """What test_sarsa_cpu.py proved for the case, from the counts the check collected."""
    case = PARITY[name]
    n, E, counts = case['n'], case['E'], ref.episode_counts
    cells = np.asarray(counts['terminal_cells'])
    assert counts['backprop'] == backprop(case) == len(cells) and counts['rollouts'] == case['rollouts'], counts
    assert cells[:, 0].sum() >= 1 and cells[:, n - 1].sum() >= 1 and cells[:, 1:n - 1].sum() >= 1, cells.tolist()
    assert (cells.sum(axis=1) < E).any(), cells.tolist()


class BootCheck:
    """A check's on_update hook: after the update of a rollout, the engine's a_n of that rollout against the
    oracle's own draw (its fp64 forward of s_n with the rollout's parameters, draw_words(n), eps(n)) by
    assert_draws_explained's q rule -- zero unexplained mismatches, the near-tie allowance the only exclusion
    (test_sarsa_cpu.py: the oracle alone has no near-tie at these seeds)."""

    def __init__(self, case):
        self.case, self.seen, self.mismatches, self.random, self.greedy = case, 0, 0, 0, 0

    def __call__(self, it, eng, ref, lr):
        overlap = self.case['check'] == 'overlap'
        k = it - 1 if overlap else it                     # the rollout just back-propagated
        b = ref.boot_hist[k]
        got = eng.slot(k & 1 if overlap else 0)['boot_actions'].cpu().numpy()
        assert ((got >= 0) & (got < self.case['A'])).all()
        self.mismatches += EP.assert_draws_explained(got[None], b, 'q', self.case['A'], ('boot', k))
        m = b['u'][0] < b['eps'][0]
        assert np.array_equal(got[m], b['sampled'][0][m])                 # the random branch is exact
        self.random += int(m.sum())
        self.greedy += int((~m).sum())
        self.seen += 1


def run_parity(name, monkeypatch, host_kw=None):
    case = PARITY[name]
    A, E, n, lives, seed, rollouts = case['A'], case['E'], case['n'], case['lives'], case['seed'], case['rollouts']
    kw = dict(case.get('opts', {}), sarsa=1, q_nstep=case['q_nstep'], **EPS)
    if case.get('lr') is not None:
        kw['learning_rate'] = case['lr']
    oracle = S.oracle_class(case)
    if case.get('catch'):
        from test_gpu_catch import stagger
        kw.update(game='catch', frames=C.FRAMES, start=stagger)
    elif host_kw is None:
        kw['start'] = EP.scheduled(backprop(case))
    kw.update(host_kw or {})
    monkeypatch.setattr(EP, 'EngineRef', oracle)
    boots = BootCheck(case)
    if case['check'] == 'overlap':
        # the check forms the late targets itself, through Rc.td_target: by the Sarsa rule, with the
        # rollout's actions and a_n from the oracle (S.Sarsa.last.boot_hist)
        monkeypatch.setattr(EP, 'Rc', S.SarsaRc(n, E, A, case['q_nstep']))
        eng, ref = EP.check_overlap_vs_oracle(A, E, n, lives, rollouts=rollouts, seed=seed, algo='q', on_update=boots,
                                              **kw)
    else:
        eng, ref = EP.check_sync_vs_oracle('q', A, E, n, lives, iters=rollouts, seed=seed, on_update=boots, **kw)
    assert type(ref) is oracle and ref is S.Sarsa.last and ref.q_nstep == case['q_nstep']
    assert eng.sarsa and eng.cfg.q_nstep == case['q_nstep'] and eng.cfg.double_q == 0
    assert eng.cfg.target_q_update_step == 40           # a target sync falls inside the run
    assert boots.seen == backprop(case) and boots.random >= 1 and boots.greedy >= 1, vars(boots)
    print(name, 'a_n: random', boots.random, 'greedy', boots.greedy, 'explained near-ties', boots.mismatches)
    assert boots.mismatches == 0                        # (no near-tie at these seeds: nothing to explain)
    assert_coverage(name, ref)
    return eng, ref


@pytest.mark.parametrize('name', [k for k, c in PARITY.items() if not c.get('host')])
def test_engine_matches_oracle(name, monkeypatch):
    """Targets rtol = atol = 1e-5, losses 1e-4, same-activation gradients 1e-4, independent gradients 2e-2,
    parameters and target parameters, zero unexplained draws, a_n against the oracle's own draw; rewards,
    terminals, ring and env state exact -- check_sync_vs_oracle / check_overlap_vs_oracle as they stand."""
    eng, _ = run_parity(name, monkeypatch)
    if PARITY[name].get('catch'):
        assert eng.game == 'catch' and eng.cfg.action_repeat == 2


def test_engine_with_host_envs_matches_oracle(monkeypatch):
    """external_env: the rollout's rewards and terminals arrive through ext_observe."""
    from src.host_env import HostEnvPool
    from test_gpu_host_env import HostSynthEnv
    case = PARITY['host']
    A, E, lives, P = case['A'], case['E'], case['lives'], case['frames']
    made = []

    def pool(seed):
        made.append(HostEnvPool([HostSynthEnv(seed, e, P, A, lives) for e in range(E)], threads=2))
        return made[0]
    start = EP.scheduled(backprop(case), host_envs=lambda: [h.env for h in made[0].envs])
    eng, _ = run_parity('host', monkeypatch, host_kw=dict(frames=P, host_pool=pool, start=start))
    assert eng.external_env


def test_sarsa_is_not_q_learning(monkeypatch):
    """On a parity case's first rollout the engine's targets are the Sarsa oracle's (1e-5, the checks' bar) and
    differ from the max oracle's by more than 1e-3 somewhere, in both forms."""
    from oracle.engine_ref import EngineRef
    for name, mx in (('sync', EngineRef), ('sync-nstep', Q.NStepQEngineRef)):
        case = PARITY[name]
        monkeypatch.setattr(EP, 'EngineRef', S.oracle_class(case))
        kw = dict(target_q_update_step=40, **EPS)
        eng, ref, _ = EP.build('q', case['A'], case['E'], case['n'], case['lives'], seed=case['seed'], sarsa=1,
                               q_nstep=case['q_nstep'], **kw)
        one = mx(ref.params, case['E'], case['n'], case['A'], 'q', case['lives'], 48, case['seed'], **kw)
        one.reset()
        eng.rollout_grad()
        torch.cuda.synchronize()
        acts = eng.actions.cpu().numpy()
        tgt = eng.returns.cpu().numpy()
        np.testing.assert_allclose(tgt, ref.iterate(acts, grads=False)['target'], rtol=1e-5, atol=1e-5)
        assert np.abs(tgt - one.iterate(acts, grads=False)['target']).max() > 1e-3, name


# ------------------------------------------------------------------ 5. graph equals eager, resume
STATE = ('params', 'target_params', 'ms', 'grads', 'loss')
RUN = dict(sarsa=1, target_q_update_step=40, learning_rate=3e-3, **EPS)


@pytest.mark.parametrize('q_nstep', [0, 1])
def test_graph_equals_eager(q_nstep):
    engs = [EP.build('q', 6, 16, 5, 0, seed=3701, overlap=True, use_graph=g, q_nstep=q_nstep, **RUN)[0]
            for g in (True, False)]
    assert engs[0].cfg.use_graph == 1 and engs[1].cfg.use_graph == 0
    for _ in range(4):
        for eng in engs:
            eng.iterate()
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(engs[0], name), getattr(engs[1], name)), name
    for k in range(2):
        assert torch.equal(engs[0].slot(k)['returns'], engs[1].slot(k)['returns']), k
        assert torch.equal(engs[0].slot(k)['boot_actions'], engs[1].slot(k)['boot_actions']), k
    assert float(engs[0].loss[0]) > 0


@pytest.mark.parametrize('E,overlap', [(8, False), (8, True)], ids=['sync', 'overlap'])
def test_resume_is_bit_for_bit(E, overlap):
    """3 iterations + save_state + load_state into a fresh engine + 3 iterations = 6 uninterrupted (boot_actions
    is no part of the state: every gradient writes it before it reads it)."""
    def make():
        return EP.build('q', 6, E, 3, 5, seed=3801, overlap=overlap, q_nstep=int(overlap), **RUN)[0]
    a, b = make(), make()
    for _ in range(6):
        a.iterate()
    for _ in range(3):
        b.iterate()
    torch.cuda.synchronize()
    blob = b.save_state()
    c = make()
    c.load_state(blob)
    for _ in range(3):
        c.iterate()
    torch.cuda.synchronize()
    for name in STATE + ('mom', 'counters', 'frame_ring'):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    for k in range(2 if overlap else 1):
        assert torch.equal(a.slot(k)['returns'], c.slot(k)['returns']), k
        assert torch.equal(a.slot(k)['boot_actions'], c.slot(k)['boot_actions']), k


# ------------------------------------------------------------------ 6. sarsa = 0, rejections
@pytest.mark.parametrize('q_nstep', [0, 1])
@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)], ids=['sync', 'overlap'])
def test_sarsa_off_changes_nothing(E, overlap, q_nstep):
    """Engine(algo='q', sarsa=0), built through a3c_engine_create_opts, against Engine(algo='q'), built as
    before: three iterations leave the same parameters, RMSProp slots, gradient, loss and targets."""
    kw = dict(overlap=overlap, target_q_update_step=40, learning_rate=3e-3, **EPS)
    if q_nstep:
        kw['q_nstep'] = 1
    a, _, _ = EP.build('q', 6, E, 5, 5, seed=3901 + E, sarsa=0, **kw)
    b, _, _ = EP.build('q', 6, E, 5, 5, seed=3901 + E, **kw)
    assert not a.sarsa and not b.sarsa and 'boot_actions' not in a.slot(0)
    for _ in range(3):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for k in range(2 if overlap else 1):
        assert torch.equal(a.slot(k)['returns'], b.slot(k)['returns']), k
    assert float(a.loss[0]) > 0


def test_rejections():
    from src import _lib
    from src.engine import Engine
    for kw, word in ((dict(algo='a3c', sarsa=1), 'sarsa is a Q-learning option'), (dict(algo='q', sarsa=2), 'sarsa must be'),
                     (dict(algo='q', sarsa=-1), 'sarsa must be'), (dict(algo='q', sarsa=1, double_q=1), 'sarsa with double_q')):
        with pytest.raises(_lib.A3CError, match=word) as ei:
            Engine(num_envs=4, n_step=2, num_frames=8, **kw)
        assert ei.value.rc == _lib.ERR_INVALID, kw
    with pytest.raises(ValueError, match='unknown engine option'):
        Engine(num_envs=4, n_step=2, num_frames=8, algo='q', sarsa=1, salsa=1)
    plain = Engine(num_envs=4, n_step=2, num_frames=8, algo='q')
    with pytest.raises(KeyError):
        plain.slot(0)['boot_actions']
    p = ctypes.c_void_p()
    assert _lib.lib().a3c_engine_slot_boot_actions(plain._h, 0, ctypes.byref(p)) == _lib.ERR_INVALID
    plain.close()
    eng = Engine(num_envs=4, n_step=2, num_frames=8, algo='q', sarsa=1, q_nstep=1)
    assert tuple(eng.slot(0)['boot_actions'].shape) == (4,) and eng.slot(0)['boot_actions'].dtype == torch.int32
    assert _lib.lib().a3c_engine_slot_boot_actions(eng._h, 1, ctypes.byref(p)) == _lib.ERR_INVALID     # sync: one slot
    eng.close()
    Engine(num_envs=4, n_step=2, num_frames=8, algo='q', sarsa=0).close()


# ------------------------------------------------------------------ 7. learning
LEARN = dict(learn_start=0, ep_end_t=1000, target_q_update_step=12800, learning_rate=2e-2)      # §4h's settings
LEARN_K = {1: 4096, 0: 8192}                  # q_nstep -> iterations


@pytest.mark.parametrize('q_nstep', [1, 0], ids=['nstep', 'one-step'])
def test_sarsa_learns_catch(q_nstep):
    """The overlapped Q engine with sarsa = 1 (256 envs, n = 5, the reference initialisers; LEARN: §4h's
    settings -- epsilon annealed over 1000 env steps per env, a target sync every 10 iterations, learning rate
    2e-2, RMSProp as the reference has it) trained LEARN_K iterations on seed 1, then 1024 greedy episodes.  The
    bar is §4g's, halfway from the random policy's exact return to the optimal one, R_rand + 0.5 (1 - R_rand)
    = 0.125: the untrained parameters play below it, the trained ones at or above it.

    LEARN_K: mean greedy play return against iterations, measured on one MI355X for seeds 1 / 2 / 3
    (tools/sarsa_learning.py; the two Q-learning columns rerun in the same session):
      sarsa, q_nstep = 1   0: -0.836 / -0.840 / -0.852,  512: -0.807 / -0.793 / -0.727,  1024: 0.525 / -0.002 / 0.014,
                           2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0,  8192: 1.0 / 1.0 / 1.0
      sarsa, one-step      1024: -0.725 / -0.732 / -0.244,  2048: -0.508 / -0.139 / -0.123,  4096: 1.0 / 1.0 / 1.0,
                           8192: 1.0 / 1.0 / 1.0
      Q, q_nstep = 1       1024: -0.586 / -0.065 / -0.113,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Q, one-step          2048: -0.410 / -0.420 / -0.326,  4096: 1.0 / 0.561 / 1.0,  8192: 1.0 / 1.0 / 1.0
    The smallest power of two at which all three seeds clear the bar is 2048 (n-step) and 4096 (one-step);
    LEARN_K is twice that (1.3 s and 2.9 s of training)."""
    import main
    from src.engine import Engine
    seed, A = 1, 3
    kw = dict(q_nstep=1) if q_nstep else {}
    eng = Engine(num_envs=256, n_step=5, action_size=A, algo='q', overlap=True, seed=seed, num_frames=C.FRAMES,
                 game='catch', sarsa=1, **kw, **LEARN)
    eng.reset(main.initial_params(eng, A, 'q', seed))
    eng.target_params.copy_(eng.params)
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    play = dict(n_episode=1024, n_step=50, refill=True, test_ep=0.0)
    before = eng.play(**play)
    for _ in range(LEARN_K[q_nstep]):
        eng.iterate()
    after = eng.play(**play)
    for out in (before, after):
        assert (out['lengths'] == C.ROWS - 1).all() and out['terminated'].all()
    r0, r1 = float(before['returns'].mean()), float(after['returns'].mean())
    print('catch, sarsa, q_nstep', q_nstep, ': mean greedy return untrained', r0, 'after', LEARN_K[q_nstep],
          'iterations', r1, 'bar', C.LEARNING_BAR)
    assert C.LEARNING_BAR == 0.125
    assert r0 < C.LEARNING_BAR, (r0, C.LEARNING_BAR)
    assert r1 >= C.LEARNING_BAR, (r1, C.LEARNING_BAR)
