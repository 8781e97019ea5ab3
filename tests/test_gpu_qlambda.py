"""lambda-return targets of the Q engine (Engine(algo='q', q_lambda=...)) on the GPU: the stand-alone
kernel bit for bit against tests/_qlambda_ref.py and, at lambda = 0 and lambda = 1, against the existing device
ops; the engine in sync and overlap mode against the oracle under the lambda rule (the existing _engine_parity
checks and their bars, with the oracle swapped for _qlambda_ref's); the engine's own endpoints; graph against
eager, resume, q_lambda = None, the rejections, the setter between iterations, learning on Catch.

What each parity case covers, and that no parity seed has a near-tie, is proved without a GPU in
tests/test_qlambda_cpu.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
import _qlambda_ref as L  # noqa: E402
from test_episode_ends_cpu import backprop  # noqa: E402
from test_gpu_sarsa import BootCheck  # noqa: E402
from test_qlambda_cpu import EPS, LAM, PARITY, SHAPES, covers  # noqa: E402

DISCOUNT = 0.99


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def dev_form(d, form):
    return {k: dev(v) for k, v in L.form_args(d, form).items()}


# ------------------------------------------------------------------ 1. a3c_lambda_q_target
@pytest.mark.parametrize('n,E', SHAPES)
def test_target_op_equals_the_restatement_bit_for_bit(n, E):
    """a3c_lambda_q_target against lambda_q_target_ref, array_equal: the same float64 operations in the same
    order with contraction off.  Every (A, zs) -- (1, 1) and (18, 20)... rows the kernel reads column by column
    or 16 bytes at a time, (31, 32) a last load that is part padding -- the three forms, lambda in (0, 0.3, 0.95,
    1) and 0.7, clipped rewards with in-range actions and standard-normal rewards with out-of-range words (-1,
    A, 2^31 - 1, -2^31: they read the column the restatement's reduction names).  Everything outside the live
    columns is 1e30, so a maximum, an argmax or a gather that reads past A shows."""
    from src.kernels import lambda_q_target
    for A, zs in L.OP_AZS:
        for normal, bad in ((False, False), (True, True)):
            for d in L.op_cases(n, E, A, zs, normal_rewards=normal, bad_words=bad):
                r, t, q = dev(d['rewards']), dev(d['terms']), dev(d['q'])
                for form in L.FORMS:
                    kw = dev_form(d, form)
                    for lam in L.OP_LAMBDAS + (LAM,):
                        g = lambda_q_target(r, t, q, A, lam, DISCOUNT, **kw).cpu().numpy()
                        want = L.lambda_q_target_ref(d['rewards'], d['terms'], d['q'], A, DISCOUNT, lam,
                                                     **L.form_args(d, form))
                        assert g.shape == (n, E) and np.isfinite(g).all() and np.abs(g).max() < 1e6, (A, zs, form, lam)
                        miss = np.argwhere(g != want)
                        assert miss.size == 0, (A, zs, normal, form, lam, len(miss), miss[:4].tolist(),
                                                [(float(g[i, e]), float(want[i, e])) for i, e in miss[:4]])


def test_target_op_reads_unaligned_rows_column_by_column():
    """Rows whose base is not 16-byte aligned (a view one float into a buffer) with zs % 4 == 0: the same result
    as the aligned copy."""
    from src.kernels import lambda_q_target
    n, E, A, zs = 5, 37, 6, 8
    d, = L.op_cases(n, E, A, zs)
    r, t = dev(d['rewards']), dev(d['terms'])
    for form in ('q', 'double'):
        kw = dev_form(d, form)
        want = lambda_q_target(r, t, dev(d['q']), A, LAM, DISCOUNT, **kw)
        buf = torch.zeros(n * E * zs + 1, device='cuda')
        buf[1:] = dev(d['q']).reshape(-1)
        q = buf[1:].view(n * E, zs)
        assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        if form == 'double':
            sbuf = torch.zeros(n * E * zs + 1, device='cuda')
            sbuf[1:] = kw['q_sel'].reshape(-1)
            kw = dict(q_sel=sbuf[1:].view(n * E, zs))
        assert torch.equal(lambda_q_target(r, t, q, A, LAM, DISCOUNT, **kw), want), form


@pytest.mark.parametrize('n,E', [(1, 300), (5, 37), (64, 300), (2, 1)])
def test_target_op_endpoints_are_the_existing_ops(n, E):
    """lambda = 0 is a3c_td_target (double: fed the value at q_sel's argmax as its one column, as the agent does)
    and a3c_sarsa_target(nstep = 0); lambda = 1 is a3c_nstep_q_target and a3c_sarsa_target(nstep = 1) on the
    rows of s_n: torch.equal."""
    from src.kernels import lambda_q_target, nstep_q_target, sarsa_target, td_target
    for A, zs in L.OP_AZS:
        for normal in (False, True):
            for d in L.op_cases(n, E, A, zs, normal_rewards=normal):
                r, t, q, qs = dev(d['rewards']), dev(d['terms']), dev(d['q']), dev(d['q_sel'])
                a, b = dev(d['actions']), dev(d['boot'])
                last, last_sel = q[(n - 1) * E:].contiguous(), qs[(n - 1) * E:].contiguous()
                tag = (A, zs, normal)
                assert torch.equal(lambda_q_target(r, t, q, A, 0.0, DISCOUNT).reshape(-1),
                                   td_target(r.reshape(-1), t.reshape(-1), q, A, DISCOUNT)), tag
                assert torch.equal(lambda_q_target(r, t, q, A, 1.0, DISCOUNT), nstep_q_target(r, t, last, A, DISCOUNT)), tag
                picked = q[torch.arange(n * E, device='cuda'), qs[:, :A].argmax(dim=1)].reshape(-1, 1).contiguous()
                assert torch.equal(lambda_q_target(r, t, q, A, 0.0, DISCOUNT, q_sel=qs).reshape(-1),
                                   td_target(r.reshape(-1), t.reshape(-1), picked, 1, DISCOUNT)), tag
                assert torch.equal(lambda_q_target(r, t, q, A, 1.0, DISCOUNT, q_sel=qs),
                                   nstep_q_target(r, t, last, A, DISCOUNT, q_sel=last_sel)), tag
                assert torch.equal(lambda_q_target(r, t, q, A, 0.0, DISCOUNT, actions=a, boot_actions=b),
                                   sarsa_target(r, t, a, b, q, A, DISCOUNT)), tag
                assert torch.equal(lambda_q_target(r, t, q, A, 1.0, DISCOUNT, actions=a, boot_actions=b),
                                   sarsa_target(r, t, a, b, last, A, DISCOUNT, nstep=True)), tag


def test_target_op_rejects_invalid_arguments():
    from src import _lib
    lib = _lib.lib()
    d = L.op_cases(2, 5, 3, 4)[0]
    r, t, a, b = dev(d['rewards']), dev(d['terms']), dev(d['actions']), dev(d['boot'])
    q, qs = dev(d['q']), dev(d['q_sel'])
    out = torch.empty((2, 5), device='cuda')
    p, s, null = _lib.ptr, _lib.stream_handle(), ctypes.c_void_p(0)

    def call(r_=p(r), t_=p(t), a_=null, b_=null, q_=p(q), qs_=null, out_=p(out), n=2, E=5, A=3, zs=4, lam=0.5):
        return lib.a3c_lambda_q_target(r_, t_, a_, b_, q_, qs_, n, E, A, zs, DISCOUNT, lam, out_, s)
    assert call() == 0 and call(qs_=p(qs)) == 0 and call(a_=p(a), b_=p(b)) == 0 and call(lam=0.0) == 0 and call(lam=1.0) == 0
    for kw in (dict(r_=null), dict(t_=null), dict(q_=null), dict(out_=null), dict(a_=p(a)), dict(b_=p(b)),
               dict(a_=p(a), b_=p(b), qs_=p(qs)), dict(lam=-1e-9), dict(lam=1.0 + 1e-9), dict(lam=float('nan')),
               dict(n=0), dict(E=0), dict(A=0), dict(A=5, zs=4)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert b'a3c_lambda_q_target' in lib.a3c_last_error(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. engine parity
def run_parity(name, monkeypatch):
    case = PARITY[name]
    A, E, n, lives, seed, rollouts = case['A'], case['E'], case['n'], case['lives'], case['seed'], case['rollouts']
    sarsa = case['form'] == 'sarsa'
    kw = dict(L.case_options(case), q_lambda=case['lam'], start=EP.scheduled(backprop(case)), **EPS)
    oracle = L.case_oracle(case)
    monkeypatch.setattr(EP, 'EngineRef', oracle)
    boots = BootCheck(case) if sarsa else None
    if case['check'] == 'overlap':
        # the check forms the late targets itself, through Rc.td_target / Rc.td_target_double: by the lambda rule
        monkeypatch.setattr(EP, 'Rc', L.QLambdaRc(n, E, A, case['lam'], sarsa=sarsa))
        eng, ref = EP.check_overlap_vs_oracle(A, E, n, lives, rollouts=rollouts, seed=seed, algo='q', on_update=boots,
                                              **kw)
    else:
        eng, ref = EP.check_sync_vs_oracle('q', A, E, n, lives, iters=rollouts, seed=seed, on_update=boots, **kw)
    assert type(ref) is oracle and ref is L.QLambda.last and ref.lam == case['lam'] == eng.q_lambda
    assert eng.sarsa == sarsa and eng.cfg.double_q == int(case['form'] == 'double') and eng.cfg.q_nstep == 0
    assert eng.cfg.target_q_update_step == 40           # a target sync falls inside the run
    assert ref.global_step >= 40
    if sarsa:
        assert boots.seen == backprop(case) and boots.random >= 1 and boots.greedy >= 1, vars(boots)
        print(name, 'a_n: random', boots.random, 'greedy', boots.greedy, 'explained near-ties', boots.mismatches)
        assert boots.mismatches == 0                    # (no near-tie at these seeds: nothing to explain)
    counts = ref.episode_counts
    cells = np.asarray(counts['terminal_cells'])
    assert counts['backprop'] == backprop(case) == len(cells) and counts['rollouts'] == rollouts, counts
    assert covers(cells, n, E), cells.tolist()
    return eng, ref


@pytest.mark.parametrize('name', list(PARITY))
def test_engine_matches_oracle(name, monkeypatch):
    """Targets rtol = atol = 1e-5, losses 1e-4, same-activation gradients 1e-4, independent gradients 2e-2,
    parameters and target parameters, zero unexplained draws, Sarsa: a_n against the oracle's own draw; rewards,
    terminals, ring and env state exact -- check_sync_vs_oracle / check_overlap_vs_oracle as they stand."""
    run_parity(name, monkeypatch)


# ------------------------------------------------------------------ 3. the engine's endpoints
STATE = ('params', 'target_params', 'ms', 'grads', 'loss')
FORM_KW = dict(q={}, double=dict(double_q=1), sarsa=dict(sarsa=1))
RUN = dict(target_q_update_step=40, learning_rate=3e-3, **EPS)


def assert_same_run(a, b, slots):
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for k in range(slots):
        assert torch.equal(a.slot(k)['returns'], b.slot(k)['returns']), k
        if a.sarsa:
            assert torch.equal(a.slot(k)['boot_actions'], b.slot(k)['boot_actions']), k
    assert float(a.loss[0]) > 0


@pytest.mark.parametrize('form', L.FORMS)
@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)], ids=['sync', 'overlap'])
def test_lambda_zero_is_the_one_step_engine_bit_for_bit(E, overlap, form):
    """q_lambda = 0.0 against the engine without it: six iterations (a target sync among them, terminals inside
    the rollouts) leave the same parameters, target parameters, RMSProp slots, gradient, loss and targets."""
    kw = dict(overlap=overlap, **FORM_KW[form], **RUN)
    a, ra, _ = EP.build('q', 6, E, 5, 5, seed=4201 + E, q_lambda=0.0, **kw)
    b, rb, _ = EP.build('q', 6, E, 5, 5, seed=4201 + E, **kw)
    assert a.q_lambda == 0.0 and b.q_lambda is None
    for eng, ref in ((a, ra), (b, rb)):
        EP.scheduled(5)(eng, ref)
    ended = 0
    for k in range(6):
        a.iterate()
        b.iterate()
        ended += int(a.slot(k & 1 if overlap else 0)['terminals'].sum())
    assert_same_run(a, b, 2 if overlap else 1)
    assert ended >= 1 and int(a.counters[1]) >= 40


@pytest.mark.parametrize('form', L.FORMS)
def test_lambda_one_is_the_nstep_engine_and_lambda_between_is_neither(form):
    """One rollout of four engines from the same seed and parameters -- q_lambda unset, 0.7, 1.0, and q_nstep =
    1 -- with terminals inside it: the same actions (and a_n); q_lambda = 1.0's targets are the n-step
    engine's at rtol = atol = 1e-5 (its rows of s_n come from a forward of another batch size, so bit
    identity is not claimed); q_lambda = 0.7's differ from the one-step engine's and from the n-step engine's
    by more than 1e-3 somewhere."""
    A, E, n = 6, 8, 5
    got = {}
    for key, kw in (('one', {}), ('mid', dict(q_lambda=LAM)), ('end', dict(q_lambda=1.0)), ('nstep', dict(q_nstep=1))):
        eng, ref, _ = EP.build('q', A, E, n, 5, seed=4301, **kw, **FORM_KW[form], **RUN)
        EP.scheduled(2)(eng, ref)           # env e ends e % 10 + 1 steps from now: envs 5 .. 7 behind the rollout
        eng.rollout_grad()
        torch.cuda.synchronize()
        got[key] = {k: eng.slot(0)[k].cpu().numpy().copy() for k in ('actions', 'returns', 'terminals', 'rewards') +
                    (('boot_actions',) if form == 'sarsa' else ())}
        eng.close()
    for key in ('mid', 'end', 'nstep'):
        for k in got['one']:
            if k != 'returns':
                assert np.array_equal(got[key][k], got['one'][k]), (key, k)
    ended = got['one']['terminals'].any(axis=0)
    assert ended.any() and not ended.all()
    np.testing.assert_allclose(got['end']['returns'], got['nstep']['returns'], rtol=1e-5, atol=1e-5)
    assert np.abs(got['mid']['returns'] - got['one']['returns']).max() > 1e-3
    assert np.abs(got['mid']['returns'] - got['nstep']['returns']).max() > 1e-3
    assert np.abs(got['one']['returns'] - got['nstep']['returns']).max() > 1e-3


# ------------------------------------------------------------------ 4. graph equals eager, resume, None
@pytest.mark.parametrize('form', L.FORMS)
def test_graph_equals_eager(form):
    engs = [EP.build('q', 6, 16, 5, 5, seed=4401, overlap=True, use_graph=g, q_lambda=LAM, **FORM_KW[form], **RUN)[0]
            for g in (True, False)]
    assert engs[0].cfg.use_graph == 1 and engs[1].cfg.use_graph == 0
    for _ in range(4):
        for eng in engs:
            eng.iterate()
    assert_same_run(engs[0], engs[1], 2)


@pytest.mark.parametrize('E,overlap,form', [(8, False, 'sarsa'), (8, True, 'q'), (8, True, 'double')],
                         ids=['sync-sarsa', 'overlap-q', 'overlap-double'])
def test_resume_is_bit_for_bit(E, overlap, form):
    """3 iterations + save_state + load_state into a fresh engine created with the same q_lambda + 3 iterations
    = 6 uninterrupted: q_lambda is no part of the state, the create gives it again."""
    def make():
        return EP.build('q', 6, E, 3, 5, seed=4501, overlap=overlap, q_lambda=LAM, **FORM_KW[form], **RUN)[0]
    a, b = make(), make()
    for _ in range(6):
        a.iterate()
    for _ in range(3):
        b.iterate()
    torch.cuda.synchronize()
    blob = b.save_state()
    plain = EP.build('q', 6, E, 3, 5, seed=4501, overlap=overlap, **FORM_KW[form], **RUN)[0]
    assert plain.save_state().size == blob.size            # (no byte of the state is the option's)
    c = make()
    c.load_state(blob)
    for _ in range(3):
        c.iterate()
    torch.cuda.synchronize()
    for name in STATE + ('mom', 'counters', 'frame_ring'):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    for k in range(2 if overlap else 1):
        assert torch.equal(a.slot(k)['returns'], c.slot(k)['returns']), k


@pytest.mark.parametrize('form', L.FORMS)
@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)], ids=['sync', 'overlap'])
def test_q_lambda_none_changes_nothing(E, overlap, form):
    """Engine(q_lambda=None) makes no call: three iterations equal the engine built without the keyword."""
    kw = dict(overlap=overlap, **FORM_KW[form], **RUN)
    a, _, _ = EP.build('q', 6, E, 5, 5, seed=4601 + E, q_lambda=None, **kw)
    b, _, _ = EP.build('q', 6, E, 5, 5, seed=4601 + E, **kw)
    assert a.q_lambda is None and b.q_lambda is None
    for _ in range(3):
        a.iterate()
        b.iterate()
    assert_same_run(a, b, 2 if overlap else 1)


# ------------------------------------------------------------------ 5. rejections, the setter
def test_rejections():
    from src import _lib
    from src.engine import Engine
    small = dict(num_envs=4, n_step=2, num_frames=8)
    for kw, word in ((dict(algo='a3c', q_lambda=0.5), 'q_lambda is a Q-learning option'),
                     (dict(algo='q', q_nstep=1, q_lambda=0.5), 'q_lambda with q_nstep'),
                     (dict(algo='q', q_lambda=-0.1), 'q_lambda must be in'), (dict(algo='q', q_lambda=1.1), 'q_lambda must be in'),
                     (dict(algo='q', q_lambda=float('nan')), 'q_lambda must be in')):
        with pytest.raises(ValueError, match=word):
            Engine(**small, **kw)
    setter = _lib.lib().a3c_engine_set_q_lambda
    last = _lib.lib().a3c_last_error
    a3c = Engine(**small, algo='a3c')
    assert setter(a3c._h, 1, 0.5) == _lib.ERR_INVALID and b'Q-learning option' in last()
    assert setter(a3c._h, 0, 0.0) == _lib.ERR_INVALID
    with pytest.raises(ValueError, match='Q-learning option'):
        a3c.set_q_lambda(0.5)
    a3c.close()
    nstep = Engine(**small, algo='q', q_nstep=1)
    assert setter(nstep._h, 1, 1.0) == _lib.ERR_INVALID and b'q_nstep' in last()
    with pytest.raises(ValueError, match='q_lambda with q_nstep'):
        nstep.set_q_lambda(1.0)
    nstep.close()
    eng = Engine(**small, algo='q', q_lambda=0.25)
    assert eng.q_lambda == 0.25
    for on, lam, word in ((2, 0.5, b'on must be 0 or 1'), (-1, 0.5, b'on must be 0 or 1'), (1, -0.5, b'lambda must be'),
                          (1, 1.5, b'lambda must be'), (1, float('nan'), b'lambda must be')):
        assert setter(eng._h, on, lam) == _lib.ERR_INVALID and word in last(), (on, lam)
    assert setter(None, 1, 0.5) == _lib.ERR_INVALID and b'null' in last()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='q_lambda must be in'):
            eng.set_q_lambda(bad)
    assert eng.q_lambda == 0.25
    eng.set_q_lambda(None)
    assert eng.q_lambda is None
    eng.set_q_lambda(1)
    assert eng.q_lambda == 1.0
    eng.close()


@pytest.mark.parametrize('form', ['q', 'sarsa'])
def test_setter_between_iterations_takes_effect_on_the_next_gradient(form):
    """Created with 0.3 and set to 0.7 before the first iteration: the engine created with 0.7, bit for bit.
    Then on two one-step engines in step: after set_q_lambda(0.7) on one, the next rollout draws the same
    actions and its targets differ; while that gradient is pending the setter answers A3C_ERR_STATE, after the
    apply it is taken."""
    from src import _lib
    kw = dict(**FORM_KW[form], **RUN)
    a, _, _ = EP.build('q', 6, 8, 5, 5, seed=4701, q_lambda=0.3, **kw)
    b, _, _ = EP.build('q', 6, 8, 5, 5, seed=4701, q_lambda=LAM, **kw)
    a.set_q_lambda(LAM)
    for _ in range(3):
        a.iterate()
        b.iterate()
    assert_same_run(a, b, 1)
    c, _, _ = EP.build('q', 6, 8, 5, 5, seed=4702, **kw)
    d, _, _ = EP.build('q', 6, 8, 5, 5, seed=4702, **kw)
    for _ in range(2):
        c.iterate()
        d.iterate()
    assert_same_run(c, d, 1)
    d.set_q_lambda(LAM)
    c.rollout_grad()
    d.rollout_grad()
    torch.cuda.synchronize()
    assert torch.equal(c.actions, d.actions) and torch.equal(c.rewards, d.rewards)
    assert float((c.returns - d.returns).abs().max()) > 1e-3
    with pytest.raises(_lib.A3CError) as ei:
        d.set_q_lambda(None)
    assert ei.value.rc == _lib.ERR_STATE and d.q_lambda == LAM
    c.apply()
    d.apply()
    torch.cuda.synchronize()
    d.set_q_lambda(None)
    assert d.q_lambda is None and not torch.equal(c.params, d.params)


# ------------------------------------------------------------------ 6. learning
LEARN = dict(learn_start=0, ep_end_t=1000, target_q_update_step=12800, learning_rate=2e-2)      # §4h's settings
LEARN_LAMBDA = 0.8
LEARN_K = 4096


@pytest.mark.parametrize('sarsa', [0, 1], ids=['q', 'sarsa'])
def test_qlambda_learns_catch(sarsa):
    """The overlapped Q engine with q_lambda = 0.8 (256 envs, n = 5, the reference initialisers; LEARN: §4h's
    settings -- epsilon annealed over 1000 env steps per env, a target sync every 10 iterations, learning rate
    2e-2, RMSProp as the reference has it) trained LEARN_K iterations on seed 1, then 1024 greedy episodes.  The
    bar is §4g's, halfway from the random policy's exact return to the optimal one, R_rand + 0.5 (1 - R_rand)
    = 0.125: the untrained parameters play below it, the trained ones at or above it.

    LEARN_K: mean greedy play return against iterations, measured on one MI355X for seeds 1 / 2 / 3
    (tools/q_lambda_learning.py; the one-step and n-step columns rerun in the same session; every run starts at
    -0.836 / -0.840 / -0.852):
      Q, one-step and lambda = 0     1024: -0.707 / -0.719 / -0.738,  2048: -0.412 / -0.506 / -0.295,
                                     4096: 1.0 / 0.541 / 1.0,  8192: 1.0 / 1.0 / 1.0
      Q, lambda = 0.5                1024: -0.355 / -0.521 / -0.156,  2048: 0.756 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Q, lambda = 0.8                1024: -0.723 / -0.182 / 0.033,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Q, lambda = 0.95               1024: 0.213 / -0.008 / 0.078,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Q, lambda = 1 and q_nstep      1024: -0.555 / -0.068 / -0.039,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Sarsa, one-step and lambda = 0 1024: -0.707 / -0.744 / -0.213,  2048: -0.510 / -0.221 / -0.109,
                                     4096: 1.0 / 1.0 / 1.0,  8192: 1.0 / 1.0 / 1.0
      Sarsa, lambda = 0.5            1024: -0.707 / -0.365 / -0.152,  2048: 0.371 / -0.769 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Sarsa, lambda = 0.8            1024: -0.082 / -0.094 / 0.152,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Sarsa, lambda = 0.95           1024: 0.176 / -0.018 / 0.393,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
      Sarsa, lambda = 1 and q_nstep  1024: 0.559 / -0.033 / 0.088,  2048: 1.0 / 1.0 / 1.0,  4096: 1.0 / 1.0 / 1.0
    (the lambda = 0 and lambda = 1 runs repeat the one-step and the n-step engine's to the digit).  At lambda =
    0.8 the smallest power of two at which all three seeds clear the bar is 2048, for Q and for Sarsa; LEARN_K is
    twice that (1.4 s of training)."""
    import main
    from src.engine import Engine
    seed, A = 1, 3
    kw = dict(sarsa=1) if sarsa else {}
    eng = Engine(num_envs=256, n_step=5, action_size=A, algo='q', overlap=True, seed=seed, num_frames=C.FRAMES,
                 game='catch', q_lambda=LEARN_LAMBDA, **kw, **LEARN)
    assert 0.0 < eng.q_lambda < 1.0
    eng.reset(main.initial_params(eng, A, 'q', seed))
    eng.target_params.copy_(eng.params)
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    play = dict(n_episode=1024, n_step=50, refill=True, test_ep=0.0)
    before = eng.play(**play)
    for _ in range(LEARN_K):
        eng.iterate()
    after = eng.play(**play)
    for out in (before, after):
        assert (out['lengths'] == C.ROWS - 1).all() and out['terminated'].all()
    r0, r1 = float(before['returns'].mean()), float(after['returns'].mean())
    print('catch, q_lambda', LEARN_LAMBDA, 'sarsa', sarsa, ': mean greedy return untrained', r0, 'after', LEARN_K,
          'iterations', r1, 'bar', C.LEARNING_BAR)
    assert C.LEARNING_BAR == 0.125
    assert r0 < C.LEARNING_BAR, (r0, C.LEARNING_BAR)
    assert r1 >= C.LEARNING_BAR, (r1, C.LEARNING_BAR)
