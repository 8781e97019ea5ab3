"""lambda-return targets of the Q engine (Engine(algo='q', q_lambda=...)): Peng's Q(lambda), its
double-Q form and Sarsa(lambda), numpy restatement.  Test infrastructure only (imported by
tests/test_qlambda_cpu.py and tests/test_gpu_qlambda.py).

The rule, as include/a3c_hip.h states it (everything in float64), with qt [n*E, >= A] the target network's rows
of s_1 .. s_n, b = i*E + e:

    B_i = max_a qt[b][a]                                   Q
          qt[b][first argmax_a q_sel[b][a]]                double Q: q_sel the same states' rows under the
                                                           rollout's own parameters
          qt[b][a'], a' = i < n-1 ? actions[i+1][e] : a_n[e]     Sarsa; an action word w is the column (uint32)w % A
    G = B_{n-1}
    for i = n-1 .. 0:   mix = (1 - lambda) * B_i + lambda * G;   if term[i][e]: mix = 0
                        G = r[i][e] + discount * mix;   target[i][e] = (float)G

lambda_q_target_ref is that rule in that operation order, lambda_q_target_brute the definition it restates;
QLambda turns an oracle.engine_ref.EngineRef (or a subclass on another env) into the lambda learner; QLambdaRc
lets _engine_parity.check_overlap_vs_oracle, which forms the overlap pipeline's late targets itself, form them
by the same rule."""
import numpy as np

import _qn_ref as Q
import _sarsa_ref as S
from oracle import ref_cpu as R
from oracle.engine_ref import EngineRef, acts_batch

FORMS = ('q', 'double', 'sarsa')


def bootstrap_values(q_target, A, n, E, q_sel=None, actions=None, boot_actions=None):
    """B [n, E] float32: the bootstrap value of s_{i+1} for every cell, by the form the arguments name."""
    qt = np.asarray(q_target)
    assert qt.shape[0] == n * E and qt.shape[1] >= A
    assert q_sel is None or actions is None
    assert (actions is None) == (boot_actions is None)
    rows = np.arange(n * E)
    if actions is not None:
        actions = np.asarray(actions)
        assert actions.shape == (n, E) and np.asarray(boot_actions).shape == (E,)
        nxt = np.concatenate([actions[1:], np.asarray(boot_actions)[None]])        # a' of step i
        b = qt[rows, S.column(nxt, A).reshape(-1)]
    elif q_sel is not None:
        qs = np.asarray(q_sel)
        assert qs.shape[0] == n * E
        b = qt[rows, np.argmax(qs[:, :A], axis=1)]                                # np.argmax: the first maximum
    else:
        b = qt[:, :A].max(axis=1)
    return b.reshape(n, E)


def lambda_q_target_ref(rewards, terms, q_target, A, discount, lam, q_sel=None, actions=None, boot_actions=None,
                        out_dtype=np.float32):
    """rewards, terms [n, E]; q_target [n*E, >= A] (columns >= A are never read); q_sel [n*E, >= A] or None;
    actions [n, E] and boot_actions [E], or both None.  Returns the targets [n, E] float32
    (out_dtype=np.float64: before that rounding)."""
    rewards, terms = np.asarray(rewards), np.asarray(terms)
    n, E = rewards.shape
    assert terms.shape == (n, E)
    B = bootstrap_values(q_target, A, n, E, q_sel, actions, boot_actions).astype(np.float64)
    lam, discount = np.float64(lam), np.float64(discount)
    keep = np.float64(1.0) - lam
    g = B[n - 1].copy()
    out = np.empty((n, E), out_dtype)
    for i in range(n - 1, -1, -1):
        mix = keep * B[i] + lam * g
        mix = np.where(terms[i] != 0, np.float64(0.0), mix)
        g = rewards[i].astype(np.float64) + discount * mix
        out[i] = g
    return out


def lambda_q_target_brute(rewards, terms, q_target, A, discount, lam, q_sel=None, actions=None, boot_actions=None):
    """The definition without the recursion.  For cell (i, e) with N = n - i steps left, the k-step return is
    G(k) = sum_{j<k} discount^j r[i+j] + discount^k B_{i+k-1}, without the bootstrap when a terminal lies in
    steps i .. i+k-1; a terminal at step i+T-1 makes every G(k >= T) that same return, so with M = min(T, N)
    target = (1 - lam) sum_{k=1}^{M-1} lam^(k-1) G(k) + lam^(M-1) G(M).  float64 [n, E]."""
    rewards, terms = np.asarray(rewards, np.float64), np.asarray(terms)
    n, E = rewards.shape
    B = bootstrap_values(q_target, A, n, E, q_sel, actions, boot_actions).astype(np.float64)
    out = np.zeros((n, E), np.float64)
    for i in range(n):                     # (the envs of a step together: the sums are explicit, per k)
        N = n - i
        total, acc, open_ = np.zeros(E), np.zeros(E), np.ones(E, bool)      # open_: k < M so far
        for k in range(1, N + 1):
            total = total + discount ** (k - 1) * rewards[i + k - 1]
            term = terms[i + k - 1] != 0
            Gk = np.where(term, total, total + discount ** k * B[i + k - 1])
            is_M = term | (k == N)
            weight = np.where(is_M, lam ** (k - 1), (1.0 - lam) * lam ** (k - 1))      # (0.0 ** 0 is 1)
            acc = acc + np.where(open_, weight * Gk, 0.0)
            open_ = open_ & ~is_M
        out[i] = acc
    return out


# ------------------------------------------------------------------ data of the stand-alone op
OP_E, OP_N = Q.OP_E, Q.OP_N
OP_AZS = Q.OP_AZS + ((31, 32),)          # (31, 32): a row of eight 16-byte loads whose last column is padding
OP_LAMBDAS = (0.0, 0.3, 0.95, 1.0)
PAD = np.float32(1e30)                    # outside the live columns: a read past A wins every maximum
BAD_WORDS = (-1, None, 2 ** 31 - 1, -2 ** 31)      # None: A itself


def op_cases(n, E, A, zs, normal_rewards=False, bad_words=False, pad=PAD):
    """The data sets the tests run at (n, E, A, zs): a list of dicts rewards, terms, actions [n, E], boot [E],
    q, q_sel [n*E, zs] (`pad` outside the A live columns).  Terminals by _qn_ref.op_terminals: E >= 5: one set,
    envs e % 5 == 4 without a terminal; smaller E: two sets, the second without any.  q_sel = -q on the live
    columns, so double Q picks the row's minimum; actions are uniform over [0, A); bad_words: a few cells of
    actions and boot hold -1, A, 2^31 - 1 and -2^31 instead."""
    sets = []
    frees = [set(range(4, E, 5))] if E >= 5 else [set(), set(range(E))]
    for v, free in enumerate(frees):
        rng = np.random.default_rng([n, E, A, zs, v, int(normal_rewards), 79])
        rewards = (rng.standard_normal((n, E)).astype(np.float32) if normal_rewards
                   else rng.choice(Q.CLIPPED, (n, E)))
        q = np.full((n * E, zs), pad, np.float32)
        q[:, :A] = rng.standard_normal((n * E, A)).astype(np.float32)
        q_sel = np.full((n * E, zs), pad, np.float32)
        q_sel[:, :A] = -q[:, :A]
        actions = rng.integers(0, A, (n, E)).astype(np.int32)
        boot = rng.integers(0, A, E).astype(np.int32)
        if bad_words:
            words = [A if w is None else w for w in BAD_WORDS]
            for j, w in enumerate(words):
                boot[(2 * j + v) % E] = w
                actions[(j + 1) % n, (3 * j + 1) % E] = w
        sets.append(dict(rewards=rewards, terms=Q.op_terminals(n, E, rng, free), actions=actions, boot=boot, q=q,
                         q_sel=q_sel))
    return sets


def form_args(d, form):
    """The keyword arguments that make lambda_q_target_ref (and src.kernels.lambda_q_target, given device
    tensors of the same names) take the form on a data set."""
    if form == 'double':
        return dict(q_sel=d['q_sel'])
    if form == 'sarsa':
        return dict(actions=d['actions'], boot_actions=d['boot'])
    assert form == 'q'
    return {}


# ------------------------------------------------------------------ the oracle
class QLambda:
    """Mixin in front of EngineRef (or a subclass of it): iterate() takes the parent's rollout and replaces its
    one-step target by the lambda-return of the rollout, from the target network's rows of s_1 .. s_n; double_q
    (the parent's option): at the argmax of self.params' rows of the same states; sarsa (class attribute): at
    the rollout's next actions, behind it a_n drawn as _sarsa_ref.Sarsa draws it (boot_hist, boot_forced: as
    there).  Then the parent's Q loss / backward / clip on it."""
    lam = 1.0
    sarsa = 0
    last = None                       # the newest instance (the parity checks build the oracle themselves)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.boot_hist = []
        self.boot_forced = None
        QLambda.last = self

    def iterate(self, forced_actions=None, grads=True):
        assert self.algo == 'q' and not self.lstm and not (self.sarsa and self.double_q)
        out = super().iterate(forced_actions, grads=False)
        n, E, A, h = self.n, self.E, self.A, self.h
        form = {}
        if self.sarsa:
            boot = S.Sarsa.draw_boot(self)
            boot['actions'] = out['actions']
            self.boot_hist.append(boot)
            out['boot'] = boot
            a_n = boot['sampled'][0] if self.boot_forced is None else np.asarray(self.boot_forced, np.int32)
            form = dict(actions=out['actions'], boot_actions=a_n)
        nxt = np.concatenate([self.states(self.tau + t) for t in range(1, n + 1)])
        qt = R.forward(self.tparams, nxt, 'q', dtype=self.dtype, keep=False)['z']
        if self.double_q:
            qo = R.forward(self.params, nxt, 'q', dtype=self.dtype, keep=False)['z']
            form = dict(q_sel=qo[:, :A].astype(np.float32))
        out['q_target_rows'] = qt
        out['one_step_target'] = out['target']
        target = lambda_q_target_ref(out['rewards'], out['terminals'], qt[:, :A].astype(np.float32), A, h['discount'],
                                     self.lam, **form)
        out['target'] = target
        if not grads:
            return out
        # the parent's lines for algo q (oracle/engine_ref.py iterate), on this target
        states = np.concatenate([self.states(self.tau + t) for t in range(n)])      # b = t*E + e
        B = n * E
        fwd = R.forward(self.params, states, 'q', self.dqn_type, dtype=self.dtype)
        out['acts_batch'] = acts_batch(fwd)
        flat_acts = out['actions'].reshape(-1)
        loss, dz = R.q_loss_and_dz(fwd['z'], flat_acts, target.reshape(-1).astype(self.dtype))
        losses = dict(loss=loss, q_mean=fwd['z'][np.arange(B), flat_acts].mean())
        if grads == 'losses':
            out.update(losses=losses, z_batch=fwd['z'])
            return out
        g = R.backward(self.params, fwd, dz, 'q', self.dqn_type)
        gr = {k: np.asarray(v, np.float32).reshape(self.params[k].shape) for k, v in g.items()}
        sumsq = {k: np.float32(np.sum(v.astype(np.float64) ** 2)) for k, v in gr.items()}
        clipped = {k: R.clip_by_norm(v, h['clip_norm']) for k, v in gr.items()}
        out.update(losses=losses, grads=gr, sumsq=sumsq, clipped=clipped, z_batch=fwd['z'])
        return out


def oracle_class(lam, sarsa=0, base=EngineRef):
    """The lambda learner on `base`'s env (double Q is the base's own option double_q)."""
    return type('QLambda' + ('Sarsa' if sarsa else '') + base.__name__, (QLambda, base),
                dict(lam=float(lam), sarsa=int(sarsa)))


class QLambdaRc:
    """oracle.ref_cpu with td_target / td_target_double replaced by the lambda rule, for
    _engine_parity.check_overlap_vs_oracle: that check forms the late targets of rollout k-1 itself, after the
    oracle replayed rollout k, from the oracle's forward of the rollout's next states s_1 .. s_n ([n*E, zs] rows,
    b = t*E + e) with the target network as it stands at gradient time (double_q: and with the rollout's own
    parameters).  Sarsa: the rollout's actions and its a_n -- drawn at rollout time with the rollout's
    parameters -- come from the oracle's boot_hist[-2] (QLambda.last: the newest oracle)."""

    def __init__(self, n, E, A, lam, sarsa=0):
        self.n, self.E, self.A, self.lam, self.sarsa = int(n), int(E), int(A), float(lam), int(sarsa)

    def __getattr__(self, name):
        return getattr(R, name)

    def _target(self, reward, terminal, q_next, discount, **form):
        n, E = self.n, self.E
        q = np.asarray(q_next)
        assert q.shape[0] == n * E and q.dtype == np.float32
        return lambda_q_target_ref(np.asarray(reward).reshape(n, E), np.asarray(terminal).reshape(n, E), q[:, :self.A],
                                   self.A, discount, self.lam, **form).reshape(-1)

    def td_target(self, reward, terminal, q_next, discount=0.99):
        form = {}
        if self.sarsa:
            ref = QLambda.last
            boot = ref.boot_hist[-2]
            a_n = boot['sampled'][0] if ref.boot_forced is None else np.asarray(ref.boot_forced, np.int32)
            form = dict(actions=boot['actions'], boot_actions=a_n)
        return self._target(reward, terminal, q_next, discount, **form)

    def td_target_double(self, reward, terminal, q_next_target, q_next_online, discount=0.99):
        assert not self.sarsa
        qo = np.asarray(q_next_online)
        assert qo.shape[0] == self.n * self.E and qo.dtype == np.float32
        return self._target(reward, terminal, q_next_target, discount, q_sel=qo[:, :self.A])


# ------------------------------------------------------------------ the parity cases, by the oracle alone
def case_oracle(case):
    return oracle_class(case['lam'], sarsa=case['form'] == 'sarsa')


def case_options(case):
    """The engine options a parity case runs with beside q_lambda (the oracle takes double_q under its name)."""
    kw = {}
    if case['form'] == 'double':
        kw['double_q'] = 1
    if case['form'] == 'sarsa':
        kw['sarsa'] = 1
    if case.get('lr') is not None:
        kw['learning_rate'] = case['lr']
    return kw


def oracle_alone(case, extra, scale=4.0):
    """A parity case of tests/test_qlambda_cpu.PARITY replayed by the oracle with its own draws, in the order the
    case's _engine_parity check replays it (sync: rollout, gradient, apply; overlap: rollout k with the
    parameters after update k-2, the late targets of rollout k-1 behind it, apply).  extra: the options every
    case runs with.  Returns (outs: every rollout's out, with out['late'] the late targets where the overlap
    order forms them; ref)."""
    import _engine_parity as EP
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    from test_episode_ends_cpu import backprop
    A, E, n, seed = case['A'], case['E'], case['n'], case['seed']
    kw = {k: v for k, v in dict(case_options(case), target_q_update_step=40, **extra).items() if k in EP.REF_KEYS}
    p = init_params(param_names_shapes(A, 'q'), seed=seed, stddev=0.02 * scale)
    ref = case_oracle(case)(p, E, n, A, 'q', case['lives'], case.get('frames', 48), seed, **kw)
    ref.reset()
    d = EP.schedule(E, n, backprop(case), ref.env.action_repeat)       # _engine_parity.scheduled(), the oracle's half
    ref.env.ep_len[:] = (ref.env.ep_step.astype(np.int64) + d).astype(np.uint32)
    outs = []
    if case['check'] == 'sync':
        for _ in range(case['rollouts']):
            out = ref.iterate()
            outs.append(out)
            ref.apply(out['clipped'])
        return outs, ref
    rc = QLambdaRc(n, E, A, case['lam'], sarsa=case['form'] == 'sarsa')
    hist = []
    for k in range(case['rollouts']):
        Pk = {kk: v.copy() for kk, v in ref.params.items()}
        out = ref.iterate(grads=False)
        planes = EP.rollout_planes(ref, n)
        out['next_states'] = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
        ref.tau += n
        hist.append((Pk, planes, out))
        outs.append(out)
        if k == 0:
            continue
        Pp, planes_p, out_p = hist[k - 1]
        qn = R.forward(ref.tparams, out_p['next_states'], 'q', keep=False)['z'].astype(np.float32)
        if case['form'] == 'double':
            qo = R.forward(Pp, out_p['next_states'], 'q', keep=False)['z']
            want = rc.td_target_double(out_p['rewards'].reshape(-1), out_p['terminals'].reshape(-1), qn,
                                       qo[:, :A].astype(np.float32), ref.h['discount'])
        else:
            want = rc.td_target(out_p['rewards'].reshape(-1), out_p['terminals'].reshape(-1), qn, ref.h['discount'])
        out_p['late'] = want.astype(np.float32).reshape(n, E)
        out_p['late_rows'] = qn
        _, _, g, _ = EP.q_independent(Pp, planes_p, out_p['actions'], out_p['late'])
        ref.apply({kk: R.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g.items()}, advance_tau=False,
                  tau=out_p['tau'])
    return outs, ref
