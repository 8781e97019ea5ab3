"""Asynchronous one-step and n-step Sarsa (Engine(algo='q', sarsa=1)), numpy restatement.
Test infrastructure only (imported by tests/test_sarsa_cpu.py and tests/test_gpu_sarsa.py).

The rule, as include/a3c_hip.h states it (everything in float64):

    a_n[e] = the draw the rollout's head would make for env e at step n of the rollout, from the Q rows of
             s_n under the rollout's own parameters:  u < eps ? rnd : first argmax_a Qo(s_n)[e][a]
    one-step, b = i*E + e:   a' = i < n-1 ? actions[i+1][e] : a_n[e]
                             target[b] = (float)((1 - term[b]) * discount * Qt(s_{i+1})[e][a'] + r[b])
    n-step:                  R = Qt(s_n)[e][a_n[e]]
                             for i = n-1 .. 0:  if term[i][e]: R = 0;  R = r[i][e] + discount * R;  target[i][e] = (float)R
    an action word w is the column (uint32)w % A.

sarsa_target_ref is that rule and boot_action_ref the draw; Sarsa turns an oracle.engine_ref.EngineRef (or a
subclass on another env) into the Sarsa learner; SarsaRc lets _engine_parity.check_overlap_vs_oracle, which
forms the overlap pipeline's late targets itself, form them by the same rule, with the rollout's actions and
a_n carried by the oracle (Sarsa.boot_hist)."""
import numpy as np

import _qn_ref as Q
from oracle import philox as px
from oracle import ref_cpu as R
from oracle.engine_ref import EngineRef, acts_batch


def column(words, A):
    """The column an action word selects: the word as an unsigned 32-bit value, modulo A."""
    return (np.asarray(words).astype(np.int64) & 0xFFFFFFFF) % int(A)


def sarsa_target_ref(rewards, terms, actions, boot_actions, q_target, A, discount, nstep, out_dtype=np.float32):
    """rewards, terms, actions [n, E]; boot_actions [E]; q_target the target network's rows (columns >= A are
    never read): [n*E, >= A] of s_1 .. s_n (b = i*E + e), or with nstep [E, >= A] of s_n.  Returns the targets
    [n, E] float32 (out_dtype=np.float64: before that rounding)."""
    rewards, terms, actions = np.asarray(rewards), np.asarray(terms), np.asarray(actions)
    qt = np.asarray(q_target)
    n, E = rewards.shape
    assert terms.shape == (n, E) and actions.shape == (n, E) and np.asarray(boot_actions).shape == (E,)
    an = column(boot_actions, A)
    out = np.empty((n, E), out_dtype)
    if nstep:
        assert qt.shape[0] == E
        ret = qt[np.arange(E), an].astype(np.float64)
        for i in range(n - 1, -1, -1):
            ret = np.where(terms[i] != 0, np.float64(0.0), ret)
            ret = rewards[i].astype(np.float64) + np.float64(discount) * ret
            out[i] = ret
        return out
    assert qt.shape[0] == n * E
    for i in range(n):
        a = column(actions[i + 1], A) if i < n - 1 else an
        m = qt[i * E + np.arange(E), a].astype(np.float64)
        t = (terms[i] != 0).astype(np.float64)
        out[i] = (1.0 - t) * np.float64(discount) * m + rewards[i].astype(np.float64)      # ref_cpu.td_target's order
    return out


def sarsa_target_brute(rewards, terms, actions, boot_actions, q_target, A, discount, nstep):
    """The definition, cell by cell and without the recursion.  float64 [n, E]."""
    rewards, terms, actions = np.asarray(rewards, np.float64), np.asarray(terms), np.asarray(actions)
    qt = np.asarray(q_target, np.float64)
    n, E = rewards.shape
    out = np.zeros((n, E), np.float64)
    for e in range(E):
        an = (int(boot_actions[e]) & 0xFFFFFFFF) % A
        for i in range(n):
            if not nstep:
                a = an if i == n - 1 else (int(actions[i + 1, e]) & 0xFFFFFFFF) % A
                out[i, e] = rewards[i, e] + (0.0 if terms[i, e] else discount * qt[i * E + e, a])
                continue
            total, cut = 0.0, False
            for k in range(n - i):
                total += discount ** k * rewards[i + k, e]
                if terms[i + k, e]:
                    cut = True
                    break
            out[i, e] = total if cut else total + discount ** (n - i) * qt[e, an]
    return out


def argmax_actions(q_rows, n, E, A):
    """(actions [n, E], boot [E]) that make a' the first argmax of every row of q_rows [n*E, >= A] (row i*E + e
    is s_{i+1}): actions[i+1] = argmax of rows i, boot = argmax of rows n-1; actions[0] is not an a' (zeros)."""
    arg = np.argmax(np.asarray(q_rows)[:, :A], axis=1).astype(np.int32).reshape(n, E)
    actions = np.zeros((n, E), np.int32)
    actions[1:] = arg[:-1]
    return actions, arg[n - 1].copy()


# ------------------------------------------------------------------ data of the stand-alone ops
OP_E, OP_N, OP_AZS = Q.OP_E, Q.OP_N, Q.OP_AZS
BAD_WORDS = (-1, None, 2 ** 31 - 1)          # None: A itself


def op_cases(n, E, A, zs, normal_rewards=False, bad_words=False):
    """The data sets the GPU test runs at (n, E, A, zs): a list of dicts rewards, terms, actions [n, E], boot [E],
    q [n*E, zs] (NaN outside the A live columns; the n-step form reads its last E rows, s_n).  Terminals by
    _qn_ref.op_terminals: E >= 5: one set, envs e % 5 == 4 without a terminal; smaller E: two sets, the second
    without any.  Actions are uniform over [0, A), but an env without a terminal has the argmin of its s_n row
    as its boot action; bad_words: a few cells of actions and boot hold -1, A and
    2^31 - 1 instead."""
    sets = []
    frees = [set(range(4, E, 5))] if E >= 5 else [set(), set(range(E))]
    for v, free in enumerate(frees):
        rng = np.random.default_rng([n, E, A, zs, v, int(normal_rewards), 77])
        rewards = (rng.standard_normal((n, E)).astype(np.float32) if normal_rewards
                   else rng.choice(Q.CLIPPED, (n, E)))
        q = np.full((n * E, zs), np.nan, np.float32)
        q[:, :A] = rng.standard_normal((n * E, A)).astype(np.float32)
        actions = rng.integers(0, A, (n, E)).astype(np.int32)
        boot = rng.integers(0, A, E).astype(np.int32)
        for e in free:                    # (A > 1: not the maximum, so the bootstrap must change the env's targets)
            boot[e] = int(np.argmin(q[(n - 1) * E + e, :A]))
        if bad_words:
            words = [A if w is None else w for w in BAD_WORDS]
            for j, w in enumerate(words):
                boot[(2 * j + v) % E] = w
                actions[(j + 1) % n, (3 * j + 1) % E] = w
        sets.append(dict(rewards=rewards, terms=Q.op_terminals(n, E, rng, free), actions=actions, boot=boot, q=q))
    return sets


def rows_of(d, nstep, n, E):
    """The target rows a form reads from a data set's q."""
    return d['q'][(n - 1) * E:] if nstep else d['q']


def boot_action_ref(q, eps, A, tau, env_id_base=0, seed=123):
    """a3c_boot_action: (actions [E] int32, random [E] bool -- the branch taken)."""
    q = np.asarray(q)
    E = q.shape[0]
    k0, k1 = px.seed_key(seed)
    ids = np.arange(env_id_base, env_id_base + E, dtype=np.uint32)
    tau = int(tau)
    x = px.philox4x32(np.uint32(tau & 0xFFFFFFFF), np.uint32(tau >> 32), ids, px.P_ACTION, k0, k1)
    u, rnd = px.u01(x[0]), (x[1] % np.uint32(A)).astype(np.int32)
    random = u < np.asarray(eps, np.float32)
    greedy = np.argmax(q[:, :A], axis=1).astype(np.int32)            # np.argmax: the first maximum
    return np.where(random, rnd, greedy).astype(np.int32), random


BOOT_TAUS = (3, 8, 7 + 2 ** 32)        # the engine's first tau, a later one, one past the counter's low word
BOOT_SEED = 0x123456789ABCDEF         # both key words set


def boot_cases(E, A, zs, ties=False):
    """Q rows [E, zs] (NaN outside the live columns) and eps [E] holding 0, 1 and values in between; ties (A >= 2):
    small integers, and every row's maximum occurs a second time behind its first occurrence or before it."""
    assert A >= 2 or not ties
    rng = np.random.default_rng([E, A, zs, int(ties), 78])
    q = np.full((E, zs), np.nan, np.float32)
    if ties:
        vals = rng.integers(0, 3, (E, A)).astype(np.float32)
        top = vals.max(axis=1)
        for e in range(E):                        # a second copy of the maximum behind the first
            first = int(np.argmax(vals[e]))
            vals[e, (first + 1 + int(rng.integers(0, A - 1))) % A] = top[e]
        q[:, :A] = vals
    else:
        q[:, :A] = rng.standard_normal((E, A)).astype(np.float32)
    eps = rng.choice(np.array([0.0, 1.0, 0.1, 0.5, 0.9], np.float32), E)
    return q, eps.astype(np.float32)


# ------------------------------------------------------------------ the oracle
class Sarsa:
    """Mixin in front of EngineRef (or a subclass of it): iterate() takes the parent's rollout, draws a_n for the
    bootstrap state s_n as the rollout's head would at step n (draw_words(n), eps(n), the first argmax of the
    fp64 forward of s_n with self.params -- the rollout's parameters), and replaces the max target by the
    Sarsa target (q_nstep: its n-step form); then the parent's Q loss / backward / clip on it.

    boot_hist: per rollout a dict actions, sampled [1, E] (a_n), z [1][E, zs], u, eps [1, E] -- the keys
    _engine_parity.assert_draws_explained reads -- kept for the late-target adapter (SarsaRc) and for the
    comparison with the engine's boot_actions.  boot_forced: set to the engine's a_n [E] to replay with it (the
    default None replays with the oracle's own draw)."""
    q_nstep = 0
    last = None                       # the newest instance (the parity checks build the oracle themselves)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.boot_hist = []
        self.boot_forced = None
        Sarsa.last = self

    def draw_boot(self):
        n, A = self.n, self.A
        z = R.forward(self.params, self.states(self.tau + n), 'q', dtype=self.dtype, keep=False)['z']
        u, rnd = self.draw_words(n)
        eps = self.eps(n)
        greedy = np.argmax(z[:, :A].astype(np.float32), axis=1).astype(np.int32)
        a_n = np.where(u < eps, rnd, greedy).astype(np.int32)
        return dict(sampled=a_n[None], z=z[None], u=np.asarray(u, np.float32)[None], eps=eps[None])

    def iterate(self, forced_actions=None, grads=True):
        assert self.algo == 'q' and not self.lstm and not self.double_q
        out = super().iterate(forced_actions, grads=False)
        n, E, A, h = self.n, self.E, self.A, self.h
        boot = self.draw_boot()
        boot['actions'] = out['actions']
        self.boot_hist.append(boot)
        a_n = boot['sampled'][0] if self.boot_forced is None else np.asarray(self.boot_forced, np.int32)
        first = n if self.q_nstep else 1
        nxt = np.concatenate([self.states(self.tau + t) for t in range(first, n + 1)])
        qt = R.forward(self.tparams, nxt, 'q', dtype=self.dtype, keep=False)['z']
        out['boot'] = boot
        out['q_target_rows'] = qt
        target = sarsa_target_ref(out['rewards'], out['terminals'], out['actions'], a_n, qt.astype(np.float32), A,
                                  h['discount'], self.q_nstep)
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


class SarsaEngineRef(Sarsa, EngineRef):
    """oracle.engine_ref.EngineRef learning by one-step Sarsa (the synthetic env)."""


class NStepSarsaEngineRef(Sarsa, EngineRef):
    """... by n-step Sarsa."""
    q_nstep = 1


class SarsaRc:
    """oracle.ref_cpu with td_target replaced by the Sarsa rule, for _engine_parity.check_overlap_vs_oracle:
    that check forms the late targets of rollout k-1 itself, after the oracle replayed rollout k, from the
    oracle's forward of the rollout's next states s_1 .. s_n ([n*E, zs] rows, b = t*E + e) with the target
    network as it stands at gradient time.  The rollout's actions and its a_n -- drawn at rollout time with the
    rollout's parameters -- come from the oracle's boot_hist[-2] (Sarsa.last: the newest oracle)."""

    def __init__(self, n, E, A, q_nstep):
        self.n, self.E, self.A, self.q_nstep = int(n), int(E), int(A), int(q_nstep)

    def __getattr__(self, name):
        return getattr(R, name)

    def td_target(self, reward, terminal, q_next, discount=0.99):
        n, E = self.n, self.E
        ref = Sarsa.last
        boot = ref.boot_hist[-2]
        a_n = boot['sampled'][0] if ref.boot_forced is None else np.asarray(ref.boot_forced, np.int32)
        q = np.asarray(q_next)
        assert q.shape[0] == n * E and q.dtype == np.float32
        rows = q[(n - 1) * E:] if self.q_nstep else q
        return sarsa_target_ref(np.asarray(reward).reshape(n, E), np.asarray(terminal).reshape(n, E), boot['actions'],
                                a_n, rows, self.A, discount, self.q_nstep).reshape(-1)

    def td_target_double(self, *args, **kw):
        raise AssertionError('Sarsa has no double-Q form')


# ------------------------------------------------------------------ the parity cases, by the oracle alone
def oracle_class(case):
    import _catch_ref as C
    base = C.CatchEngineRef if case.get('catch') else EngineRef
    return type(('NStep' if case['q_nstep'] else '') + 'Sarsa' + base.__name__, (Sarsa, base),
                dict(q_nstep=int(case['q_nstep'])))


def oracle_alone(case, extra, scale=4.0):
    """A parity case of tests/test_sarsa_cpu.PARITY replayed by the oracle with its own draws, in the order the
    case's _engine_parity check replays it (sync: rollout, gradient, apply; overlap: rollout k with the
    parameters after update k-2, the late targets of rollout k-1 behind it, apply).  extra: the options every
    case runs with.  Returns (boot_hist, the largest |Sarsa target - max target| over the rollouts)."""
    import _catch_ref as C
    import _engine_parity as EP
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    from test_episode_ends_cpu import backprop
    A, E, n, seed = case['A'], case['E'], case['n'], case['seed']
    kw = dict(case.get('opts', {}), target_q_update_step=40, **extra)
    if case.get('lr') is not None:
        kw['learning_rate'] = case['lr']
    p = init_params(param_names_shapes(A, 'q'), seed=seed, stddev=0.02 * scale)
    frames = C.FRAMES if case.get('catch') else case.get('frames', 48)
    ref = oracle_class(case)(p, E, n, A, 'q', case['lives'], frames, seed, **kw)
    ref.reset()
    if case.get('catch'):                                   # tests/test_gpu_catch.py stagger(), the oracle's half
        c, _, pp = C.decode(ref.env.frame)
        r = (np.arange(E) * ref.env.action_repeat) % (C.ROWS - 1)
        ref.env.frame[:] = C.encode(c, r, pp).astype(np.uint32)
        ref.env.ep_step[:] = r
    else:                                                   # _engine_parity.scheduled(), the oracle's half
        d = EP.schedule(E, n, backprop(case), ref.env.action_repeat)
        ref.env.ep_len[:] = (ref.env.ep_step.astype(np.int64) + d).astype(np.uint32)
    differ = 0.0

    def max_target(out, qrows):
        if case['q_nstep']:
            return Q.nstep_q_target_ref(out['rewards'], out['terminals'], qrows[:, :A].astype(np.float32), None,
                                        ref.h['discount'])
        return R.td_target(out['rewards'].reshape(-1), out['terminals'].reshape(-1), qrows[:, :A].astype(np.float32),
                           ref.h['discount']).astype(np.float32).reshape(n, E)

    if case['check'] == 'sync':
        for _ in range(case['rollouts']):
            out = ref.iterate()
            differ = max(differ, float(np.abs(out['target'] - max_target(out, out['q_target_rows'])).max()))
            ref.apply(out['clipped'])
        return ref.boot_hist, differ
    rc = SarsaRc(n, E, A, case['q_nstep'])
    hist = []
    for k in range(case['rollouts']):
        Pk = {kk: v.copy() for kk, v in ref.params.items()}
        out = ref.iterate(grads=False)
        planes = EP.rollout_planes(ref, n)
        out['next_states'] = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
        ref.tau += n
        hist.append((Pk, planes, out))
        if k == 0:
            continue
        Pp, planes_p, out_p = hist[k - 1]
        qn = R.forward(ref.tparams, out_p['next_states'], 'q', keep=False)['z'].astype(np.float32)
        want = rc.td_target(out_p['rewards'].reshape(-1), out_p['terminals'].reshape(-1), qn,
                            ref.h['discount']).astype(np.float32).reshape(n, E)
        differ = max(differ, float(np.abs(want - max_target(out_p, qn[(n - 1) * E:] if case['q_nstep'] else qn)).max()))
        _, _, g, _ = EP.q_independent(Pp, planes_p, out_p['actions'], want)
        ref.apply({kk: R.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g.items()}, advance_tau=False,
                  tau=out_p['tau'])
    return ref.boot_hist, differ
