"""Asynchronous n-step Q-learning (Algorithm S2 of the A3C paper), numpy restatement.
Test infrastructure only (imported by tests/test_q_nstep_cpu.py and tests/test_gpu_q_nstep.py).

The rule, as include/a3c_hip.h states it (everything in float64):

    B_e = max_a Qt(s_n)[e][a]                        Qt: the target network
          double Q: Qt(s_n)[e][argmax_a Qo(s_n)[e][a]]   Qo: the rollout's own parameters; first maximum
    R   = B_e
    for i = n-1 .. 0:   if term[i][e]: R = 0;   R = r[i][e] + discount * R;   target[i][e] = (float)R

nstep_q_target_ref is that rule; NStepQ turns an oracle.engine_ref.EngineRef (or a subclass on another
env) into the n-step learner; NStepRc lets _engine_parity.check_overlap_vs_oracle, which forms the
overlap pipeline's late targets itself, form them by the same rule."""
import numpy as np

from oracle import ref_cpu as R
from oracle.engine_ref import EngineRef, acts_batch


def nstep_q_target_ref(rewards, terms, q_boot, q_sel, discount, out_dtype=np.float32):
    """rewards, terms [n, E]; q_boot [E, A] the bootstrap state's Q rows (live columns only); q_sel
    [E, A] or None.  Returns the targets [n, E] float32 (out_dtype=np.float64: before that rounding)."""
    rewards, terms = np.asarray(rewards), np.asarray(terms)
    qb = np.asarray(q_boot)
    n, E = rewards.shape
    assert terms.shape == (n, E) and qb.shape[0] == E
    if q_sel is None:
        boot = qb.max(axis=1)
    else:
        boot = qb[np.arange(E), np.argmax(np.asarray(q_sel), axis=1)]      # np.argmax: the first maximum
    ret = boot.astype(np.float64)
    out = np.empty((n, E), out_dtype)
    for i in range(n - 1, -1, -1):
        ret = np.where(terms[i] != 0, np.float64(0.0), ret)
        ret = rewards[i].astype(np.float64) + np.float64(discount) * ret
        out[i] = ret
    return out


def nstep_q_target_brute(rewards, terms, q_boot, q_sel, discount):
    """The definition without the recursion: target[i][e] = sum_k discount^k r[i+k][e] up to the
    first terminal at or after i, plus discount^(n-i) B_e when there is none.  float64 [n, E]."""
    rewards, terms = np.asarray(rewards, np.float64), np.asarray(terms)
    qb = np.asarray(q_boot, np.float64)
    n, E = rewards.shape
    out = np.zeros((n, E), np.float64)
    for e in range(E):
        boot = qb[e].max() if q_sel is None else qb[e][int(np.argmax(np.asarray(q_sel)[e]))]
        for i in range(n):
            total, cut = 0.0, False
            for k in range(n - i):
                total += discount ** k * rewards[i + k, e]
                if terms[i + k, e]:
                    cut = True
                    break
            out[i, e] = total if cut else total + discount ** (n - i) * boot
    return out


# ------------------------------------------------------------------ data of the stand-alone op
OP_E = (1, 37, 300)                          # one thread, a partial block, past the 256-thread block
OP_N = (1, 2, 5, 64)
OP_AZS = ((1, 1), (3, 4), (6, 8), (18, 20))
CLIPPED = np.array([-2, -1, 0, 0, 0, 1], np.float32)     # the engine's clipped rewards, life-loss penalty included


def op_terminals(n, E, rng, free):
    """Terminals [n, E].  Envs in `free` have none (their bootstrap is used at full depth); the others
    get random ones plus, by env (every pattern on every env when fewer than 4 are not free): i = 0, an
    interior step, i = n-1, two steps in a row."""
    terms = (rng.random((n, E)) < 0.1).astype(np.uint8)
    mid = n // 2
    busy = [e for e in range(E) if e not in free]
    for j, e in enumerate(busy):
        for p in (range(4) if len(busy) < 4 else (j % 4,)):
            if p == 0:
                terms[0, e] = 1
            elif p == 1:
                terms[mid, e] = 1
            elif p == 2:
                terms[n - 1, e] = 1
            else:
                terms[mid, e] = 1
                terms[min(mid + 1, n - 1), e] = 1
    terms[:, sorted(free)] = 0
    return terms


def op_cases(n, E, A, zs, normal_rewards=False):
    """The data sets the GPU test runs at (n, E, A, zs): a list of dicts rewards, terms [n, E], q_boot,
    q_sel [E, zs] (NaN outside the A live columns).  E >= 5: one set, envs e % 5 == 4 without a terminal;
    smaller E: two sets, the second without any terminal.  Wherever an env has no terminal (and A > 1)
    q_sel's argmax is q_boot's argmin, so double Q must change its targets."""
    sets = []
    frees = [set(range(4, E, 5))] if E >= 5 else [set(), set(range(E))]
    for v, free in enumerate(frees):
        rng = np.random.default_rng([n, E, A, zs, v, int(normal_rewards)])
        rewards = (rng.standard_normal((n, E)).astype(np.float32) if normal_rewards
                   else rng.choice(CLIPPED, (n, E)))
        q_boot = np.full((E, zs), np.nan, np.float32)
        q_sel = np.full((E, zs), np.nan, np.float32)
        q_boot[:, :A] = rng.standard_normal((E, A)).astype(np.float32)
        q_sel[:, :A] = rng.standard_normal((E, A)).astype(np.float32)
        for e in free:
            q_sel[e, :A] = -q_boot[e, :A]
        sets.append(dict(rewards=rewards, terms=op_terminals(n, E, rng, free), q_boot=q_boot, q_sel=q_sel))
    return sets


class NStepQ:
    """Mixin in front of EngineRef (or a subclass of it): iterate() takes the parent's rollout and
    replaces the one-step TD target by the n-step target of the rollout, bootstrapped from the
    target network on s_n (double_q: at the argmax of self.params there), then runs the parent's Q
    loss / backward / clip on it."""

    def iterate(self, forced_actions=None, grads=True):
        assert self.algo == 'q' and not self.lstm
        out = super().iterate(forced_actions, grads=False)
        n, A, h = self.n, self.A, self.h
        s_n = self.states(self.tau + n)
        qt = R.forward(self.tparams, s_n, 'q', dtype=self.dtype, keep=False)['z']
        qsel = None
        if self.double_q:
            qo = R.forward(self.params, s_n, 'q', dtype=self.dtype, keep=False)['z']
            qsel = qo[:, :A].astype(np.float32)
            out['q_boot_online'] = qo
        out['q_boot'] = qt
        target = nstep_q_target_ref(out['rewards'], out['terminals'], qt[:, :A].astype(np.float32), qsel,
                                    h['discount'])
        out['target'] = target
        if not grads:
            return out
        # the parent's lines for algo q (oracle/engine_ref.py iterate), on this target
        states = np.concatenate([self.states(self.tau + t) for t in range(n)])      # b = t*E + e
        B = n * self.E
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


class NStepQEngineRef(NStepQ, EngineRef):
    """oracle.engine_ref.EngineRef learning by n-step Q (the synthetic env)."""


class NStepRc:
    """oracle.ref_cpu with td_target / td_target_double replaced by the n-step rule, for
    _engine_parity.check_overlap_vs_oracle: that check forms the late targets of rollout k-1 itself,
    from the oracle's forward of the rollout's next states s_1 .. s_n ([n*E, zs] rows, b = t*E + e)
    with the target network as it stands at gradient time (double_q: and with the rollout's own
    parameters).  The n-step rule reads the last E rows of those, s_n, and nothing else."""

    def __init__(self, n, E, A):
        self.n, self.E, self.A = int(n), int(E), int(A)

    def __getattr__(self, name):
        return getattr(R, name)

    def _rows(self, q):
        q = np.asarray(q)
        assert q.shape[0] == self.n * self.E
        return q[(self.n - 1) * self.E:, :self.A].astype(np.float32)

    def td_target(self, reward, terminal, q_next, discount=0.99):
        return nstep_q_target_ref(np.asarray(reward).reshape(self.n, self.E), np.asarray(terminal).reshape(self.n, self.E),
                                  self._rows(q_next), None, discount).reshape(-1)

    def td_target_double(self, reward, terminal, q_next_target, q_next_online, discount=0.99):
        return nstep_q_target_ref(np.asarray(reward).reshape(self.n, self.E), np.asarray(terminal).reshape(self.n, self.E),
                                  self._rows(q_next_target), self._rows(q_next_online), discount).reshape(-1)
