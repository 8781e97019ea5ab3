"""Shared checks of the batched engine against the CPU replay oracle (oracle/engine_ref.py).

Test infrastructure only (imported by tests/test_gpu_*.py).  Each check drives the HIP engine
through src/engine.py (the C-ABI) and replays the same iteration on the oracle with the engine's
own action draws, then asserts:
  * env dynamics, rewards, terminals and the frame ring (Environment.screen + History) bit-exact;
  * the engine's draws agree with the oracle's policy except at fp32 cdf boundaries;
  * n-step returns / TD targets within 1e-5;
  * losses within 1e-4 of max(1, |loss|) (north star: 1e-3);
  * gradients within 1e-4 relative-L2 of the fp64 oracle backward on the engine's own saved
    activations (same ReLU masks), and within 2e-2 of the fully independent fp64 forward+backward;
  * the saved activations themselves (act_l*, and the LSTM sequence) within 1e-4 of the oracle's
    independent fp64 batch forward (assert_saved_acts);
  * parameters after clip + RMSProp within 1e-5 over the iterations.

Three legs, because no two of them see everything:
  1. same-activation gradients (1e-4): pins the backward kernels, but believes whatever the engine
     saved -- a stale or misplaced sample in act_l* passes it trivially;
  2. independent gradients (2e-2; the bound leaves room for ReLU-mask flips at fp32): pins the
     whole update against an fp64 forward + backward that never saw the engine's buffers, but the
     gradient is a sum over the batch in which a sample weighs as much as its dz (a3c: its
     advantage R - V), so one wrong sample can be diluted below the bound.  Measured with the
     oracle alone (nips trunk, A = 6, init stddev 0.08, seed 131, the first rollout): sample b's
     saved l1 / l2 / h3 replaced by sample b+1's and back-propagated, the largest rel-L2 change
     over the weight tensors, per replaced sample:

       batch                          min      median   max      under 2e-2     that sample's l1
       a3c, B = 40   (E = 8,   n = 5) 0.007    0.086    0.75     3 of 40        off by >= 0.35
       a3c, B = 1280 (E = 256, n = 5) 0.0001   0.0022   0.050    37 of 40 (*)   off by >= 0.35
       q,   B = 40                    0.0002   0.042    0.061    5 of 40        off by >= 0.32
                                                   (*) every 32nd sample      (layer max 1.0)

     (a3c, B = 40, two updates later: 21 of 40 under 2e-2.)  At the shapes the bench runs, a whole
     stale sample passes the 2e-2 check nine times in ten; at the small shapes, whenever its
     advantage is small (tests/test_parity_checks_cpu.py asserts that for the least-advantage
     sample);
  3. saved activations against the independent forward (1e-4, the bound of assert_z for the same
     class of arithmetic): a stale sample misses it by more than three orders of magnitude.  This
     is the failure the overlap pipeline is exposed to -- a slot is written by the rollout stream
     and read one iteration later by the backward stream, and the fused kernel writes step t+1's
     l1 / l2 from step t's launch, across the slot boundary -- so the overlap checks run it on slot
     k-1 after iterate() k, the buffer the backward just consumed.
Every check_* asserts all three plus the independent loss.  Q-learning on the overlap pipeline
forms its TD targets late (with the target network as it stands after rollout k), so its
independent leg is q_independent on those late targets, not the rollout-time oracle batch.
The largest independent rel-L2 a check saw is printed at its end and kept in INDEPENDENT_MAX.
Episode boundaries: every check also counts the terminals and game overs of its rollouts per
(rollout, t) cell (EpisodeCount; printed, kept in EPISODE_COUNTS and left on the returned oracle as
ref.episode_counts), and compares the env state after every synchronised iteration.  The env ends
an episode only after 200-2000 steps, so a check that must see game overs passes
start=scheduled(K), which shortens ep_len in engine and oracle alike (schedule, end_episodes);
tests/test_gpu_episode_ends.py does, and asserts the counts.
Reference: agent.py:141-207 (act / observe / batch_update), agent.py:306-321 (loss, clip, apply),
network.py:60-94 + assets/a3c.png (A3C losses, n-step returns), main.py:63-65 (RMSProp)."""
import numpy as np
import torch

from oracle import ref_cpu as Rc
from oracle.engine_ref import EngineRef, acts_batch


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# engine options the oracle takes under the same name: a value given to the engine reaches EngineRef
REF_KEYS = ('target_q_update_step', 'learning_rate', 'frame84', 'double_q', 'ep_start', 'ep_end_t', 'learn_start',
            'dqn_type', 'gamma', 'discount', 'beta', 'max_step', 'decay', 'momentum', 'epsilon', 'clip_norm',
            'literal_adv', 'random_start', 'action_repeat')


def build(algo, A, E, n, lives, seed, frames=48, use_graph=False, scale=4.0, params=None, **kw):
    """An engine and an oracle from the same seed and initial parameters (stddev 0.02*scale, or
    params(names_shapes) -> {name: array} where given).
    external_env=True: the engine's frames come from host-stepped envs (no device frame pool)."""
    from src.engine import Engine
    from src.initializers import init_params, flatten_host
    from src.kernels import param_names_shapes
    eng_frames = 1 if kw.get('external_env') else frames
    eng = Engine(num_envs=E, n_step=n, action_size=A, algo=algo, start_lives=lives, num_frames=eng_frames, seed=seed,
                 use_graph=use_graph, **kw)
    ns = param_names_shapes(A, algo, dqn_type=kw.get('dqn_type', 'nips'))
    p = init_params(ns, seed=seed, stddev=0.02 * scale) if params is None else params(ns)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), p))
    ref = EngineRef(p, E, n, A, algo, lives, frames, seed, **{k: v for k, v in kw.items() if k in REF_KEYS})
    ref.reset()
    return eng, ref, ns


def unflat(eng, ns, flat):
    f = flat.cpu().numpy()
    return {name: f[off:off + sz].reshape(shp) for (name, shp), off, sz in zip(ns, eng.offsets, eng.sizes)}


def same_act_grads(slot, planes, P, algo, A, n, E, tgt, beta=0.01, literal_adv=False):
    """oracle loss + backward of one rollout on the engine's saved activations of that rollout
    (slot: Engine.slot(k), or the engine itself in sync mode)."""
    g = (lambda k: slot[k]) if isinstance(slot, dict) else (lambda k: getattr(slot, k))
    nature = ('act_l4' in slot) if isinstance(slot, dict) else getattr(slot, 'dqn_type', 'nips') == 'nature'
    B = n * E
    zw = A + 1 if algo == 'a3c' else A
    z = g('z').cpu().numpy()[:n].reshape(B, -1)[:, :zw].astype(np.float64)
    x0 = Rc.states_nhwc(planes).astype(np.float64) / 255.0
    if nature:      # network.py:30-42: conv 32 / 64 / 64 (NHWC), flat 3136, fc 512
        l1 = g('act_l1').cpu().numpy().astype(np.float64).reshape(B, 20, 20, 32)
        l2 = g('act_l2').cpu().numpy().astype(np.float64).reshape(B, 9, 9, 64)
        l3 = g('act_l3').cpu().numpy().astype(np.float64)
        fwd = dict(z=z, h3=g('act_l4').cpu().numpy().astype(np.float64), flat=l3,
                   acts=[x0, l1, l2, l3.reshape(B, 7, 7, 64)])
    else:
        l1 = g('act_l1').cpu().numpy().astype(np.float64).reshape(B, 20, 20, 16)
        l2 = g('act_l2').cpu().numpy().astype(np.float64)
        fwd = dict(z=z, h3=g('act_l3').cpu().numpy().astype(np.float64), flat=l2,
                   acts=[x0, l1, l2.reshape(B, 9, 9, 32)])
    acts = g('actions').cpu().numpy().reshape(-1)
    if algo == 'a3c':
        losses, dz = Rc.a3c_loss_and_dz(z, acts, tgt.reshape(-1).astype(np.float64), beta, bool(literal_adv))
    else:
        loss, dz = Rc.q_loss_and_dz(z, acts, tgt.reshape(-1).astype(np.float64))
        losses = dict(loss=loss)
    gr = Rc.backward(P, fwd, dz, algo, 'nature' if nature else 'nips')
    return losses, {k: np.asarray(v, np.float32).reshape(P[k].shape) for k, v in gr.items()}


def assert_saved_acts(slot, out, n, E, tag, rtol=1e-4):
    """A slot's saved trunk activations (and, with the LSTM head, its sequence buffers) against
    the oracle's independent fp64 batch forward out['acts_batch'] (/ out['lstm']), in the layouts
    same_act_grads assumes (NHWC rows, b = t*E + e).  Bound: assert_z's, for the same class of
    arithmetic (fp32 MFMA sums against fp64); lstm_h keeps its own rtol 1e-4 / atol 2e-5."""
    g = (lambda k: slot[k]) if isinstance(slot, dict) else (lambda k: getattr(slot, k))
    ab = out['acts_batch']
    layers = [k for k in ('l1', 'l2', 'l3') if k in ab] + ['h3']
    nature = ('act_l4' in slot) if isinstance(slot, dict) else getattr(slot, 'dqn_type', 'nips') == 'nature'
    assert len(layers) == (4 if nature else 3), (tag, layers, nature)
    B = n * E
    for i, k in enumerate(layers):
        a = g(f'act_l{i + 1}').cpu().numpy()
        r = ab[k].reshape(B, -1)
        assert a.size == r.size, (tag, k, a.shape, r.shape)
        np.testing.assert_allclose(a.reshape(B, -1), r, rtol=rtol, atol=rtol * max(1.0, float(np.abs(r).max())),
                                   err_msg=str((tag, f'act_l{i + 1}')))
    if 'lstm' in out:
        seq = out['lstm']
        # (lstm_hp / lstm_cp: every step's carried-in state, zeroed where the step before it -- the
        # previous rollout's last step for t = 0 -- was terminal)
        for key, rk in (('lstm_h', 'H'), ('lstm_hp', 'HP')):
            np.testing.assert_allclose(g(key).cpu().numpy(), seq[rk], rtol=1e-4, atol=2e-5, err_msg=str((tag, key)))
        for key, rk in (('lstm_c', 'C'), ('lstm_cp', 'CP'), ('lstm_gates', 'G')):
            r = np.asarray(seq[rk])
            np.testing.assert_allclose(g(key).cpu().numpy(), r, rtol=rtol,
                                       atol=rtol * max(1.0, float(np.abs(r).max())), err_msg=str((tag, key)))


INDEPENDENT_MAX = {}     # label of a check -> the largest independent rel-L2 it saw


def assert_independent_grads(G, ref_grads, names, tag, worst=None, bound=2e-2):
    """Every gradient tensor within `bound` relative-L2 of the fully independent fp64 forward +
    backward (ReLU-mask flips at fp32 allowed); worst: a dict collecting the per-tensor maxima."""
    for name in names:
        r = float(rel_l2(G[name], ref_grads[name]))
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), r)
        assert r < bound, (tag, name, r)


def report_independent(label, worst):
    """Log the headroom of a check's 2e-2 assertions (run pytest with -s to see it)."""
    top = max(worst.values()) if worst else 0.0
    INDEPENDENT_MAX[label] = top
    print(f'independent rel-L2 max {label}: {top:.3e} ' +
          ' '.join(f'{k}={v:.1e}' for k, v in sorted(worst.items())))
    return top


EPISODE_COUNTS = {}      # label of a check -> the terminals and game overs it saw (EpisodeCount.report)


def schedule(E, n, K, action_repeat=1):
    """Steps-from-now d [E] that put one game over on every (rollout, t) cell of K rollouts of n
    steps when E >= n * K: env e ends at env step e % (n * K).  In raw emulator steps; with
    action_repeat = r the episode of env e ends e % r raw steps before its act would finish, in
    the middle of the repeat (environment.py:78-96, the break on terminal)."""
    e = np.arange(E, dtype=np.int64)
    r = int(action_repeat)
    return r * (1 + e % (n * K)) - e % r


def end_episodes(eng, ref, d, host_envs=None):
    """End env e's episode d[e] >= 1 raw steps from now, in the engine and the oracle alike:
    ep_len = ep_step + d (the oracle's ep_step: the two are in lock-step).  The engine's env state
    is double-buffered by step parity; both rows are written, and the one that is not current is
    overwritten by the next step.  Only on an idle engine.  After its reset an env draws a new
    ep_len >= 200, so every env ends once per call.  host_envs: the per-env SyntheticAtari objects
    of a host-stepped engine (whose envs are not on the device), shortened instead."""
    d = np.asarray(d, np.int64)
    assert d.shape == (ref.E,) and (d >= 1).all()
    new = ref.env.ep_step.astype(np.int64) + d
    ref.env.ep_len[:] = new.astype(np.uint32)
    if host_envs is not None:
        for e, env in enumerate(host_envs):
            assert env.E == 1 and int(env.ep_step[0]) == int(ref.env.ep_step[e])
            env.ep_len[0] = new[e]
        return
    torch.cuda.synchronize()
    row = torch.as_tensor(new.astype(np.int32)).cuda()
    for parity in range(2):
        eng._env['ep_len'][parity].copy_(row)
    torch.cuda.synchronize()


def scheduled(K, host_envs=None):
    """A check's start(eng, ref) hook: schedule() over K back-propagated rollouts."""
    def start(eng, ref):
        end_episodes(eng, ref, schedule(ref.E, ref.n, K, ref.env.action_repeat),
                     None if host_envs is None else host_envs())
    return start


class EpisodeCount:
    """Terminals and game overs of a check's rollouts by (rollout, t) cell, from the oracle's
    replay (out['terminals'], out['game_overs']: the env_reset calls, where `episode` advanced)."""

    def __init__(self):
        self.terms, self.overs = [], []

    def add(self, out):
        self.terms.append(out['terminals'].astype(np.int64).sum(axis=1))
        self.overs.append(out['game_overs'].astype(np.int64).sum(axis=1))

    def report(self, label, backprop=None):
        """Log the counts (pytest -s) and keep them in EPISODE_COUNTS[label].  backprop: how many of
        the rollouts were back-propagated (default: all); 'cells' / 'terminal_cells' [backprop, n]
        hold those rollouts only, which is what a coverage assertion is about."""
        terms, overs = np.array(self.terms), np.array(self.overs)
        K = len(terms) if backprop is None else backprop
        c = dict(rollouts=len(terms), backprop=K, terminals=int(terms.sum()), first=int(terms[:, 0].sum()),
                 last=int(terms[:, -1].sum()), game_overs=int(overs.sum()), cells=overs[:K], terminal_cells=terms[:K])
        EPISODE_COUNTS[label] = c
        print(f"episode ends {label}: terminals {c['terminals']} (first / last step {c['first']} / {c['last']}) "
              f"game overs {c['game_overs']}, per (rollout, t) of the {K} back-propagated rollouts "
              f"{overs[:K].tolist()}")
        return c


def q_independent(P, planes, actions, want):
    """The independent leg of Q-learning for given (late) TD targets: the oracle's own fp64 forward
    of the rollout's states with parameters P, its loss against `want` and its backward.
    Returns (losses, z [B, A], gradients, acts_batch)."""
    fwd = Rc.forward(P, Rc.states_nhwc(planes), 'q')
    loss, dz = Rc.q_loss_and_dz(fwd['z'], np.asarray(actions).reshape(-1), np.asarray(want, np.float64).reshape(-1))
    ab = acts_batch(fwd)
    g = Rc.backward(P, fwd, dz, 'q')
    return dict(loss=loss), fwd['z'], {k: np.asarray(v, np.float32).reshape(P[k].shape) for k, v in g.items()}, ab


def rollout_planes(ref, n):
    """[n*E,4,84,84] u8 states of the oracle's current rollout (b = t*E + e); call after
    ref.iterate() (the states hold the frames the rollout produced) and before tau advances."""
    return np.concatenate([np.transpose(ref.states(ref.tau + t), (0, 3, 1, 2)) for t in range(n)])


def _boundary_distance(z, a, u):
    """How far u lies outside action a's interval [cdf[a-1], cdf[a]) of softmax(z) in fp64 (the
    draw rule of ref_cpu.sample_categorical: the first j with cdf[j] > u, else A-1); 0 inside."""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max())
    cdf = np.cumsum(e / e.sum())
    lo = cdf[a - 1] if a > 0 else 0.0
    hi = cdf[a] if a < len(z) - 1 else np.inf
    return max(lo - float(u), float(u) - hi, 0.0)


def assert_draws_explained(acts, out, algo, A, tag, z_eng=None, tol=1e-5, tol_self=1e-6):
    """Zero unexplained action mismatches (agent.py:141-151 epsilon-greedy, network.py:72
    categorical draw).  Every engine action equals the oracle's draw on the same Philox word u,
    except where the two fp32 evaluations may legitimately disagree:
      * a3c: u lies within `tol` of the boundary of the engine's action's interval in the oracle's
        own fp64 CDF (its independent forward's logits);
      * q: u >= eps for both (the random branch is exact), and the engine's greedy action's q is
        within `tol` (relative to max(1, |q|)) of the oracle's top value -- a near-tie.
    z_eng [n, E, >= A]: the engine's own saved head rows; the sampler restated on them must put
    every engine action inside its interval to `tol_self` (ulp-level: the fused sampler's expf
    against numpy's exp), which pins the fused head kernel's draw itself."""
    acts = np.asarray(acts).reshape(out['sampled'].shape)
    bad = []
    for t, e in np.argwhere(acts != out['sampled']):
        a, b = int(acts[t, e]), int(out['sampled'][t, e])
        z = out['z'][t][e, :A]
        if algo == 'a3c':
            d = _boundary_distance(z, a, out['u'][t, e])
            why = d <= tol
        else:
            u, eps = float(out['u'][t, e]), float(out['eps'][t, e])
            gap = float(np.max(z) - z[a])
            d = gap / max(1.0, float(np.abs(z).max()))
            why = (u >= eps or abs(u - eps) <= tol) and d <= tol
        if not why:
            bad.append((int(t), int(e), a, b, d))
    assert not bad, (tag, 'unexplained draw mismatches (t, e, engine, oracle, distance)', len(bad), bad[:8])
    if z_eng is not None and algo == 'a3c':
        ze = np.asarray(z_eng, np.float64).reshape(acts.shape + (-1,))[..., :A]
        off = [(int(t), int(e), int(acts[t, e])) for t in range(acts.shape[0]) for e in range(acts.shape[1])
               if _boundary_distance(ze[t, e], acts[t, e], out['u'][t, e]) > tol_self]
        assert not off, (tag, 'engine draw outside its own CDF interval (t, e, action)', len(off), off[:8])
    return len(np.argwhere(acts != out['sampled']))


def assert_z(z_eng, z_ref, A_or_zw, tag, rtol=1e-4):
    """The rollout's saved head rows [n, E, zs] against the oracle's independent fp64 forward."""
    ze = np.asarray(z_eng, np.float64)[..., :A_or_zw]
    zr = np.asarray(z_ref, np.float64)[..., :A_or_zw]
    np.testing.assert_allclose(ze, zr, rtol=rtol, atol=rtol * max(1.0, float(np.abs(zr).max())), err_msg=str(tag))


def assert_losses(loss, ref_losses, algo, tag):
    keys = ('policy', 'value', 'entropy', 'total') if algo == 'a3c' else ('loss',)
    for i, k in enumerate(keys):
        # sums of +- per-sample terms: 1e-4 of max(1, |sum|) (north star 1e-3)
        assert abs(loss[i] - ref_losses[k]) <= 1e-4 * max(1.0, abs(ref_losses[k])), (tag, k, loss[i], ref_losses[k])


def assert_params(eng, ns, ref, tag):
    P = unflat(eng, ns, eng.params)
    for name, _ in ns:
        d = np.abs(P[name] - ref.params[name]).max()
        assert d <= 1e-5 * max(1.0, np.abs(ref.params[name]).max()), (tag, name, d)


def assert_env_state(eng, ref, tag, tau=None):
    """tau: the step whose parity row is current (default: the engine's own tau counter)."""
    for f, ref_v in (('frame', ref.env.frame), ('lives', ref.env.lives), ('episode', ref.env.episode),
                     ('ep_step', ref.env.ep_step), ('ep_len', ref.env.ep_len)):
        got = eng.env_field(f) if tau is None else eng._env[f][int(tau) & 1]
        assert np.array_equal(got.cpu().numpy(), ref_v.astype(np.int32)), (tag, f)


def check_sync_vs_oracle(algo, A, E, n, lives, iters=3, seed=None, frames=48, scale=4.0, independent=True,
                         host_pool=None, on_update=None, start=None, **kw):
    """Synchronous engine (rollout_grad + apply): every iteration against the oracle.
    on_update(it, eng, ref, lr): called after every checked update with the oracle's learning rate
    of that update (for checks of a case's own: the schedule word, the clip regimes).
    start(eng, ref): called once before the first rollout (to resume both at a later step).
    host_pool(seed): a host env pool factory -- the engine then runs with external_env and its
    n env steps are driven by Engine.rollout_host."""
    seed = 123 + E if seed is None else seed
    kw.setdefault('target_q_update_step', 40)
    pool = None
    if host_pool is not None:
        kw['external_env'] = True
    eng, ref, ns = build(algo, A, E, n, lives, seed=seed, frames=frames, scale=scale, **kw)
    if host_pool is not None:
        pool = host_pool(seed)
        eng.begin_host(pool)
    if start is not None:
        start(eng, ref)
    torch.cuda.synchronize()
    if pool is None:
        assert np.array_equal(eng.env_frame.cpu().numpy(), ref.env.frame.astype(np.int32))
    R = eng.ring_slots
    worst = {}
    counts = EpisodeCount()
    ring = eng.frame_ring.cpu().numpy()
    for c in range(4):
        assert np.array_equal(ring[:, c % R], ref.ring[:, c % R])
    for it in range(iters):
        Pk = unflat(eng, ns, eng.params)          # the parameters this rollout runs with
        if pool is not None:
            eng.rollout_host(pool)
        eng.rollout_grad()
        torch.cuda.synchronize()
        acts = eng.actions.cpu().numpy()
        out = ref.iterate(forced_actions=acts)
        counts.add(out)
        planes = rollout_planes(ref, n)           # after: the rollout's own frames are in the ring
        zw = A + 1 if algo == 'a3c' else A
        z_eng = eng.z.cpu().numpy()[:n].reshape(n, E, -1)
        assert_draws_explained(acts, out, algo, A, it, z_eng=z_eng)
        assert_z(z_eng, out['z'], zw, it)
        assert_saved_acts(eng, out, n, E, ('saved', it))
        assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards']), it
        assert np.array_equal(eng.terminals.cpu().numpy(), out['terminals']), it
        gr = eng.frame_ring.cpu().numpy()
        bad = [(e, sl) for e in range(E) for sl in range(R) if not np.array_equal(gr[e, sl], ref.ring[e, sl])]
        assert not bad, (it, ref.tau, bad[:8])
        tgt = eng.returns.cpu().numpy()
        np.testing.assert_allclose(tgt, out['target'], rtol=1e-5, atol=1e-5)
        assert_losses(eng.loss.cpu().numpy(), out['losses'], algo, it)
        G = unflat(eng, ns, eng.grads)
        # single GPU: the per-tensor clip is fused into apply, so after rollout_grad the buffer
        # holds the raw gradient
        _, g_same = same_act_grads(eng, planes, Pk, algo, A, n, E, tgt, ref.h['beta'], ref.h['literal_adv'])
        for name, _ in ns:
            assert rel_l2(G[name], g_same[name]) < 1e-4, (it, name, rel_l2(G[name], g_same[name]))
        if independent:     # fully independent fp64 oracle: ReLU-mask flips allowed
            assert_independent_grads(G, out['grads'], [name for name, _ in ns], it, worst)
        eng.apply()
        torch.cuda.synchronize()
        ss = eng.sumsq.cpu().numpy()
        for i, (name, _) in enumerate(ns):
            assert np.isclose(ss[i], np.sum(G[name].astype(np.float64) ** 2), rtol=1e-5), (it, name)
        # the oracle optimizer consumes the same-mask gradients so the two parameter
        # trajectories stay comparable at 1e-5 over iterations
        lr = ref.apply({k: Rc.clip_by_norm(v, ref.h['clip_norm']) for k, v in g_same.items()})
        assert_params(eng, ns, ref, it)
        if on_update is not None:
            on_update(it, eng, ref, lr)
        cnt = eng.counters.cpu().numpy()
        assert cnt[0] == ref.tau and cnt[1] == ref.global_step
        if pool is None:
            assert_env_state(eng, ref, it)
        if algo == 'q':
            T = unflat(eng, ns, eng.target_params)
            for name, _ in ns:
                np.testing.assert_allclose(T[name], ref.tparams[name], rtol=1e-5, atol=1e-6)
    if pool is not None:
        pool.close()
    label = f'sync {algo} A={A} E={E} n={n} {eng.dqn_type}'
    report_independent(label, worst)
    ref.episode_counts = counts.report(label)
    return eng, ref


def check_overlap_vs_oracle(A, E, n, lives, rollouts=5, seed=77, frames=48, scale=4.0, algo='a3c', hogwild=False,
                            on_update=None, start=None, **kw):
    """Overlap (stale-1) pipeline: rollout k uses the parameters after update k-2.  The oracle is
    replayed in that order with the engine's own actions and activations.  algo='q': the TD targets
    of rollout k-1 are formed by its backward, after rollout k, with the target network as it
    stands then (synced by apply k-2 at the latest), so the replay recomputes them from the
    rollout's next-state planes with the oracle's target parameters at that point.
    hogwild=True: the engine runs Engine.iterate_hogwild on a one-shard HogwildPS (the clipped
    gradient of rollout k-1 pushed and the shard pulled under rollout k): the same stale-1 replay.
    After iterate() k, slot k-1 -- the buffer the backward just consumed -- is held against the
    independent forward of rollout k-1 (assert_saved_acts), and the engine's loss, head rows and
    gradient against the independent leg (q: q_independent on the late targets; hogwild: the
    clipped independent gradient, the engine's buffer being clipped in place).
    start(eng, ref): called once before the first rollout, on the idle engine.  After every
    iterate() the env state (episode, ep_step, ep_len, lives, frame) equals the oracle's."""
    if algo == 'q':
        kw.setdefault('target_q_update_step', 40)
    eng, ref, ns = build(algo, A, E, n, lives, seed=seed, frames=frames, scale=scale, overlap=True, **kw)
    ps = None
    if hogwild:
        from src.hogwild import HogwildPS
        ps = HogwildPS(eng.params, decay=ref.h['decay'], momentum=ref.h['momentum'], epsilon=ref.h['epsilon'])
    hist = []                  # per rollout: (oracle params used, planes, oracle out)
    worst = {}
    counts = EpisodeCount()
    names = [name for name, _ in ns]
    if start is not None:
        start(eng, ref)
        torch.cuda.synchronize()
    for k in range(rollouts):
        if ps is not None:
            eng.iterate_hogwild(ps)
        else:
            eng.iterate()
        torch.cuda.synchronize()
        sl = eng.slot(k & 1)
        Pk = {kk: v.copy() for kk, v in ref.params.items()}
        # (q: the batch forward + backward wait for the late targets, see q_independent below)
        out = ref.iterate(forced_actions=sl['actions'].cpu().numpy(), grads=algo != 'q')
        planes = rollout_planes(ref, n)
        if algo == 'q':                                 # s_{t+1} of every step, for the late TD target
            out['next_states'] = np.concatenate([ref.states(ref.tau + t + 1) for t in range(n)])
        ref.tau += n                                    # the rollout owns tau in overlap mode
        counts.add(out)
        assert np.array_equal(sl['rewards'].cpu().numpy(), out['rewards']), k
        assert np.array_equal(sl['terminals'].cpu().numpy(), out['terminals']), k
        assert_env_state(eng, ref, k, tau=ref.tau)      # (the row by the oracle's tau: the engine is idle)
        ring = eng.frame_ring.cpu().numpy()            # the rollout's new screens, bit-exact
        for t in range(n):
            tt = ref.tau - n + t + 1
            assert np.array_equal(ring[:, tt % eng.ring_slots], ref.ring[:, tt % ref.R]), (k, t)
        zw = A + 1 if algo == 'a3c' else A
        z_eng = sl['z'].cpu().numpy()[:n].reshape(n, E, -1)
        assert_draws_explained(sl['actions'].cpu().numpy(), out, algo, A, k, z_eng=z_eng)
        assert_z(z_eng, out['z'], zw, k)       # the rollout's head rows vs the independent fp64 forward
        hist.append((Pk, planes, out))
        if k == 0:
            assert not eng.grad_ready
            continue
        Pp, planes_p, out_p = hist[k - 1]
        slp = eng.slot((k - 1) & 1)
        tgt = slp['returns'].cpu().numpy()
        want = out_p['target']
        if algo == 'q':
            qn = Rc.forward(ref.tparams, out_p['next_states'], 'q', keep=False)['z']
            if kw.get('double_q'):     # the argmax of the online net the rollout ran (its q rows)
                qo = Rc.forward(Pp, out_p['next_states'], 'q', keep=False)['z']
                want = Rc.td_target_double(out_p['rewards'].reshape(-1), out_p['terminals'].reshape(-1),
                                           qn.astype(np.float32), qo[:, :A].astype(np.float32),
                                           ref.h['discount']).astype(np.float32).reshape(n, E)
            else:
                want = Rc.td_target(out_p['rewards'].reshape(-1), out_p['terminals'].reshape(-1),
                                    qn.astype(np.float32), ref.h['discount']).astype(np.float32).reshape(n, E)
        np.testing.assert_allclose(tgt, want, rtol=1e-5, atol=1e-5)
        losses, g_same = same_act_grads(slp, planes_p, Pp, algo, A, n, E, tgt, ref.h['beta'], ref.h['literal_adv'])
        assert_losses(eng.loss.cpu().numpy(), losses, algo, k)
        # independent: the oracle's own fp64 batch forward of rollout k-1 (its logits, values and
        # bootstrap targets / q rows), not the engine's saved activations.  q: formed here, with the
        # late targets (the rollout-time oracle targets are not the ones the backward used)
        if algo == 'q':
            ind_losses, z_ind, g_ind, out_p['acts_batch'] = q_independent(Pp, planes_p, out_p['actions'], want)
        else:
            ind_losses, z_ind, g_ind = out_p['losses'], out_p['z_batch'], out_p['grads']
        assert_saved_acts(slp, out_p, n, E, ('saved', k))
        assert_losses(eng.loss.cpu().numpy(), ind_losses, algo, ('independent', k))
        assert_z(slp['z'].cpu().numpy()[:n].reshape(n * E, -1), z_ind, zw, ('z_batch', k))
        G = unflat(eng, ns, eng.grads)
        if ps is not None:     # (hogwild clips the buffer in place before its push)
            g_same_c = {kk: Rc.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g_same.items()}
            g_ind = {kk: Rc.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g_ind.items()}
        for name in names:
            want_g = g_same_c[name] if ps is not None else g_same[name]
            assert rel_l2(G[name], want_g) < 1e-4, (k, name, rel_l2(G[name], want_g))
        assert_independent_grads(G, g_ind, names, k, worst)
        out_p.pop('acts_batch', None)       # (checked; the replay keeps every rollout's out alive)
        lr = ref.apply({kk: Rc.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g_same.items()}, advance_tau=False,
                       tau=out_p['tau'])
        assert_params(eng, ns, ref, k)
        if on_update is not None:
            on_update(k, eng, ref, lr)
        if ps is not None:
            assert torch.equal(ps.gather(), eng.params)
        assert int(eng.counters[1].item()) == ref.global_step
        if algo == 'q':
            T = unflat(eng, ns, eng.target_params)
            for name, _ in ns:
                np.testing.assert_allclose(T[name], ref.tparams[name], rtol=1e-5, atol=1e-6)
    if ps is not None:
        ps.close()
    label = f"overlap{'-hogwild' if hogwild else ''} {algo} A={A} E={E} n={n} {eng.dqn_type}"
    report_independent(label, worst)
    ref.episode_counts = counts.report(label, backprop=rollouts - 1)    # (the last rollout has no backward)
    return eng, ref


def check_hogwild1_vs_oracle(A, E, n, lives, iters=3, seed=91, frames=48, scale=4.0, on_update=None, start=None,
                             **kw):
    """Hogwild with one worker (src/hogwild.py at world 1): rollout + gradient, per-worker clip,
    unlocked RMSProp push into the sharded PS, pull.  With one worker the push order is fixed, so
    it must equal the oracle's clip + RMSProp step for step.
    start(eng, ref): called once before the first rollout."""
    from src.hogwild import HogwildPS
    algo = 'a3c'
    eng, ref, ns = build(algo, A, E, n, lives, seed=seed, frames=frames, scale=scale, **kw)
    ps = HogwildPS(eng.params, decay=ref.h['decay'], momentum=ref.h['momentum'], epsilon=ref.h['epsilon'])
    worst = {}
    counts = EpisodeCount()
    names = [name for name, _ in ns]
    try:
        if start is not None:
            start(eng, ref)
            torch.cuda.synchronize()
        for it in range(iters):
            Pk = unflat(eng, ns, eng.params)
            eng.iterate_hogwild(ps)
            torch.cuda.synchronize()
            acts = eng.actions.cpu().numpy()
            out = ref.iterate(forced_actions=acts)
            counts.add(out)
            planes = rollout_planes(ref, n)
            z_eng = eng.z.cpu().numpy()[:n].reshape(n, E, -1)
            assert_draws_explained(acts, out, algo, A, it, z_eng=z_eng)
            assert_z(z_eng, out['z'], A + 1, it)
            assert_saved_acts(eng, out, n, E, ('saved', it))
            assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards']), it
            assert np.array_equal(eng.terminals.cpu().numpy(), out['terminals']), it
            tgt = eng.returns.cpu().numpy()
            np.testing.assert_allclose(tgt, out['target'], rtol=1e-5, atol=1e-5)
            losses, g_same = same_act_grads(eng, planes, Pk, algo, A, n, E, tgt, ref.h['beta'], ref.h['literal_adv'])
            assert_losses(eng.loss.cpu().numpy(), losses, algo, it)
            assert_losses(eng.loss.cpu().numpy(), out['losses'], algo, ('independent', it))
            clipped = {k: Rc.clip_by_norm(v, ref.h['clip_norm']) for k, v in g_same.items()}
            G = unflat(eng, ns, eng.grads)        # the engine's buffer holds the clipped gradient
            for name in names:
                assert rel_l2(G[name], clipped[name]) < 1e-4, (it, name)
            g_ind = {k: Rc.clip_by_norm(v, ref.h['clip_norm']) for k, v in out['grads'].items()}
            assert_independent_grads(G, g_ind, names, it, worst)
            lr = ref.apply(clipped)
            assert_params(eng, ns, ref, it)
            if on_update is not None:
                on_update(it, eng, ref, lr)
            assert torch.equal(ps.gather(), eng.params)
            cnt = eng.counters.cpu().numpy()
            assert cnt[0] == ref.tau and cnt[1] == ref.global_step
            assert_env_state(eng, ref, it)
    finally:
        ps.close()
    label = f'hogwild-sync a3c A={A} E={E} n={n}'
    report_independent(label, worst)
    ref.episode_counts = counts.report(label)
    return eng, ref
