"""The engine parity checkers (tests/_engine_parity.py) proven sharp on the CPU.

The checkers take any mapping of CPU tensors as a "slot", so a slot is built here from the oracle's
own fp64 forward rounded to float32 (E = 8, n = 5, nips trunk, A = 6, init stddev 0.08), and the
"engine's" gradient is the oracle backward on that slot -- what an engine that back-propagates its
saved buffers computes.  Then the slot is corrupted the way the overlap pipeline could corrupt it
(a stale or misplaced sample: one sample's act_l1/2/3 replaced by its neighbour's) and each leg is
asked whether it notices:
  * assert_saved_acts raises for every one of the 40 samples, and for a single element off by 1e-2;
  * the 2e-2 independent gradient check alone does not see the least-advantage sample -- the blind
    spot assert_saved_acts closes;
  * q: a loss formed with the rollout-time TD targets instead of the late ones fails the
    independent loss assertion once the target network has changed in between.
No GPU, no engine: buffer corruption lives only here, on copies."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import ref_cpu as Rc  # noqa: E402
from oracle.engine_ref import EngineRef  # noqa: E402
from _engine_parity import (assert_independent_grads, assert_losses, assert_saved_acts, assert_z,  # noqa: E402
                            q_independent, rel_l2, rollout_planes, same_act_grads)

A, E, N = 6, 8, 5
B = N * E
TRUNK = ('act_l1', 'act_l2', 'act_l3')


def _rollout(algo):
    """One oracle rollout with its own draws: (ref, parameters it ran with, out, planes)."""
    p = Rc.init_params(Rc.param_shapes(A, algo), seed=131, stddev=0.08)
    ref = EngineRef(p, E, N, A, algo, 0, 48, 131, learning_rate=3e-3, target_q_update_step=N * E)
    ref.reset()
    P = {k: v.copy() for k, v in ref.params.items()}
    out = ref.iterate()
    return ref, P, out, rollout_planes(ref, N)


@pytest.fixture(scope='module')
def a3c():
    return _rollout('a3c')


@pytest.fixture(scope='module')
def q():
    ref, P, out, planes = _rollout('q')
    nxt = np.concatenate([ref.states(ref.tau + t + 1) for t in range(N)])
    # an update with a target sync between the rollout and its backward (the overlap pipeline's
    # order): the late targets come from the target network as it stands now
    t_before = {k: v.copy() for k, v in ref.tparams.items()}
    ref.apply(out['clipped'])
    assert max(np.abs(ref.tparams[k] - t_before[k]).max() for k in t_before) > 1e-3
    qn = Rc.forward(ref.tparams, nxt, 'q', keep=False)['z']
    want = Rc.td_target(out['rewards'].reshape(-1), out['terminals'].reshape(-1), qn.astype(np.float32),
                        ref.h['discount']).astype(np.float32).reshape(N, E)
    return ref, P, out, planes, want


def _slot(out, algo):
    """The oracle's independent forward as an engine slot: float32 CPU tensors, engine layouts."""
    ab = out['acts_batch']
    zw = A + 1 if algo == 'a3c' else A
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy())  # noqa: E731
    return dict(act_l1=f(ab['l1'].reshape(B, -1)), act_l2=f(ab['l2'].reshape(B, -1)), act_l3=f(ab['h3']),
                z=f(out['z_batch'].reshape(N, E, zw)), actions=torch.from_numpy(out['actions'].copy()))


def _with_stale_sample(slot, b):
    """Sample b's saved trunk activations replaced by its neighbour's (z and actions untouched)."""
    s = {k: v.clone() for k, v in slot.items()}
    for k in TRUNK:
        s[k][b] = slot[k][(b + 1) % B]
    return s


def test_slot_layout_is_the_engines(a3c):
    _, _, out, _ = a3c
    s = _slot(out, 'a3c')
    assert s['act_l1'].shape == (B, 6400) and s['act_l2'].shape == (B, 2592) and s['act_l3'].shape == (B, 256)
    assert 'x0' not in out and all(v.dtype == np.float32 for v in out['acts_batch'].values())
    assert sorted(out['acts_batch']) == ['h3', 'l1', 'l2']


@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_clean_slot_passes_every_leg(algo, a3c, q):
    ref, P, out, planes = (a3c if algo == 'a3c' else q)[:4]
    s = _slot(out, algo)
    assert_saved_acts(s, out, N, E, 'clean')
    losses, G = same_act_grads(s, planes, P, algo, A, N, E, out['target'])
    keys = ('policy', 'value', 'entropy', 'total') if algo == 'a3c' else ('loss',)
    assert_losses([losses[k] for k in keys], out['losses'], algo, 'clean')
    for name in G:      # float32 rounding of the activations only
        assert rel_l2(G[name], out['grads'][name]) < 1e-4, name
    assert_independent_grads(G, out['grads'], list(G), 'clean')


@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_saved_acts_catches_every_stale_sample(algo, a3c, q):
    out = (a3c if algo == 'a3c' else q)[2]
    s = _slot(out, algo)
    for b in range(B):
        with pytest.raises(AssertionError):
            assert_saved_acts(_with_stale_sample(s, b), out, N, E, ('stale', b))
    # each layer on its own
    for k in TRUNK:
        one = {kk: v.clone() for kk, v in s.items()}
        one[k][17] = s[k][18]
        with pytest.raises(AssertionError, match=k):
            assert_saved_acts(one, out, N, E, ('stale', k))


def test_stale_sample_misses_the_bound_by_orders_of_magnitude(a3c):
    """The stale sample's l1 is off by a third of the layer's largest value: > 1e3 times the bound."""
    out = a3c[2]
    l1 = out['acts_batch']['l1'].reshape(B, -1)
    atol = 1e-4 * max(1.0, float(np.abs(l1).max()))
    off = [float(np.abs(l1[b] - l1[(b + 1) % B]).max()) for b in range(B)]
    assert min(off) > 1e3 * atol, (min(off), atol)


def test_gradient_bound_alone_is_blind_to_a_stale_sample(a3c):
    """a3c: a sample enters every gradient tensor in proportion to its dz, i.e. to its advantage
    R - V (plus the small entropy term), and the gradient sums B = 40 of them.  The stale sample of
    least |R - V| therefore moves no tensor by 2e-2: the independent gradient check passes a slot
    that holds another sample's activations.  This is the blind spot assert_saved_acts closes;
    (the same-activation leg believes the slot by construction)."""
    ref, P, out, planes = a3c
    s = _slot(out, 'a3c')
    adv = np.abs(out['target'].reshape(-1).astype(np.float64) - out['z_batch'][:, A])
    b = int(np.argmin(adv))
    stale = _with_stale_sample(s, b)
    _, G = same_act_grads(stale, planes, P, 'a3c', A, N, E, out['target'])
    worst = {}
    assert_independent_grads(G, out['grads'], list(G), ('stale', b), worst)       # does not raise
    # ... although the gradient did change, by more than the 1e-4 of the same-activation leg
    assert 1e-4 < max(worst.values()) < 2e-2, worst
    with pytest.raises(AssertionError):
        assert_saved_acts(stale, out, N, E, ('stale', b))
    # a sample of large advantage does show in the gradient: the bound is not vacuous
    big = _with_stale_sample(s, int(np.argmax(adv)))
    _, G = same_act_grads(big, planes, P, 'a3c', A, N, E, out['target'])
    with pytest.raises(AssertionError):
        assert_independent_grads(G, out['grads'], list(G), 'stale-big')


def test_saved_acts_catches_one_element(a3c):
    out = a3c[2]
    s = _slot(out, 'a3c')
    s['act_l2'][23, 1000] += 1e-2
    with pytest.raises(AssertionError, match='act_l2'):
        assert_saved_acts(s, out, N, E, 'element')


def test_q_rollout_time_targets_fail_the_independent_leg(q):
    """Overlap Q-learning forms its TD targets late.  An engine that used the rollout-time targets
    (the target network before the sync) is caught by the independent loss on the late ones."""
    ref, P, out, planes, want = q
    s = _slot(out, 'q')
    ind_losses, z_ind, g_ind, ab = q_independent(P, planes, out['actions'], want)
    assert_saved_acts(s, dict(acts_batch=ab), N, E, 'q late')
    assert_z(s['z'].numpy().reshape(B, -1), z_ind, A, 'q late')
    late, G = same_act_grads(s, planes, P, 'q', A, N, E, want)
    assert_losses([late['loss']], ind_losses, 'q', 'late')
    assert_independent_grads(G, g_ind, list(G), 'late')
    early, G = same_act_grads(s, planes, P, 'q', A, N, E, out['target'])
    with pytest.raises(AssertionError):
        assert_losses([early['loss']], ind_losses, 'q', 'rollout-time')
    with pytest.raises(AssertionError):
        assert_independent_grads(G, g_ind, list(G), 'rollout-time')
