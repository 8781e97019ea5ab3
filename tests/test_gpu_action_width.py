"""Action sets wider than 8: the other side of every fork the head code takes on action_size.

The C-ABI accepts action_size 1..31; the synthetic games have 4 and 6, real Atari sets have up to
18.  The head code forks on that value (csrc/net_head.h), and the row stride of everything that
reads a head row is zs = round_up(A + 1 (a3c) or A (q), 4).  The widths below are the smallest that
reach each distinct path:

  algo  A   nout  zs   reaches
  a3c   3   4     4    narrow head_row and select_with, no padding column
  a3c   7   8     8    narrow head_row completely full (8 outputs in 8 lane slots), no padding
  a3c   8   9     12   the mixed case: wide head_row (nout > 8) with the narrow select_with (A <= 8)
  q     8   8     8    narrow both, no padding
  q     9   9     12   wide both: the first wide q
  both  18  19/18 20   the full Atari set; zs not a multiple of 8
  both  31  32/31 32   the ABI's maximum; a3c has no padding column
  q     1   1     4    degenerate: x.y % 1, argmax over one (forward, select, td_target only)

Same bars as the narrow widths everywhere (tests/_net_parity.py, tests/_engine_parity.py): none is
widened here.  Where zs > A(+1) the padding columns must be exactly 0; where zs == A(+1) a row of
sentinels after the last head row must survive (a value written one lane off lands there)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import philox as px  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from _engine_parity import check_overlap_vs_oracle, check_sync_vs_oracle  # noqa: E402
from _net_parity import (GUARD, check_forward, check_loss_backward, close, cu, guarded_z,  # noqa: E402
                         make_params, rel_l2)


@pytest.fixture(scope='module')
def K():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


def a3c_zs(algo, A):
    return ((A + 1 if algo == 'a3c' else A) + 3) // 4 * 4


# ------------------------------------------------------------------ 1. NIPS forward, loss + backward
@pytest.mark.parametrize('algo,A,B', [('a3c', 3, 5), ('a3c', 7, 5), ('a3c', 8, 5), ('q', 8, 5), ('q', 9, 5),
                                      ('a3c', 18, 5), ('q', 18, 5), ('a3c', 31, 5), ('q', 31, 5), ('q', 1, 5),
                                      ('a3c', 18, 37), ('q', 18, 37)])
def test_forward_matches_oracle_wide(K, algo, A, B):
    """Net.forward (k_head of net_fwd.hip).  nout > 8 runs head_row's W == FC (256) wave-sum loop,
    whose value head is written by lane A; nout <= 8 the lane-packed form (a3c 7: all 8 slots
    taken).  z columns past A(+1) are exactly 0 for zs in {12, 20}; with no padding column (a3c 3,
    7, 31; q 8) the sentinel row after row B - 1 survives.  B = 5 is one row past a
    4-rows-per-workgroup block, B = 37 ten blocks with a ragged last one."""
    assert K.Net(A, algo).zs == a3c_zs(algo, A)
    check_forward(K, algo, A, B)


# B = 17 is the smallest batch the head weight GEMM splits: a3c_gemm_plan_split(FC, zs, B, 128) is
# min(128 / tiles, ktiles, 32) with tiles = ceil(256 / 64) * ceil(zs / 64) = 4 and ktiles =
# ceil(B / BK), BK = 16 (gemm.hip), so it exceeds 1 from B = 17 on
@pytest.mark.parametrize('algo,A,B,literal', [('a3c', 7, 7, False), ('a3c', 8, 7, False), ('a3c', 18, 7, False),
                                              ('a3c', 31, 7, False), ('q', 8, 7, False), ('q', 9, 7, False),
                                              ('q', 18, 7, False), ('q', 31, 7, False), ('a3c', 18, 17, False),
                                              ('q', 18, 17, False), ('a3c', 18, 7, True)])
def test_loss_backward_matches_oracle_wide(K, algo, A, B, literal):
    """Net.loss_backward at zs in {8, 12, 20, 32}: k_head_bwd<256> (dz rows of stride zs, dl3 over A
    columns of the head weights), the head weight-gradient GEMM with N = ldb = zs (unsplit at B = 7;
    at B = 17 two K slabs folded by the k_finalize segments), and the finalize segments that carve
    the [FC][zs] product into p_w [FC][A] and q_w [FC][1] at column A.  The 64-float gaps between
    the tensors of the gradient buffer keep their sentinel."""
    check_loss_backward(K, algo, A, B, literal)


# ------------------------------------------------------------------ 2. nature trunk, per-op
def nature_case(K, A, B, literal, beta=0.01):
    from src.initializers import flatten_host
    net = K.NatureNet(A)
    p = make_params(net, seed=A + B, scale=4.0)
    rng = np.random.default_rng(100 + A + B)
    planes = rng.integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)
    actions = rng.integers(0, A, B).astype(np.int32)
    target = rng.standard_normal(B).astype(np.float32)
    flat = cu(flatten_host(net.names_shapes, net.offsets, net.total, p))
    states = cu(planes)
    zbuf = guarded_z(B, net.zs)
    fwd = net.forward(flat, states, z=zbuf)
    grads, loss = net.loss_backward(flat, states, fwd, cu(actions), cu(target), beta=beta, literal_adv=literal)
    return net, p, planes, actions, target, zbuf, fwd, grads, loss


@pytest.mark.parametrize('A,B,literal', [(18, 5, False), (7, 3, False), (8, 1, True), (31, 37, False)])
def test_nature_forward_loss_backward_match_oracle(K, A, B, literal):
    """kernels.NatureNet.forward / loss_backward called directly against ref_cpu.forward / backward
    with dqn_type='nature'.  nout > 8 (A = 8, 18, 31) runs head_row's W == 512 wave-sum loop in
    k_nat_head, A = 7 its two-pass lane-packed form; then k_head_bwd<512>, the head weight GEMM with
    N = ldb = zs in {8, 12, 20, 32} and the finalize segments at column A (nature.hip).  B = 37
    gives the three dW passes a ragged last K chunk and the head GEMM more than one K tile (split);
    A = 8 at B = 1 is the mixed wide head_row / narrow select width with literal_adv."""
    check_nature_forward_loss_backward(K, A, B, literal)


def check_nature_forward_loss_backward(K, A, B, literal, beta=0.01):
    net, p, planes, actions, target, zbuf, fwd, grads, loss = nature_case(K, A, B, literal, beta)
    zw = A + 1
    assert net.zs == a3c_zs('a3c', A)
    states = R.states_nhwc(planes)
    ref = R.forward(p, states, 'a3c', 'nature', dtype=np.float64)
    z = fwd['z'].cpu().numpy()
    close(z[:, :zw], ref['z'])
    assert not z[:, zw:].any()
    assert np.array_equal(zbuf[B].cpu().numpy(), np.full(net.zs, GUARD, np.float32))
    close(fwd['l1'].cpu().numpy().reshape(B, 20, 20, 32), ref['acts'][1])
    close(fwd['l2'].cpu().numpy().reshape(B, 9, 9, 64), ref['acts'][2])
    close(fwd['l3'].cpu().numpy(), ref['flat'])
    close(fwd['l4'].cpu().numpy(), ref['h3'])
    g = grads.cpu().numpy()
    lg = loss.cpu().numpy()

    def check(ref_f, gtol, ltol):
        losses, dz = R.a3c_loss_and_dz(ref_f['z'], actions, target.astype(np.float64), beta, literal)
        g_ref = R.backward(p, ref_f, dz, 'a3c', 'nature')
        for (name, shp), o, n in zip(net.names_shapes, net.offsets, net.sizes):
            err = rel_l2(g[o:o + n].reshape(shp), g_ref[name].reshape(shp))
            assert err < gtol, (name, err)
        for i, key in enumerate(('policy', 'value', 'entropy', 'total')):
            assert abs(lg[i] - losses[key]) <= ltol * max(1.0, abs(losses[key])), (key, lg[i], losses[key])

    # the oracle backward on the kernels' own activations (the same ReLU masks): 1e-4, losses 1e-5
    fa = {k: v.cpu().numpy().astype(np.float64) for k, v in fwd.items()}
    same = dict(z=fa['z'][:, :zw], h3=fa['l4'], flat=fa['l3'],
                acts=[states.astype(np.float64) / 255.0, fa['l1'].reshape(B, 20, 20, 32),
                      fa['l2'].reshape(B, 9, 9, 64), fa['l3'].reshape(B, 7, 7, 64)])
    check(same, 1e-4, 1e-5)
    # the fully independent fp64 forward + backward (ReLU flips allowed): 2e-2, losses 1e-4
    check(ref, 2e-2, 1e-4)


# ------------------------------------------------------------------ 3. select_action, td_target
def select_rows(A, B, zs):
    """Head rows [B, zs]: logits of spread 2 in the first A columns, +1e30 in every other one (the
    a3c value column and the padding), so a read past A cannot go unseen."""
    rng = np.random.default_rng(3 + A)
    z = np.full((B, zs), 1e30, np.float32)
    z[:, :A] = rng.standard_normal((B, A)).astype(np.float32) * 2
    return rng, z


SELECT_WIDTHS = [(1, None), (7, None), (8, None), (9, None), (18, None), (31, None), (18, 32)]


@pytest.mark.parametrize('A,stride', SELECT_WIDTHS)
def test_select_action_categorical_wide(K, A, stride):
    """k_select, categorical mode: A <= 8 the v_readlane form of select_with, A > 8 its general
    wave_max / wave_sum / __shfl form with the j < A bound on the sequential CDF.  Equal to
    ref_cpu.sample_categorical away from CDF boundaries (the 1e-5 mask, at most 8 of 4096 rows);
    every action drawn at least B / (8 A) times.  Stride a3c_zs, and A = 18 at stride 32."""
    B, seed, tau = 4096, 123, 77
    zs = stride or a3c_zs('a3c', A)
    _, z = select_rows(A, B, zs)
    x = px.philox4x32(tau, 0, np.arange(B, dtype=np.uint32), px.P_ACTION, *px.seed_key(seed))
    a_gpu = K.select_action(0, cu(z), A, seed, tau).cpu().numpy()
    pi, _, _ = R.softmax_stats(z[:, :A].astype(np.float64))
    u = px.u01(x[0])
    a_ref = R.sample_categorical(pi.astype(np.float32), u)
    near = np.min(np.abs(np.cumsum(pi, axis=1) - u[:, None].astype(np.float64)), axis=1) < 1e-5
    print('A', A, 'zs', zs, 'rows near a CDF boundary', int(near.sum()),
          'mismatches among them', int((a_gpu[near] != a_ref[near]).sum()))
    assert near.sum() <= 8
    assert np.array_equal(a_gpu[~near], a_ref[~near])
    assert a_gpu.min() >= 0 and a_gpu.max() < A
    assert np.bincount(a_gpu, minlength=A).min() >= B / (8 * A)


@pytest.mark.parametrize('A,stride', SELECT_WIDTHS)
def test_select_action_eps_greedy_wide(K, A, stride):
    """k_select, epsilon-greedy mode: the narrow (A <= 8) and the general (__shfl loop, j < A)
    argmax of select_with and the random branch x.y % A (A = 1: always 0), exactly equal."""
    B, seed, tau = 4096, 123, 77
    zs = stride or a3c_zs('q', A)
    rng, z = select_rows(A, B, zs)
    eps = rng.random(B).astype(np.float32)
    x = px.philox4x32(tau, 0, np.arange(B, dtype=np.uint32), px.P_ACTION, *px.seed_key(seed))
    a_gpu = K.select_action(1, cu(z), A, seed, tau, eps=cu(eps)).cpu().numpy()
    a_ref = np.where(px.u01(x[0]) < eps, x[1] % A, np.argmax(z[:, :A], axis=1))
    assert np.array_equal(a_gpu, a_ref)


@pytest.mark.parametrize('A', [8, 9, 18, 31])
def test_select_action_greedy_ties_take_the_first(K, A):
    """Rows whose maximum occurs twice, at every index pair i < j (so 7 and 8, the edge of the
    narrow form's 8 lanes, and 0 and A - 1): tf.argmax / np.argmax return the first."""
    pairs = [(i, j) for i in range(A) for j in range(i + 1, A)]
    B = len(pairs)
    zs = a3c_zs('q', A)
    rng = np.random.default_rng(A)
    z = np.full((B, zs), 1e30, np.float32)
    z[:, :A] = -rng.random((B, A)).astype(np.float32)
    for r, (i, j) in enumerate(pairs):
        z[r, i] = z[r, j] = 1.0
    assert np.array_equal(np.argmax(z[:, :A], axis=1), [i for i, _ in pairs])
    a_gpu = K.select_action(1, cu(z), A, 5, 9, eps=cu(np.zeros(B, np.float32))).cpu().numpy()
    assert np.array_equal(a_gpu, np.argmax(z[:, :A], axis=1))


@pytest.mark.parametrize('A,zs', [(18, 20), (9, 12), (1, 4)])
def test_td_target_bit_exact_wide(K, A, zs):
    """k_td_target (no qsel) over rows of stride zs in {20, 12, 4} with +1e30 in the padding columns:
    the max runs over the first A columns only; bit-exact against ref_cpu.td_target."""
    rng = np.random.default_rng(40 + A)
    B = 1500
    rew = rng.choice(np.array([-1, 0, 0, 0, 1], np.float32), B)
    term = (rng.random(B) < 0.2).astype(np.uint8)
    qn = np.full((B, zs), 1e30, np.float32)
    qn[:, :A] = rng.standard_normal((B, A)).astype(np.float32)
    got = K.td_target(cu(rew), cu(term), cu(qn), A).cpu().numpy()
    assert np.array_equal(got, R.td_target(rew, term, qn[:, :A], 0.99).astype(np.float32))


# ------------------------------------------------------------------ 4. engine parity
@pytest.mark.parametrize('algo,A,E,n,lives,kw', [
    ('a3c', 18, 6, 3, 3, {}), ('a3c', 8, 5, 3, 0, {}), ('a3c', 7, 5, 3, 0, {}), ('q', 18, 5, 4, 3, {}),
    ('q', 9, 5, 4, 3, {}), ('a3c', 18, 6, 3, 3, dict(frame84=1)), ('q', 18, 5, 4, 3, dict(double_q=1))],
    ids=['a3c-18', 'a3c-8', 'a3c-7', 'q-18', 'q-9', 'a3c-18-frame84', 'q-18-double_q'])
def test_engine_sync_matches_oracle_wide(algo, A, E, n, lives, kw):
    """The synchronous engine against the replay oracle (every bar of check_sync_vs_oracle): the
    fused rollout heads k_head_screen* draw with the wide head_row (W = 256) and, for A > 8, the
    wide select_with (a3c: categorical, q: epsilon-greedy); a3c 8 is the mixed wide head_row /
    narrow select_with case, a3c 7 the full narrow form.  The backward reads z, dz and the head
    GEMM at zs in {8, 12, 20}; q forms its TD target from target-net rows of stride zs (double_q:
    k_td_target with qsel, the online net's argmax over 18 columns of stride 20)."""
    check_sync_vs_oracle(algo, A, E, n, lives, **kw)


@pytest.mark.parametrize('algo,kw', [('a3c', {}), ('q', dict(target_q_update_step=100)),
                                     ('q', dict(target_q_update_step=100, double_q=1))],
                         ids=['a3c', 'q', 'q-double_q'])
def test_engine_overlap_matches_oracle_wide(algo, kw):
    """The overlapped (stale-1) pipeline at A = 18, zs = 20: k_head_screen_conv12 and the bootstrap
    head fold draw and write rows of stride 20 (wide head_row at W = 256, wide select_with); q forms
    the late TD target from stride-20 rows (double_q: with qsel)."""
    check_overlap_vs_oracle(18, 8, 3, 0, rollouts=4, seed=79, learning_rate=3e-3, algo=algo, **kw)


def test_engine_nature_sync_matches_oracle_wide():
    """The nature trunk's engine at A = 18: k_nat_head with the wide head_row at W = 512 and the wide
    categorical select_with, k_head_bwd<512>, the head GEMM and finalize segments at zs = 20."""
    check_sync_vs_oracle('a3c', 18, 8, 3, 0, iters=2, seed=508, frames=48, scale=2.0, learning_rate=2e-3,
                         dqn_type='nature')
