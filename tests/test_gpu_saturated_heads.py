"""The heads on saturated policies: every softmax, log-softmax, categorical draw and LSTM gate of the
kernels on the inputs of tests/_saturated.py -- peaked rows (top-two gaps to 1e4), common offsets
(+-1000 on the loss, +-3e4 on the draw, +-100 on the engine's policy bias), values and returns to
1e4, gates at 0 and 1 -- against the fp64 oracle.  A head kernel without the max-shift in front of
its expf passes every other test of the suite and fails here (tests/test_saturated_cpu.py shows it
on the CPU, where it also holds every bar below to the float32 oracle at half its width).  Tried
once on an MI355X with the library built without the shift (expf(z) in select_with and k_head_bwd,
log pi = z - logf(s)): test_gpu_action_width, test_gpu_kernels, test_gpu_lstm and test_gpu_gae passed
whole, and of this file every test of parts 1, 2 (categorical) and 4 failed but the play tail at
-100, where expf gives five-bit denormals and no draw of its 9 episodes met the difference.

No bar of an existing test is widened: parts 2 to 4 run under the bars of test_gpu_action_width,
test_gpu_lstm and the engine drivers as they are; part 1 adds a per-row bar on dz, which the
whole-tensor bars cannot see (a saturated row's dz is 1e-7 of its neighbours')."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _saturated as S  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from _engine_parity import (assert_losses, build, check_overlap_vs_oracle, check_sync_vs_oracle,  # noqa: E402
                            rollout_planes, same_act_grads, unflat)
from _net_parity import cu, make_params, rel_l2  # noqa: E402


@pytest.fixture(scope='module')
def K():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


# ------------------------------------------------------------------ 1. loss + head backward, per row
_FORWARDS = {}


def trunk_forward(K, dqn_type, A, algo='a3c'):
    """One real forward of 126 random states per (trunk, algo, A), shared by the cases that replace
    its head rows and fc activations: (net, p, flat, planes, states, fwd)."""
    key = (dqn_type, algo, A)
    if key not in _FORWARDS:
        net = K.NatureNet(A) if dqn_type == 'nature' else K.Net(A, algo)
        p = make_params(net, seed=A + 11, scale=4.0)
        planes = np.random.default_rng(A + 7).integers(0, 256, (S.N_SAMPLES, 4, 84, 84), dtype=np.uint8)
        if dqn_type == 'nature':
            from src.initializers import flatten_host
            flat = cu(flatten_host(net.names_shapes, net.offsets, net.total, p))
        else:
            flat = net.flatten(p)
        states = cu(planes)
        fwd = net.forward(flat, states)
        torch.cuda.synchronize()
        _FORWARDS[key] = (net, p, flat, planes, states, fwd)
    return _FORWARDS[key]


def head_loss_backward(K, dqn_type, algo, A, z, actions, target, literal):
    """The loss + backward entry point on a real forward whose head rows are replaced by z (1e30 in
    the padding columns) and whose fc activations by one-hot rows.  Returns the gradients by name,
    the losses, and the oracle's fp64 (gradients, losses, dz) on the same activations."""
    net, p, flat, planes, states, fwd = trunk_forward(K, dqn_type, A, algo)
    fc = 'l4' if dqn_type == 'nature' else 'l3'
    B, zw = z.shape
    zpad = np.full((B, net.zs), 1e30, np.float32)
    zpad[:, :zw] = z
    h = S.one_hot(B, int(fwd[fc].shape[1]))
    case = dict(fwd)
    case['z'], case[fc] = cu(zpad), cu(h)
    grads, loss = net.loss_backward(flat, states, case, cu(actions), cu(target), beta=S.BETA, literal_adv=literal)
    torch.cuda.synchronize()
    g = grads.cpu().numpy()
    got = {name: g[o:o + n].reshape(shp) for (name, shp), o, n in zip(net.names_shapes, net.offsets, net.sizes)}
    acts = {k: fwd[k].cpu().numpy() for k in fwd if k not in ('z', fc)}
    ref = S.same_act_fwd(dqn_type, planes, acts, z, h)
    return got, loss.cpu().numpy(), S.oracle_loss_backward(p, ref, algo, dqn_type, actions, target, literal)


def assert_whole_tensors(got, lg, g_ref, ref_loss, tag):
    """check_loss_backward's bars on the same activations: 1e-4 relative-L2 per tensor, losses
    within 1e-5 of max(1, |loss|)."""
    for name, v in got.items():
        assert np.isfinite(v).all(), (tag, name)
        err = rel_l2(v, g_ref[name].reshape(v.shape))
        assert err < 1e-4, (tag, name, err)
    assert np.isfinite(lg).all(), (tag, lg)
    for i, r in enumerate(ref_loss):
        assert abs(lg[i] - r) <= 1e-5 * max(1.0, abs(r)), (tag, i, lg[i], r)


HEAD_CASES = [(t, A, pair, False) for t in ('nips', 'nature') for A in (6, 18) for pair in S.VR_PAIRS]
HEAD_CASES += [(t, A, S.LITERAL_PAIR, True) for t in ('nips', 'nature') for A in (6, 18)]


@pytest.mark.parametrize('dqn_type,A,pair,literal', HEAD_CASES)
def test_loss_backward_per_row_on_saturated_rows(K, dqn_type, A, pair, literal):
    """a3c_loss_backward / a3c_nature_loss_backward (k_head_bwd<256> / <512>; A = 6: the rows fit the
    narrow head forms, zs = 8; A = 18: the wide ones, zs = 20) on the 126 samples of
    _saturated.head_case, one (V, R) pair per call.  p_w's row b is sample b's dz, q_w's its dV.

    Per row: max |dz - dz_fp64| over the A logits <= 4 r32 x 2^-24 x max(|R - V|, beta ln A), where
    r32 is the float32 oracle's own worst ratio over these rows (4.29 at A = 6, 1.98 at A = 18) and
    the 4 the margin for the wave-tree summation order and the device's expf / logf.  dV is bit-equal
    to -(R - V); with literal_adv within 4 x 2^-24 max(|adv|, |log pi(a)|) of fp64.

    Measured on an MI355X, the kernels' worst ratio per (V, R) pair, the same on both trunks (they
    share k_head_bwd's row arithmetic), next to r32 and the bar 4 r32:
      pair               (0, 0.5)  (100, 100.25)  (-50, 50)  (1e4, -1e4)  (3, 3)    r32    bar
      A = 6                1.78        1.69          1.69        2.21       0.96    4.29   17.17
      A = 18               1.82        1.82          1.81        1.98       0.14    1.98    7.91
    literal_adv on (-50, 50): the same ratios; dV's worst error 0.35 (A = 6) and 0.32 (A = 18) of its
    bound.  The worst rows are the gap 10 and gap 17 rows and the random N(0, 10) rows."""
    V, Rt = pair
    z, actions, target = S.head_case(A, V, Rt)
    got, lg, (g_ref, ref_loss, dz64) = head_loss_backward(K, dqn_type, 'a3c', A, z, actions, target, literal)
    B = S.N_SAMPLES
    dz, dV = got['p_w'][:B], got['q_w'][:B, 0]
    assert np.isfinite(dz).all() and np.isfinite(dV).all()
    assert not got['p_w'][B:].any() and not got['q_w'][B:].any()
    r32 = S.r32(A)
    ratios = S.row_ratios(dz, dz64, A, V, Rt)
    worst = int(ratios.argmax())
    print(f'saturated head rows {dqn_type} A={A} V={V:g} R={Rt:g} literal={int(literal)}: worst ratio '
          f'{ratios.max():.2f} (sample {worst}, row {worst // 3}) r32 {r32:.2f} bar {4 * r32:.2f}')
    assert (ratios <= 4 * r32).all(), (float(ratios.max()), worst, 4 * r32)
    if literal:
        err = np.abs(dV.astype(np.float64) - dz64[:, A])
        print(f'   dV literal: worst error / bound {float((err / S.dv_bound(z, actions, target)).max()):.2f}')
        assert (err <= S.dv_bound(z, actions, target)).all()
    else:
        assert np.array_equal(dV, -(target - z[:, A]))
    assert_whole_tensors(got, lg, g_ref, ref_loss, (dqn_type, A, pair, literal))


@pytest.mark.parametrize('A', [6, 18])
def test_q_loss_backward_on_large_rows(K, A):
    """The q head of a3c_loss_backward on Q rows and targets to 1e4 through the same one-hot
    construction: check_loss_backward's bars, and per sample dz(a) = -2 (target - Q(a)) / B to three
    roundings (the difference, the fp32 1 / B and the product: 3 x 2^-24 relative, held to 4)."""
    z, actions, target = S.q_case(A)
    got, lg, (g_ref, ref_loss, dz64) = head_loss_backward(K, 'nips', 'q', A, z, actions, target, False)
    B = S.N_SAMPLES
    dz = got['q_w'][:B]
    assert np.isfinite(dz).all() and not got['q_w'][B:].any()
    assert ((dz != 0) == (dz64 != 0)).all()
    err = np.abs(dz - dz64)
    print(f'q head A={A}: worst dz error {float((err / np.maximum(np.abs(dz64), 1e-300)).max() / S.EPS24):.2f} x 2^-24')
    assert (err <= 4 * S.EPS24 * np.abs(dz64)).all()
    assert_whole_tensors(got, lg, g_ref, ref_loss, ('q', A))


# ------------------------------------------------------------------ 2. action draw
@pytest.mark.parametrize('A,stride', S.DRAW_WIDTHS)
def test_select_action_categorical_saturated(K, A, stride):
    """k_select, categorical mode, on rows of spread 2 to 2000 and offsets 0 / +-3e4 (both forms of
    select_with: A <= 8 and A > 8): equal to ref_cpu.sample_categorical away from CDF boundaries
    (the 1e-5 mask, at most 8 of 4096 rows), every action drawn at least B / (8 A) times.  About a
    third of the rows have a top-two gap past 104, where every other expf is exactly 0."""
    zs = stride or (A + 1 + 3) // 4 * 4
    _, z = S.draw_rows(A, zs)
    a_ref, near, _, _ = S.draw_reference(z, A)
    a_gpu = K.select_action(0, cu(z), A, S.DRAW_SEED, S.DRAW_TAU).cpu().numpy()
    print('A', A, 'zs', zs, 'rows near a CDF boundary', int(near.sum()),
          'mismatches among them', int((a_gpu[near] != a_ref[near]).sum()))
    assert near.sum() <= 8
    assert np.array_equal(a_gpu[~near], a_ref[~near])
    assert a_gpu.min() >= 0 and a_gpu.max() < A
    assert np.bincount(a_gpu, minlength=A).min() >= S.DRAW_B / (8 * A)


@pytest.mark.parametrize('A,stride', S.DRAW_WIDTHS)
def test_select_action_eps_greedy_saturated(K, A, stride):
    """k_select, epsilon-greedy mode on the same rows (strides of the q head): exactly equal."""
    zs = stride or (A + 3) // 4 * 4
    rng, z = S.draw_rows(A, zs)
    eps = rng.random(S.DRAW_B).astype(np.float32)
    _, _, u, x = S.draw_reference(z, A)
    a_gpu = K.select_action(1, cu(z), A, S.DRAW_SEED, S.DRAW_TAU, eps=cu(eps)).cpu().numpy()
    a_ref = np.where(u < eps, x[1] % A, np.argmax(z[:, :A], axis=1))
    assert np.array_equal(a_gpu, a_ref)


# ------------------------------------------------------------------ 3. LSTM cell and BPTT
@pytest.mark.parametrize('B', [17, 37])
def test_lstm_step_saturated_gates(K, B):
    """a3c_lstm_step with bias levels +-20 / +-120 and cell states to 1e3: sigmoidf_ through
    expf = inf and expf = 0, tanhf at +-1, under test_gpu_lstm's bars (rtol 1e-5, atol 5e-6 on h, c
    and the gates).  At least 30 % of each gate is exactly 0.0 or +-1.0 in float32, 30 % is not."""
    case = S.lstm_step_case(B)
    w, b, x, h, c, terms = case
    hr, cr, gr = S.lstm_step_oracle(case)
    S.assert_gate_coverage(gr, B)
    out = K.lstm_step(cu(w), cu(b), cu(x), cu(h), cu(c), cu(terms))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ('h', 'c', 'gates'):
        assert np.isfinite(got[k]).all(), k
    print(f"lstm step B={B}: worst |error| h {np.abs(got['h'] - hr).max():.1e} gates {np.abs(got['gates'] - gr).max():.1e} "
          f"c relative {np.abs((got['c'] - cr) / np.maximum(np.abs(cr), 1)).max():.1e}")
    np.testing.assert_allclose(got['h'], hr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(got['c'], cr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(got['gates'], gr, rtol=1e-5, atol=5e-6)
    keep = (1 - terms.astype(np.float32))[:, None]
    assert np.array_equal(got['hp'], h * keep) and np.array_equal(got['cp'], c * keep)
    # the kernel's own gates saturate where the oracle's do
    shares = S.saturated_shares(got['gates'])
    assert min(shares) >= 0.3 and max(shares) <= 0.7, shares


@pytest.mark.parametrize('n,E', [(3, 17), (5, 37)])
def test_lstm_bptt_saturated_gates(K, n, E):
    """a3c_lstm_bptt over a sequence whose gates are 0 / 1 on a third or more of the units and whose
    cell states reach 100: relative-L2 1e-5 on dx, dw, db, and per gate on dw and db."""
    inputs = S.lstm_bptt_inputs(n, E)
    prm, x, seq, terms, dH = inputs
    S.assert_gate_coverage(seq['G'], (n, E))
    dX, dW, dB = S.lstm_bptt_oracle(inputs)
    dx, dw, db = K.lstm_bptt(*[cu(a) for a in (prm['lstm_w'], x, seq['HP'], seq['CP'], seq['G'], seq['C'], terms, dH)])
    torch.cuda.synchronize()
    dx, dw, db = dx.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy()
    assert np.isfinite(dx).all() and np.isfinite(dw).all() and np.isfinite(db).all()
    U = S.U
    errs = [rel_l2(dx, dX), rel_l2(dw, dW), rel_l2(db, dB)]
    gate = [rel_l2(dw[:, g * U:(g + 1) * U], dW[:, g * U:(g + 1) * U]) for g in range(4)]
    gate += [rel_l2(db[g * U:(g + 1) * U], dB[g * U:(g + 1) * U]) for g in range(4)]
    print(f'lstm bptt saturated n={n} E={E}: dx {errs[0]:.1e} dw {errs[1]:.1e} db {errs[2]:.1e} per gate max '
          f'{max(gate):.1e}')
    assert max(errs) < 1e-5, errs
    assert max(gate) < 1e-5, gate


# ------------------------------------------------------------------ 4. the fused head kernels
def assert_logits_past_88(seen, rollouts, tag):
    print(tag, 'min |logit| per rollout', ' '.join(f'{v:.1f}' for v in seen))
    assert len(seen) == rollouts and min(seen) > 88, (tag, seen)


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_engine_sync_shifted_logits(shift):
    """k_head_screen* (narrow head_row and select_with) and k_head_bwd with fused returns, every
    logit near +-100: all bars of check_sync_vs_oracle."""
    seen = []
    check_sync_vs_oracle('a3c', 6, 8, 5, 3, iters=3, seed=131, params=S.shifted_params(131, 4.0, shift),
                         start=S.logit_recorder(6, seen))
    assert_logits_past_88(seen, 3, ('sync', shift))


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_engine_overlap_shifted_logits_wide(shift):
    """The overlapped pipeline at A = 18: k_head_screen_conv12 and the bootstrap head with the wide
    head_row and select_with, k_head_bwd<256> on rows of stride 20: all bars of
    check_overlap_vs_oracle."""
    seen = []
    check_overlap_vs_oracle(18, 8, 3, 0, rollouts=4, seed=79, learning_rate=3e-3,
                            params=S.shifted_params(79, 4.0, shift), start=S.logit_recorder(18, seen))
    assert_logits_past_88(seen, 4, ('overlap', shift))


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_engine_overlap_gae_shifted_logits_wide(shift):
    """k_head_bwd's GAE form at A = 18, gae_lambda = 0.95, overlapped.  The replay oracle forms
    n-step returns only, so this is test_gpu_gae's check instead of check_overlap_vs_oracle: every
    back-propagated rollout's returns against gae_ref on the slot's own rewards, terminals and V
    rows (1e-5 of max(1, |G|)), its losses against the oracle's on the slot's head rows at those
    returns (1e-4), and the first backward's gradient against the oracle backward on the slot's
    saved activations (1e-4 relative-L2)."""
    from test_gae_cpu import gae_ref
    from test_gpu_gae import GAMMA, assert_returns
    A, E, n, seed, lam = 18, 8, 3, 79, 0.95
    eng, ref, ns = build('a3c', A, E, n, 5, seed=seed, overlap=True, gae_lambda=lam,
                         params=S.shifted_params(seed, 4.0, shift))
    assert abs(eng.cfg.gae_lambda - lam) < 1e-7 and eng.zs == 20
    seen = []
    S.logit_recorder(A, seen)(eng, ref)
    P0 = unflat(eng, ns, eng.params)
    P0 = {k: v.copy() for k, v in P0.items()}
    planes = {}
    for k in range(4):
        eng.iterate()
        torch.cuda.synchronize()
        sl = eng.slot(k & 1)
        out = ref.iterate(forced_actions=sl['actions'].cpu().numpy(), grads=False)     # the env's replay
        planes[k] = rollout_planes(ref, n)
        ref.tau += n
        assert np.array_equal(sl['rewards'].cpu().numpy(), out['rewards']), k
        assert np.array_equal(sl['terminals'].cpu().numpy(), out['terminals']), k
        if k == 0:
            continue
        slp = eng.slot((k - 1) & 1)
        z = slp['z'].cpu().numpy()
        assert np.isfinite(z[..., :A + 1]).all() and np.abs(z[..., :A]).min() > 88
        G_ref, _ = gae_ref(slp['rewards'].cpu().numpy(), slp['terminals'].cpu().numpy(), z[:n, :, A], z[n, :, A],
                           GAMMA, lam)
        assert_returns(slp['returns'].cpu().numpy(), G_ref, ('returns', shift, k))
        R1 = R.nstep_returns(slp['rewards'].cpu().numpy(), slp['terminals'].cpu().numpy(), z[n, :, A], GAMMA)
        assert np.abs(G_ref - R1).max() > 1e-3, k            # not the lambda = 1 path
        G32 = G_ref.astype(np.float32)
        losses, _ = R.a3c_loss_and_dz(z[:n].reshape(n * E, -1)[:, :A + 1].astype(np.float64),
                                      slp['actions'].cpu().numpy().reshape(-1), G32.reshape(-1).astype(np.float64), 0.01)
        loss = eng.loss.cpu().numpy()
        assert np.isfinite(loss).all()
        assert_losses(loss, losses, 'a3c', ('loss', shift, k))
        if k == 1:      # rollout 0 ran and is back-propagated on the initial parameters
            _, g_same = same_act_grads(slp, planes[0], P0, 'a3c', A, n, E, G32)
            G = unflat(eng, ns, eng.grads)
            for name, _ in ns:
                r = rel_l2(G[name], g_same[name])
                assert r < 1e-4, (shift, name, r)
    assert_logits_past_88(seen, 4, ('overlap gae (initial parameters)', shift))


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_engine_lstm_shifted_logits(shift):
    """The LSTM head's rollout head and k_head_bwd's LSTM form (relu = 0): all bars of
    check_lstm_sync_vs_oracle."""
    from test_gpu_lstm import check_lstm_sync_vs_oracle
    seen = []
    check_lstm_sync_vs_oracle(6, 8, 5, 3, iters=3, seed=308, learning_rate=2e-3,
                              params=S.shifted_params(308, 4.0, shift), start=S.logit_recorder(6, seen))
    assert_logits_past_88(seen, 3, ('lstm', shift))


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_engine_nature_shifted_logits(shift):
    """k_nat_head and k_head_bwd<512>: all bars of check_sync_vs_oracle on the nature trunk."""
    seen = []
    check_sync_vs_oracle('a3c', 6, 8, 3, 0, iters=3, seed=508, frames=48, scale=2.0, learning_rate=2e-3,
                         dqn_type='nature', params=S.shifted_params(508, 2.0, shift), start=S.logit_recorder(6, seen))
    assert_logits_past_88(seen, 3, ('nature', shift))


@pytest.mark.parametrize('shift', S.SHIFTS)
def test_play_shifted_logits(shift):
    """The play tail's head and draw: every check of test_gpu_play.check_play."""
    from _play_ref import ref_like
    from test_gpu_play import check_play
    eng, ref, _ = build('a3c', 6, 6, 5, lives=0, seed=46, params=S.shifted_params(46, 4.0, shift))
    out, r = check_play(eng, ref_like(ref), 9, 16, tag=('play', shift))
    assert np.abs(r['z'][r['live']][:, :6]).min() > 88
