"""The saturated-policy inputs of tests/_saturated.py, the part that needs no GPU: every bar the GPU
tests (tests/test_gpu_saturated_heads.py) hold the kernels to is applied here to the oracle
evaluated in float32 against itself in float64, which must stay inside half of it; the inputs are
shown to reach the regimes they are for (coverage counts); and an fp32 softmax without the
max-shift is shown to fail on them, so a kernel that dropped the shift could not pass."""
import numpy as np
import pytest

import _saturated as S
from _net_parity import rel_l2
from oracle import ref_cpu as R


# ------------------------------------------------------------------ 1. loss + head backward
def test_head_rows_are_the_ones_described():
    rows = S.logit_rows(6)
    assert rows.shape == (42, 6)
    gaps = S.top_gap(rows, 6)
    # per offset: flat, eight gaps, a tie
    for k, off in enumerate(S.OFFSETS):
        blk = rows[10 * k:10 * k + 10]
        assert (blk[0] == np.float32(off)).all()
        assert (blk[1:9].argmax(1) == 1).all()
        assert blk[9, 0] == blk[9, 5] == np.float32(off + 50) and gaps[10 * k + 9] == 0
    # the gaps survive the offsets in float32 (1e-3 to the ulp of 1000)
    np.testing.assert_allclose(gaps[1:9], S.GAPS, rtol=2.0 ** -24, atol=0)
    np.testing.assert_allclose(gaps[11:19], S.GAPS, rtol=0, atol=2.0 ** -14)
    z, actions, target = S.head_case(6, 100.0, 100.25)
    assert z.shape == (126, 7) and (z[:, 6] == 100).all() and (target == 100.25).all()
    assert np.array_equal(actions[3:6], [1, 0, 2])           # argmax, argmin (the first), action 2


@pytest.mark.parametrize('A', [6, 18])
def test_head_rows_reach_the_fp32_edges(A):
    """1 - pi(argmax) is down to the last bits of 1.0f at gap 17 and gone from 30 on, expf(-gap) is
    denormal at 90 and exactly 0 from 104 on, and the argmin rows keep a gradient of the advantage's
    size."""
    z, actions, target = S.head_case(A, -50.0, 50.0)
    rows = z[0::3, :A]
    gap = S.top_gap(rows, A)[1:9]
    e = np.exp(-gap.astype(np.float32))
    pi1 = R.softmax_stats(rows[1:9].astype(np.float64))[0][:, 1].astype(np.float32)
    assert 0 < 1 - pi1[2] <= (A - 1) * 2.0 ** -24      # gap 17: 1 - pi is an ulp or two of 1, pure cancellation
    assert list(pi1 == 1.0) == [g >= 30 for g in S.GAPS]
    assert 0 < e[4] < np.finfo(np.float32).tiny and e[4] == np.exp(np.float32(-90.0))
    assert list(e == 0) == [g >= 104 for g in S.GAPS]
    _, dz = S.loss_dz(z, actions, target, False, np.float64)
    assert (np.abs(dz[1::3, :A]).max(axis=1) > 0.5 * 100).all()     # argmin-action samples: O(|adv|)


@pytest.mark.parametrize('A', [6, 18])
def test_head_row_bar_holds_the_fp32_oracle(A):
    """r32, the float32 oracle's worst row ratio, from which the kernels' bar 4 r32 is formed: a few
    roundings of the row's scale, on every pair (so the bar is an fp32-class bar, not a loose one)."""
    r32 = S.r32(A)
    print(f'A={A} r32 {r32:.2f}')
    assert 1.0 <= r32 <= 8.0
    for V, Rt in S.VR_PAIRS:
        z, actions, target = S.head_case(A, V, Rt)
        for literal in ((False, True) if (V, Rt) == S.LITERAL_PAIR else (False,)):
            _, dz64 = S.loss_dz(z, actions, target, literal, np.float64)
            _, dz32 = S.loss_dz(z, actions, target, literal, np.float32)
            assert np.isfinite(dz32).all()
            assert S.row_ratios(dz32, dz64, A, V, Rt).max() <= 0.5 * 4 * r32
            if literal:
                assert (np.abs(dz32[:, A] - dz64[:, A]) <= 0.5 * S.dv_bound(z, actions, target)).all()
            else:
                assert np.array_equal(dz32[:, A], -(target - z[:, A]))


def test_unshifted_softmax_fails_on_the_head_rows():
    """Without the max-shift, fp32 exp overflows on the +1000 rows and underflows to 0 / 0 on the
    -1000 rows: non-finite or wrong by more than the bar on most samples."""
    A, (V, Rt) = 6, S.VR_PAIRS[2]
    z, actions, target = S.head_case(A, V, Rt)
    _, dz64 = S.loss_dz(z, actions, target, False, np.float64)
    with np.errstate(all='ignore'):
        e = np.exp(z[:, :A])
        pi = e / e.sum(axis=1, keepdims=True)
        onehot = np.zeros_like(pi)
        onehot[np.arange(len(actions)), actions] = 1
        dz = -(target - z[:, A])[:, None] * (onehot - pi)       # the entropy term aside
    bad = ~np.isfinite(dz).all(axis=1)
    bad[~bad] = S.row_ratios(dz[~bad], dz64[~bad], A, V, Rt).max(initial=0) > 4 * S.r32(A)
    assert bad.sum() >= 60, int(bad.sum())


CPU_CASES = [(t, A, pair, lit) for t in ('nips', 'nature') for A in (6, 18) for pair in S.VR_PAIRS
             for lit in ((False, True) if pair == S.LITERAL_PAIR else (False,))]


@pytest.mark.parametrize('dqn_type,A,pair,literal', CPU_CASES)
def test_whole_tensor_bars_hold_the_fp32_oracle(dqn_type, A, pair, literal):
    """check_loss_backward's bars (1e-4 relative-L2 per tensor, losses 1e-5 of max(1, |loss|)) on
    the one-hot construction: the float32 oracle backward stays inside half of them, and the head
    weight gradients are the per-sample dz."""
    V, Rt = pair
    p, planes, acts = S.cpu_trunk(dqn_type, A)
    z, actions, target = S.head_case(A, V, Rt)
    width = 512 if dqn_type == 'nature' else 256
    fwd = S.same_act_fwd(dqn_type, planes, acts, z, S.one_hot(S.N_SAMPLES, width))
    g64, loss64, dz64 = S.oracle_loss_backward(p, fwd, 'a3c', dqn_type, actions, target, literal)
    g32, loss32, _ = S.oracle_loss_backward(p, S.cast_fwd(fwd, np.float32), 'a3c', dqn_type, actions, target, literal)
    assert np.array_equal(g64['p_w'][:S.N_SAMPLES], dz64[:, :A]) and not g64['p_w'][S.N_SAMPLES:].any()
    assert np.array_equal(g64['q_w'][:S.N_SAMPLES, 0], dz64[:, A])
    for name in g64:
        assert g32[name].dtype == np.float32 and np.isfinite(g32[name]).all()
        assert rel_l2(g32[name], g64[name]) < 0.5e-4, (name, rel_l2(g32[name], g64[name]))
    for a, b in zip(loss32, loss64):
        assert abs(float(a) - b) <= 0.5e-5 * max(1.0, abs(b)), (loss32, loss64)


@pytest.mark.parametrize('A', [6, 18])
def test_q_head_bars_hold_the_fp32_oracle(A):
    p, planes, acts = S.cpu_trunk('nips', A, algo='q')
    z, actions, target = S.q_case(A)
    fwd = S.same_act_fwd('nips', planes, acts, z, S.one_hot(S.N_SAMPLES, 256))
    g64, loss64, dz64 = S.oracle_loss_backward(p, fwd, 'q', 'nips', actions, target, False)
    g32, loss32, _ = S.oracle_loss_backward(p, S.cast_fwd(fwd, np.float32), 'q', 'nips', actions, target, False)
    assert np.array_equal(g64['q_w'][:S.N_SAMPLES], dz64)
    assert np.abs(dz64).max() > 100 and np.abs(target).max() == 1e4
    for name in g64:
        assert rel_l2(g32[name], g64[name]) < 0.5e-4, (name, rel_l2(g32[name], g64[name]))
    for a, b in zip(loss32, loss64):
        assert abs(float(a) - b) <= 0.5e-5 * max(1.0, abs(b)), (loss32, loss64)


# ------------------------------------------------------------------ 2. action draw
@pytest.mark.parametrize('A,stride', S.DRAW_WIDTHS)
def test_draw_rows_discriminate(A, stride):
    """The draw inputs: few rows at a CDF boundary, every action drawn often enough, a good share
    of rows past the gaps where 1 - pi rounds to 0 (17) and where expf underflows (104); and the
    unshifted fp32 softmax draws differently on more than 1,000 of the 4,096 rows."""
    zs = stride or (A + 1 + 3) // 4 * 4
    _, z = S.draw_rows(A, zs)
    assert (z[:, A:] == np.float32(1e30)).all()
    a_ref, near, u, _ = S.draw_reference(z, A)
    gap = S.top_gap(z, A)
    counts = np.bincount(a_ref, minlength=A)
    far, mid = int((gap > 104).sum()), int(((gap > 17) & (gap <= 104)).sum())
    a_raw = R.sample_categorical(S.unshifted_softmax32(z[:, :A]), u)
    differ = int((a_raw != a_ref).sum())
    print(f'A={A} zs={zs}: near {int(near.sum())} min count {counts.min()} gap>104 {far} gap in (17,104] {mid} '
          f'unshifted differs on {differ}')
    assert near.sum() <= 4                       # half of the cap of 8 masked rows
    assert counts.min() >= 2 * S.DRAW_B / (8 * A)
    if A > 2:
        assert far >= 1000 and mid >= 500
    assert differ > 1000


# ------------------------------------------------------------------ 3. LSTM
@pytest.mark.parametrize('B', [17, 37])
def test_lstm_step_bars_hold_the_fp32_oracle(B):
    """test_gpu_lstm's bars (rtol 1e-5, atol 5e-6 on h, c, gates), halved, on the float32 oracle;
    each gate 30 % or more saturated in float32 and 30 % or more not."""
    case = S.lstm_step_case(B)
    h64, c64, g64 = S.lstm_step_oracle(case)
    h32, c32, g32 = S.lstm_step_oracle(case, np.float32)
    shares = S.assert_gate_coverage(g64, B)
    print(f'B={B} saturated shares i/j/f/o', ' '.join(f'{s:.2f}' for s in shares), 'max |c|', float(np.abs(c64).max()),
          'errors h', float(np.abs(h32 - h64).max()), 'gates', float(np.abs(g32 - g64).max()))
    assert g32.dtype == np.float32 and np.abs(c64).max() > 1e3
    for got, want in ((h32, h64), (c32, c64), (g32, g64)):
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want, rtol=0.5e-5, atol=2.5e-6)
    # the sigmoid the kernels use, 1 / (1 + exp(-x)), goes through exp = inf on these inputs
    w, b, x, h, c, terms = case
    keep = (1 - terms.astype(np.float32))[:, None]
    pre = np.concatenate([x, h * keep], axis=1) @ w + b
    assert (pre < -89).mean() > 0.05 and (pre > 89).mean() > 0.05


@pytest.mark.parametrize('n,E', [(3, 17), (5, 37)])
def test_lstm_bptt_bars_hold_the_fp32_oracle(n, E):
    """Relative-L2 1e-5 on dx, dw, db and per gate, halved, on the float32 oracle."""
    inputs = S.lstm_bptt_inputs(n, E)
    S.assert_gate_coverage(inputs[2]['G'], (n, E))
    ref = S.lstm_bptt_oracle(inputs)
    got = S.lstm_bptt_oracle(inputs, np.float32)
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    gate = [rel_l2(got[1][:, k * S.U:(k + 1) * S.U], ref[1][:, k * S.U:(k + 1) * S.U]) for k in range(4)]
    gate += [rel_l2(got[2][k * S.U:(k + 1) * S.U], ref[2][k * S.U:(k + 1) * S.U]) for k in range(4)]
    print(f'n={n} E={E}: fp32 oracle dx {errs[0]:.1e} dw {errs[1]:.1e} db {errs[2]:.1e} per gate {max(gate):.1e}')
    assert got[1].dtype == np.float32
    assert max(errs) < 0.5e-5 and max(gate) < 0.5e-5


# ------------------------------------------------------------------ 4. shifted policy bias
@pytest.mark.parametrize('shift', S.SHIFTS)
def test_shifted_bias_keeps_the_policy_and_breaks_an_unshifted_softmax(shift):
    """p_b +- 100 puts every logit past 88 in magnitude, where fp32 exp(z) is inf (+), or a denormal
    of five bits or, flushed, 0 (-): the unshifted softmax is NaN, read as 0, or some percent off,
    while the shifted softmax is the unbiased net's to rounding."""
    from oracle.engine_ref import EngineRef
    A, E, seed = 6, 8, 131
    ns = R.param_shapes(A)
    p0 = S.shifted_params(seed, 4.0, 0.0)(ns)
    p = S.shifted_params(seed, 4.0, shift)(ns)
    assert np.array_equal(p['p_b'], np.full(A, shift, np.float32)) and np.array_equal(p['p_w'], p0['p_w'])
    seen = []
    ref = EngineRef(p, E, 5, A, 'a3c', 0, 48, seed)
    ref.reset()
    S.logit_recorder(A, seen)(None, ref)
    out = ref.iterate(grads=False)
    assert len(seen) == 1 and seen[0] > 88
    z = out['z'].reshape(-1, A + 1)[:, :A]
    ref0 = EngineRef(p0, E, 5, A, 'a3c', 0, 48, seed)
    ref0.reset()
    z0 = ref0.iterate(forced_actions=out['actions'], grads=False)['z'].reshape(-1, A + 1)[:, :A]
    np.testing.assert_allclose(R.softmax_stats(z)[0], R.softmax_stats(z0)[0], rtol=1e-12, atol=0)
    raw = S.unshifted_softmax32(z)
    pi = R.softmax_stats(z)[0]
    assert np.abs(raw - pi).max(axis=1).min() > 1e-4          # every row off by a thousand roundings
    if shift > 0:
        u = out['u'].reshape(-1)
        assert not raw.any() and (R.sample_categorical(raw, u) == A - 1).all()
        assert (R.sample_categorical(pi.astype(np.float32), u) != A - 1).sum() > len(u) // 2
