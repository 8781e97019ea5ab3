"""The nature trunk's bf16 compute mode without a GPU: the command line, the symbols, and the condition
the GPU forward bars rest on -- the rounded-operand layer lies at least 30 bars from the unrounded one; and the one
the backward bars rest on at B = 31 and 123 -- a dW slice loop that loses rows misses d / 8 at least 3-fold."""
import functools
import os

import numpy as np
import pytest

import _nat_bf16 as N
import _plan as PL
import _term_split as T
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATURE = ['--mode', 'engine', '--dqn_type', 'nature']
DW_TENSORS = ('l1_w', 'l2_w', 'l3_w')


@pytest.mark.parametrize('layer', N.LAYERS)
def test_dense_inputs_tell_the_modes_apart(layer):
    x = np.array([1.0, 1.00390625, 1.01171875, -1.01171875, 255.0], np.float32)      # 1 + 2^-8: a tie, to even
    assert np.array_equal(N.rn_bf16(x), np.array([1.0, 1.0, 1.015625, -1.015625, 255.0], np.float32))
    P = R.init_params(R.param_shapes(6, *N.NET), seed=2, stddev=0.08)
    states = R.states_nhwc(T.dense_states(2, 22))
    acts = R.forward(P, states, *N.NET, dtype=np.float32)['acts']
    x_in = states if layer == 'conv1' else np.ascontiguousarray(acts[int(layer[4:]) - 1], np.float32)
    _, bar, gap = N.layer_figures(P, layer, x_in)
    print(layer, 'bar %.3e  rounded vs unrounded %.3e  (x%.0f)' % (bar, gap, gap / bar))
    assert 0 < bar < 1e-5 and gap >= 30 * bar


@functools.lru_cache(maxsize=None)
def backward_mutants(B, tail_heavy):
    """The backward cases' batch on the oracle alone: init_params(seed 2, 0.08), dense states seeded 20 + B, the
    fp32 forward's activations, actions b % 6 -> (kc, d {tensor}, {mutant: {tensor: rel-L2 of the mutant to A}})."""
    P = R.init_params(R.param_shapes(6, *N.NET), seed=2, stddev=0.08)
    states = R.states_nhwc(T.dense_states(B, 20 + B))
    f = R.forward(P, states, *N.NET, dtype=np.float32)
    outs = dict(conv1=f['acts'][1], conv2=f['acts'][2], conv3=f['acts'][3], fc=f['h3'], head=f['z'])
    target = N.tail_heavy_targets(B) if tail_heavy else np.linspace(0.7, -0.4, B).astype(np.float32)
    _, dz = R.a3c_loss_and_dz(f['z'].astype(np.float64), (np.arange(B) % 6).astype(np.int32), target.astype(np.float64))
    kc = PL.nat_plan(6, B).kc
    A, Bref, muts = N.backward_refs(P, states, outs, dz, lost=N.dw_row_mutants(kc))
    d = {t: T.rel_l2(A[t], Bref[t]) for t in DW_TENSORS}
    return kc, d, {m: {t: T.rel_l2(g, A[t]) for t, g in gs.items()} for m, gs in muts.items()}


@pytest.mark.parametrize('B', [31, 123])
def test_lost_dw_rows_miss_the_bar_threefold(B):
    """Would d / 8 see a dW slice loop that loses rows?  The fp64 rounded-operand backward A against itself with
    reduction rows of the conv dW passes zeroed (N.dw_row_mutants): every mutant moves its pass's weight tensor at
    least 3 x beyond that tensor's d / 8, d = |A - B|.  Measured, mutant error / (d / 8):

      B     mutant    l1_w    l2_w    l3_w
      31    tail      27.1    93.2    487
      31    ragged    208     609     1894
      31    interior  17.1    -       -       (conv2, conv3: one slice a chunk, no interior slice)
      123   tail      21.1    84.5    427
      123   ragged    120     360     1453
      123   interior  39.2    11.6    86.1    (the smallest: l2_w 3.2e-3 against 2.7e-4)"""
    kc, d, errs = backward_mutants(B, True)
    assert kc == {31: (64, 32, 32), 123: (160, 64, 96)}[B]
    assert {m: sorted(e) for m, e in errs.items()} == dict(
        tail=list(DW_TENSORS), ragged=list(DW_TENSORS),
        interior=[t for t, k in zip(DW_TENSORS, kc) if k >= 64])
    for m, e in errs.items():
        for t, err in e.items():
            print(f'B={B} {m:<8} {t} mutant {err:.3e}  d/8 {d[t] / 8:.3e}  x{err / (d[t] / 8):.1f}')
            assert err >= 3 * d[t] / 8, (B, m, t, err, d[t] / 8)


def test_flat_targets_hide_a_lost_tail_row():
    """Why the backward cases' last target is 50: with the suite's flat ramp, conv1's last reduction row of 49 200 at
    B = 123 moves l1_w by less than its d / 8, and the bf16 bar would pass a kernel that dropped it."""
    _, d, errs = backward_mutants(123, False)
    print(f"flat targets B=123 tail l1_w mutant {errs['tail']['l1_w']:.3e}  d/8 {d['l1_w'] / 8:.3e}")
    assert errs['tail']['l1_w'] < d['l1_w'] / 8
    _, d, errs = backward_mutants(123, True)
    assert errs['tail']['l1_w'] >= 3 * d['l1_w'] / 8


def test_precision_flag_mapping_and_rejections():
    import main
    assert main.engine_options(main.parse_flags(NATURE + ['--precision', 'bf16'])) == dict(
        lstm=False, dqn_type='nature', precision='bf16')
    for argv in ([], NATURE, NATURE + ['--precision', 'fp32'], ['--precision', 'fp32'], ['--algo', 'q']):
        assert 'precision' not in main.engine_options(main.parse_flags(argv))
    assert main.engine_options(main.parse_flags([])) == dict(lstm=False)
    assert main.engine_options(main.parse_flags(NATURE)) == dict(lstm=False, dqn_type='nature')
    with pytest.raises(ValueError, match='--precision bf16 is the compute mode of the nature trunk'):
        main.engine_options(main.parse_flags(['--mode', 'engine', '--precision', 'bf16']))
    with pytest.raises(ValueError, match='--precision must be fp32 or bf16'):
        main.engine_options(main.parse_flags(NATURE + ['--precision', 'fp16']))
    with pytest.raises(ValueError, match='--precision is an engine option'):
        main.main(['--mode', 'agent', '--precision', 'bf16'])
    from src.engine import Engine
    with pytest.raises(ValueError, match="precision 'bf16' is the nature trunk's"):
        Engine._check_precision('bf16', 'nips')
    with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16'"):
        Engine._check_precision('half', 'nature')


def test_symbols_in_header_and_loader():
    from src import _lib
    header = open(os.path.join(ROOT, 'include', 'a3c_hip.h')).read()
    for name in ('a3c_nature_forward_prec', 'a3c_nature_loss_backward_prec', 'a3c_engine_set_precision'):
        assert name + '(' in header and name in _lib.SIGNATURES
    assert '#define A3C_PREC_FP32 0' in header and '#define A3C_PREC_BF16 1' in header
    assert (_lib.PREC_FP32, _lib.PREC_BF16) == (0, 1) and _lib.PRECISIONS == dict(fp32=0, bf16=1)
