"""The nature trunk's bf16 fc mode without a GPU: the command line, the symbols, and the two conditions the
GPU bars rest on, on the oracle alone.  `chain` is the reference of both files: tests/_nat_bf16.py's backward_refs
`mm`, rounding the passes whose names start with the given prefixes ('conv', 'fc': the mode; 'conv': the parent's)."""
import os

import numpy as np
import pytest

import _nat_bf16 as N
import _term_split as T
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATURE = ['--mode', 'engine', '--dqn_type', 'nature']
REACHED = ('l4_w', 'l3_w', 'l3_b', 'l2_w', 'l2_b', 'l1_w', 'l1_b')     # by a product of an fc backward pass
# lost work: fc dW without the last sample's row, fc dX without the last k (the A operand's last column in both)
MUTANTS = dict(fc_dW=('l4_w',), fc_dX=('l3_w', 'l3_b'))


def chain(P, states_nhwc, outs, dz, rounded, lost=None):
    fwd = T.fwd_record(P, states_nhwc, outs, *N.NET)

    def mm(name, a, b, scale):
        if name.startswith(rounded):
            a, b = N.rn_bf16(a), N.rn_bf16(b)
        if name == lost:
            a = np.array(a)
            a[:, -1] = 0
        return T.mm_fp64(name, a, b, scale)
    return T.backward_chain(P, fwd, dz, *N.NET, mm)


def oracle_batch(B):
    P = R.init_params(R.param_shapes(6, *N.NET), seed=2, stddev=0.08)
    states = R.states_nhwc(T.dense_states(B, 20 + B))
    f = R.forward(P, states, *N.NET, dtype=np.float32)
    outs = dict(conv1=f['acts'][1], conv2=f['acts'][2], conv3=f['acts'][3], fc=f['h3'], head=f['z'])
    _, dz = R.a3c_loss_and_dz(f['z'].astype(np.float64), (np.arange(B) % 6).astype(np.int32),
                              N.tail_heavy_targets(B).astype(np.float64))
    return P, states, outs, dz


def test_rounded_fc_layer_is_30_bars_from_the_unrounded():
    P, _, outs, _ = oracle_batch(3)
    _, bar, gap = N.layer_figures(P, 'fc', np.ascontiguousarray(outs['conv3'], np.float32))
    print('fc bar %.3e  rounded vs unrounded %.3e  (x%.0f)' % (bar, gap, gap / bar))
    assert 0 < bar < 1e-5 and gap >= 30 * bar


@pytest.mark.parametrize('B', [3, 65])
def test_lost_fc_rows_miss_the_bar_threefold(B):
    """d = |A - C| per reached tensor (A: conv and fc passes rounded, C: conv passes only) and each mutant of A against
    A.  Measured, B = 3 / 65: d 1.2e-3 .. 4.8e-3; the dW mutant moves l4_w by 0.98 / 0.51 (x3580 / x3316 of d / 8),
    the dX mutant l3_w and l3_b by 0.09 / 0.06 (x264, x326 / x170, x212)."""
    P, states, outs, dz = oracle_batch(B)
    A, C = chain(P, states, outs, dz, ('conv', 'fc')), chain(P, states, outs, dz, ('conv',))
    d = {t: T.rel_l2(A[t], C[t]) for t in REACHED}
    print(f'B={B} d ' + '  '.join(f'{t} {v:.2e}' for t, v in d.items()))
    assert min(d.values()) > 5e-4 and T.rel_l2(A['l4_b'], C['l4_b']) == 0
    for lost, tensors in MUTANTS.items():
        M = chain(P, states, outs, dz, ('conv', 'fc'), lost=lost)
        for t in tensors:
            err = T.rel_l2(M[t], A[t])
            print(f'B={B} {lost} mutant {t} {err:.3e}  d/8 {d[t] / 8:.3e}  x{err / (d[t] / 8):.0f}')
            assert err >= 3 * d[t] / 8, (B, lost, t, err, d[t] / 8)


def test_fc_precision_flag_mapping_and_rejections():
    import main
    both = NATURE + ['--precision', 'bf16', '--fc_precision', 'bf16']
    assert main.engine_options(main.parse_flags(both)) == dict(lstm=False, dqn_type='nature', precision='bf16',
                                                               fc_precision='bf16')
    assert main.engine_options(main.parse_flags(NATURE + ['--fc_precision', 'bf16'])) == dict(
        lstm=False, dqn_type='nature', fc_precision='bf16')
    assert main.engine_options(main.parse_flags(NATURE + ['--fc_precision', 'fp32'])) == dict(lstm=False, dqn_type='nature')
    assert main.engine_options(main.parse_flags(NATURE)) == dict(lstm=False, dqn_type='nature')
    with pytest.raises(ValueError, match='--fc_precision bf16 is the fc compute mode of the nature trunk'):
        main.engine_options(main.parse_flags(['--mode', 'engine', '--fc_precision', 'bf16']))
    with pytest.raises(ValueError, match='--fc_precision must be fp32 or bf16'):
        main.engine_options(main.parse_flags(NATURE + ['--fc_precision', 'fp16']))
    with pytest.raises(ValueError, match='--fc_precision is an engine option'):
        main.main(['--mode', 'agent', '--fc_precision', 'bf16'])
    from src.engine import Engine
    with pytest.raises(ValueError, match="fc_precision 'bf16' is the nature trunk's"):
        Engine._check_fc_precision('bf16', 'nips')
    with pytest.raises(ValueError, match="fc_precision must be 'fp32' or 'bf16'"):
        Engine._check_fc_precision('half', 'nature')


def test_symbols_in_header_and_loader():
    from src import _lib
    header = open(os.path.join(ROOT, 'include', 'a3c_hip.h')).read()
    for name in ('a3c_nature_forward_prec2', 'a3c_nature_loss_backward_prec2', 'a3c_engine_set_fc_precision'):
        assert name + '(' in header and name in _lib.SIGNATURES
    assert '#define A3C_KER_NAT_FCW 16' in header and '#define A3C_KER_NAT_FCX 17' in header
    assert _lib.KER_NAT_FC_BWD == dict(fc_dw=16, fc_dx=17) and _lib.KER_NAT['fc_fwd'] == 10
    assert len(_lib.SIGNATURES['a3c_nature_forward_prec2'][1]) == len(_lib.SIGNATURES['a3c_nature_forward_prec'][1]) + 1
