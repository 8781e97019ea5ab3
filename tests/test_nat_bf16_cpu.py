"""The nature trunk's bf16 compute mode without a GPU: the command line, the symbols, and the condition
the GPU forward bars rest on -- the rounded-operand layer lies at least 30 bars from the unrounded one."""
import os

import numpy as np
import pytest

import _nat_bf16 as N
import _term_split as T
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATURE = ['--mode', 'engine', '--dqn_type', 'nature']


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
