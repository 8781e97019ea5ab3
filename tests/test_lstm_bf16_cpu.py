"""The LSTM head's bf16 mode without a GPU: the GPU bars of tests/test_gpu_lstm_bf16.py separate a
kernel that rounds where the mode says from one that does not, and the flag and option checks."""
import numpy as np
import pytest

import _lstm_bf16 as LB


@pytest.mark.parametrize('B', LB.STEP_B)
def test_unrounded_cell_misses_the_step_bar(B):
    k = LB.step_case(B)
    keep = (1 - k['terms'].astype(np.float32))[:, None]
    for x in (k['x'], k['x_fold']):
        ref = LB.cell(x, k['h'] * keep, k['c'] * keep, k['w'], k['b'])
        off = LB.cell(x, k['h'] * keep, k['c'] * keep, k['w'], k['b'], r=LB.plain)
        for got, want in zip(off, ref):
            assert not np.allclose(got, want, **LB.STEP_BAR)


@pytest.mark.parametrize('n,E', LB.BPTT_SHAPES)
def test_unrounded_backward_is_outside_the_bptt_bar(n, E):
    """d = rel-L2(rounded, unrounded): the GPU bar max(d / 8, 1e-5) is d / 8 wherever a rounded product is seen."""
    case = LB.bptt_case(n, E)
    d = [LB.rel_l2(a, b) for a, b in zip(LB.backward_seq(*case, r=LB.plain), LB.backward_seq(*case))]
    print(f'n={n} E={E}: d dx {d[0]:.3e} dw {d[1]:.3e} db {d[2]:.3e}')
    assert d[1] > 8e-5
    if n > 1:
        assert d[0] > 8e-5 and d[2] > 0
    else:
        assert d[2] == 0      # (db of the last step sees no rounded product: the floor is its bar)


def test_lstm_precision_flags_and_option_checks():
    import main
    assert main.engine_options(main.parse_flags(['--lstm', 'true', '--lstm_precision', 'bf16'])) == dict(
        lstm=True, lstm_precision='bf16')
    assert main.engine_options(main.parse_flags(['--lstm', 'true'])) == dict(lstm=True)
    with pytest.raises(ValueError, match='--lstm_precision bf16 is the compute mode of the LSTM head'):
        main.engine_options(main.parse_flags(['--lstm_precision', 'bf16']))
    with pytest.raises(ValueError, match='--lstm_precision must be fp32 or bf16'):
        main.engine_options(main.parse_flags(['--lstm', 'true', '--lstm_precision', 'fp16']))
    with pytest.raises(ValueError, match='--lstm_precision is an engine option'):
        main.main(['--mode', 'agent', '--lstm', 'true', '--lstm_precision', 'bf16'])
    from src.engine import Engine
    with pytest.raises(ValueError, match="lstm_precision 'bf16' is the LSTM head's"):
        Engine._check_lstm_precision('bf16', False)
    with pytest.raises(ValueError, match="lstm_precision must be 'fp32' or 'bf16'"):
        Engine._check_lstm_precision('half', True)
    assert Engine._check_lstm_precision('bf16', True) == 'bf16'
