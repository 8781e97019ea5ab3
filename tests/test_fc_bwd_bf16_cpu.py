"""The nips fc backward's bf16 mode without a GPU: the bars of tests/test_gpu_fc_bwd_bf16.py see a lost
sample row of dW and a lost k of dX, and the flag, option and symbol checks."""
import os

import numpy as np
import pytest

import _conv_bwd_bf16 as C
import _fc_bwd_bf16 as F
import _term_split as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('mutant,tensors', [('fc_dW', ('fc_w',)), ('fc_dX', F.CONV)])
def test_bars_see_a_lost_k_index(mutant, tensors):
    """At B = 5 (one ragged slice of dW, one partial row block of dX) a product without its last K index lies more
    than 10 bars from the rounded reference (measured: 230 to 3500).  The q case: with ('a3c', 5)'s seeds column 255
    of dl3 is all but dead (norm 0.16 against a typical 4.3), so losing it is no defect those inputs could show."""
    algo, B = 'q', 5
    _, P, planes, actions, target = C.case(algo, B)
    _, outs = T.forward_emulated(P, np.ascontiguousarray(planes.transpose(0, 2, 3, 1)), algo, 'nips')
    outs = {k: v.reshape(B, -1) for k, v in outs.items()}
    dz = C.dz_of(algo, outs['head'], actions, target)
    rounded, plain = F.refs(P, planes, outs, dz, algo)
    broken, _ = F.refs(P, planes, outs, dz, algo, mutant=mutant)
    for t in (T.fc_name(algo) + '_w' if t == 'fc_w' else t for t in tensors):
        d, bar = F.bar(plain, rounded, t)
        moved = T.rel_l2(broken[t], rounded[t])
        print(f'{mutant} {t}: moved {moved:.3e}  d {d:.3e}  bar {bar:.3e}')
        assert moved > 10 * bar, (t, moved, bar)


def test_flags_options_and_symbols():
    import main
    from src import _lib
    from src.engine import Engine
    opts = lambda *a: main.engine_options(main.parse_flags(list(a)))   # noqa: E731
    assert opts('--fc_bwd_precision', 'bf16') == dict(lstm=False, fc_bwd_precision='bf16')
    assert opts('--fc_bwd_precision', 'fp32') == dict(lstm=False)
    assert opts('--algo', 'q', '--fc_bwd_precision', 'bf16', '--conv_bwd_precision', 'bf16') == dict(
        lstm=False, conv_bwd_precision='bf16', fc_bwd_precision='bf16')
    assert opts('--lstm', 'true', '--lstm_precision', 'bf16', '--fc_bwd_precision', 'bf16') == dict(
        lstm=True, lstm_precision='bf16', fc_bwd_precision='bf16')
    with pytest.raises(ValueError, match='--fc_bwd_precision bf16 is the fc backward mode of the nips trunk.*--fc_precision'):
        opts('--dqn_type', 'nature', '--fc_bwd_precision', 'bf16')
    with pytest.raises(ValueError, match='--fc_bwd_precision must be fp32 or bf16'):
        opts('--fc_bwd_precision', 'fp16')
    with pytest.raises(ValueError, match='--fc_bwd_precision is an engine option'):
        main.main(['--mode', 'agent', '--fc_bwd_precision', 'bf16'])
    with pytest.raises(ValueError, match="fc_bwd_precision 'bf16' is the nips trunk's"):
        Engine._check_fc_bwd_precision('bf16', 'nature')
    with pytest.raises(ValueError, match='fc_bwd_precision must be'):
        Engine._check_fc_bwd_precision('fp16', 'nips')
    assert Engine._check_fc_bwd_precision('bf16', 'nips') == 'bf16'
    header = open(os.path.join(ROOT, 'include', 'a3c_hip.h')).read()
    for name in ('a3c_loss_backward_prec2', 'a3c_engine_set_fc_bwd_precision', 'a3c_fc_bwd_bf16'):
        assert name + '(' in header and name in _lib.SIGNATURES and name in _lib.OPTIONAL_IN_OLD_BUILDS
    assert len(_lib.SIGNATURES['a3c_loss_backward_prec2'][1]) == len(_lib.SIGNATURES['a3c_loss_backward_prec'][1]) + 1
