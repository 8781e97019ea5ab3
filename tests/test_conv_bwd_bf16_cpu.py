"""The nips conv backward's bf16 mode without a GPU: the GPU bar of tests/test_gpu_conv_bwd_bf16.py
separates a kernel that rounds where the mode says from one that does not, the plan facts its batch sizes rest on,
and the flag, option and symbol checks."""
import os

import numpy as np
import pytest

import _conv_bwd_bf16 as C
import _term_split as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_sizes_reach_the_plan_forks():
    C.plan_facts()


@pytest.mark.parametrize('algo,B', C.CASES)
def test_unrounded_backward_is_outside_the_bar(algo, B):
    """d / 8 > 1e-5 for every tensor a rounded product reaches: the bar max(d / 8, 1e-5) is never the floor, and the
    unrounded reference (an fp32 kernel launched by mistake) lies 8 bars away."""
    _, P, planes, actions, target = C.case(algo, B)
    _, outs = T.forward_emulated(P, np.ascontiguousarray(planes.transpose(0, 2, 3, 1)), algo, 'nips')
    outs = {k: v.reshape(B, -1) for k, v in outs.items()}
    rounded, plain = C.refs(P, planes, outs, C.dz_of(algo, outs['head'], actions, target), algo)
    for t in C.MOVED:
        d = T.rel_l2(plain[t], rounded[t])
        print(f'{algo} B={B} {t}: d {d:.3e}')
        assert d / 8 > 1e-5, (t, d)
    assert T.rel_l2(plain['l2_b'], rounded['l2_b']) < 1e-12      # (no rounded product: fp64 summation order only)


def test_flags_options_and_symbols():
    import main
    from src import _lib
    from src.engine import Engine
    opts = lambda *a: main.engine_options(main.parse_flags(list(a)))   # noqa: E731
    assert opts('--conv_bwd_precision', 'bf16') == dict(lstm=False, conv_bwd_precision='bf16')
    assert opts('--conv_bwd_precision', 'fp32') == dict(lstm=False)
    assert opts('--algo', 'q', '--conv_bwd_precision', 'bf16')['conv_bwd_precision'] == 'bf16'
    assert opts('--lstm', 'true', '--conv_bwd_precision', 'bf16') == dict(lstm=True, conv_bwd_precision='bf16')
    with pytest.raises(ValueError, match='--conv_bwd_precision bf16 is the conv backward mode of the nips trunk'):
        opts('--dqn_type', 'nature', '--conv_bwd_precision', 'bf16')
    with pytest.raises(ValueError, match='--conv_bwd_precision must be fp32 or bf16'):
        opts('--conv_bwd_precision', 'fp16')
    with pytest.raises(ValueError, match='--conv_bwd_precision is an engine option'):
        main.main(['--mode', 'agent', '--conv_bwd_precision', 'bf16'])
    with pytest.raises(ValueError, match="conv_bwd_precision 'bf16' is the nips trunk's"):
        Engine._check_conv_bwd_precision('bf16', 'nature')
    assert Engine._check_conv_bwd_precision('bf16', 'nips') == 'bf16'
    header = open(os.path.join(ROOT, 'include', 'a3c_hip.h')).read()
    for name in ('a3c_loss_backward_prec', 'a3c_engine_set_conv_bwd_precision'):
        assert name + '(' in header and name in _lib.SIGNATURES
