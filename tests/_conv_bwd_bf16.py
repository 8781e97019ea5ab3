"""Inputs and the float64 reference of the nips conv backward's bf16 mode, shared by
tests/test_gpu_conv_bwd_bf16.py and tests/test_conv_bwd_bf16_cpu.py: tests/_term_split.backward_chain with both
operands of the three conv products (conv2_dW, conv2_dX, conv1_dW) through _nat_bf16.rn_bf16; masks and bias
sums come from the unrounded values there."""
import numpy as np

import _nat_bf16 as N
import _plan
import _term_split as T
from oracle import ref_cpu as R

A = 6
CASES = [('a3c', 1), ('a3c', 5), ('a3c', 259), ('q', 5)]     # per_wg 1, 1 (groups = nwg = 5), 2 with a ragged last workgroup
MOVED = ('l1_w', 'l1_b', 'l2_w')                              # tensors a rounded product reaches (l2_b: sum of dl2)


def plan_facts():
    p1, p5, p259 = (_plan.bwd_plan(A, 'a3c', B) for B in (1, 5, 259))
    assert (p1.per_wg, p5.per_wg, p5.nwg, p5.groups) == (1, 1, 5, 5) and p5.nwg < 16
    assert p259.per_wg == 2 and _plan.wg_samples(p259, p259.nwg - 1) == 1


def case(algo, B):
    """(names_shapes, P, planes [B,4,84,84] u8, actions, target)."""
    ns = R.param_shapes(A, algo)
    P = R.init_params(ns, seed=7 + B, stddev=0.08)
    return ns, P, T.dense_states(B, 40 + B), (np.arange(B) % A).astype(np.int32), N.tail_heavy_targets(B)


def dz_of(algo, z, actions, target):
    f = R.a3c_loss_and_dz if algo == 'a3c' else R.q_loss_and_dz
    return f(np.asarray(z, np.float64), actions, target.astype(np.float64))[1]


def refs(P, planes, outs, dz, algo):
    """(rounded, unrounded) fp64 gradients on the activations `outs` {conv1, conv2, fc, head}."""
    fwd = T.fwd_record(P, R.states_nhwc(planes), outs, algo, 'nips')

    def mm(name, a, b, scale):
        return T.mm_fp64(name, N.rn_bf16(a), N.rn_bf16(b), scale) if name.startswith('conv') else T.mm_fp64(name, a, b, scale)
    return T.backward_chain(P, fwd, dz, algo, 'nips', mm), R.backward(P, fwd, dz, algo, 'nips')
