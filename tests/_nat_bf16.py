"""The float64 reference of the nature trunk's bf16 compute mode: both operands of a convolution pass
through rn_bf16; the pass structure and the sequential fp32 chain are tests/_term_split.py's, unchanged."""
import numpy as np

import _term_split as T
from oracle import ref_cpu as R

NET = ('a3c', 'nature')
LAYERS = ('conv1', 'conv2', 'conv3')
CONV_TENSORS = ('l1_w', 'l1_b', 'l2_w', 'l2_b', 'l3_w', 'l3_b')


def rn_bf16(x):
    """The fp32 value of x rounded to the nearest-even bf16, as fp32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def layer_figures(P, layer, x_in):
    """One forward layer on its own input (conv1: u8 NHWC states; else the fp32 NHWC output below) -> (ref, bar, gap):
    the fp64 layer on rn_bf16 operands; 3 x the error of that layer as a sequential fp32 chain (a product of two bf16
    values is exact in fp32: accumulation is all that is left); the fp64 layer on unrounded operands against ref."""
    c = T.forward_case(P, layer, x_in, *NET)
    ev = T.Case(layer, rn_bf16(c.A), rn_bf16(c.B), bias=c.bias, scale=c.scale, relu=True).evaluate()
    plain = np.maximum(c._post64(c.A.astype(np.float64) @ c.B.astype(np.float64)), 0)
    return ev['ref'], 3.0 * T.rel_l2(ev['honest'], ev['ref']), T.rel_l2(plain, ev['ref'])


def backward_refs(P, states_nhwc, outs, dz):
    """(A, B) on the activations `outs`: the fp64 backward with both operands of every conv pass rounded from the
    fp32 value the pass reads, and with no rounding; ReLU masks and bias sums (of the unrounded dY) are shared."""
    fwd = T.fwd_record(P, states_nhwc, outs, *NET)

    def mm(name, a, b, scale):
        if name.startswith('conv'):
            a, b = rn_bf16(a), rn_bf16(b)
        return T.mm_fp64(name, a, b, scale)
    return T.backward_chain(P, fwd, dz, *NET, mm), R.backward(P, fwd, dz, *NET)
