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


def backward_refs(P, states_nhwc, outs, dz, lost=None):
    """(A, B) on the activations `outs`: the fp64 backward with both operands of every conv pass rounded from the
    fp32 value the pass reads, and with no rounding; ReLU masks and bias sums (of the unrounded dY) are shared.
    lost {mutant: rows(pass index 0..2, reduction rows) -> the rows that mutant loses, or None}: a third value
    {mutant: {l1_w..l3_w}}, each conv dW pass of A computed again with those reduction rows zeroed (a dW product
    feeds no other tensor, so one chain carries every mutant)."""
    fwd = T.fwd_record(P, states_nhwc, outs, *NET)
    muts = {m: {} for m in (lost or {})}

    def mm(name, a, b, scale):
        if name.startswith('conv'):
            a, b = rn_bf16(a), rn_bf16(b)
            if name.endswith('_dW'):
                for m, rows in (lost or {}).items():
                    gone = rows(int(name[4]) - 1, a.shape[1])
                    if gone is not None:
                        cut = a.copy()
                        cut[:, gone] = 0
                        t = f'l{name[4]}_w'
                        muts[m][t] = T.mm_fp64(name, cut, b, scale).reshape(np.shape(P[t]))
        return T.mm_fp64(name, a, b, scale)
    A, Bref = T.backward_chain(P, fwd, dz, *NET, mm), R.backward(P, fwd, dz, *NET)
    return (A, Bref) if lost is None else (A, Bref, muts)


def tail_heavy_targets(B):
    """The backward cases' returns: the suite's ramp with the last sample's set to 50, so that the last sample
    carries the gradient and a lost tail row of a dW reduction is no longer hidden by the B - 1 samples before it
    (tests/test_nat_bf16_cpu.py holds both halves of that sentence)."""
    target = np.linspace(0.7, -0.4, B).astype(np.float32)
    target[-1] = 50.0
    return target


def dw_row_mutants(kc):
    """The three ways a dW workgroup's slice loop can lose reduction rows, as backward_refs' `lost`; kc is the plan's
    (conv1, conv2, conv3) chunk triple, slices are _plan.NAT_BK = 32 rows:
      tail      the last reduction row;
      ragged    the last chunk's last slice (rows % 32 or 32 rows);
      interior  the second slice of chunk 1, rows kc + 32 .. kc + 63, where a chunk holds two slices or more."""
    return dict(
        tail=lambda i, rows: slice(rows - 1, rows),
        ragged=lambda i, rows: slice(rows - (rows % 32 or 32), rows),
        interior=lambda i, rows: slice(kc[i] + 32, kc[i] + 64) if kc[i] >= 64 and kc[i] + 64 <= rows else None)
