"""Inputs and float64 references of the nips fc backward's bf16 mode, shared by
tests/test_gpu_fc_bwd_bf16.py and tests/test_fc_bwd_bf16_cpu.py: the two passes alone, and
tests/_term_split.backward_chain with both operands of fc_dW and fc_dX (and, with conv, of the three conv products)
through _nat_bf16.rn_bf16; masks and bias sums come from the unrounded values there."""
import numpy as np

import _nat_bf16 as N
import _term_split as T
from oracle import ref_cpu as R

FLAT, FC = 2592, 256
CONV = ('l1_w', 'l1_b', 'l2_w', 'l2_b')             # they read the new dl2 (the fc bias: a sum of the unrounded dl3)


def passes_inputs(B):
    rng = np.random.default_rng(900 + B)
    l2 = np.maximum(rng.standard_normal((B, FLAT)), 0).astype(np.float32)
    return l2, rng.standard_normal((B, FC)).astype(np.float32), (0.08 * rng.standard_normal((FLAT, FC))).astype(np.float32)


def passes_ref(l2, dl3, W, rnd=N.rn_bf16):
    """fp64 (dW, colsum, dl2) with the product operands through rnd; the mask and the sums from the fp32 values."""
    a, d, w = (np.asarray(rnd(x), np.float64) for x in (l2, dl3, W))
    return a.T @ d, dl3.astype(np.float64).sum(0), (d @ w.T) * (l2 > 0)


def bits_of(l2):
    """The forward's ReLU bits of l2 [B, 2592]: int32 [B, 81], bit n & 31 of word n >> 5."""
    b = (l2 > 0).reshape(len(l2), FLAT // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return b.sum(-1).astype(np.uint32).view(np.int32)


def mm_of(conv=False, mutant=None):
    """backward_chain's mm: fc_dW and fc_dX (conv: and the conv products) on rounded operands; mutant 'fc_dW' /
    'fc_dX' drops that product's last K index (a lost sample row, a lost k of the staged 256)."""
    def mm(name, a, b, scale):
        if name == mutant:
            a, b = a[:, :-1], b[:-1]
        if name in ('fc_dW', 'fc_dX') or (conv and name.startswith('conv')):
            a, b = N.rn_bf16(a), N.rn_bf16(b)
        return T.mm_fp64(name, a, b, scale)
    return mm


def refs(P, planes, outs, dz, algo, conv=False, mutant=None):
    """(rounded, unrounded) fp64 gradients on the activations `outs` {conv1, conv2, fc, head}."""
    fwd = T.fwd_record(P, R.states_nhwc(planes), outs, algo, 'nips')
    return T.backward_chain(P, fwd, dz, algo, 'nips', mm_of(conv, mutant)), R.backward(P, fwd, dz, algo, 'nips')


def bar(plain, rounded, t):
    """§4r's rule: an eighth of the distance between the unrounded and the rounded fp64 tensor, floored at 1e-5."""
    d = T.rel_l2(plain[t], rounded[t])
    return d, max(d / 8, 1e-5)
