"""The float64 reference of the LSTM head's bf16 compute mode: oracle.ref_cpu's lstm_cell and
lstm_backward_seq with rn_bf16 on the operands of the three matrix products and nowhere else."""
import numpy as np

from _nat_bf16 import rn_bf16
from oracle import ref_cpu as Rc

U = 256
STEP_BAR = dict(rtol=1e-5, atol=5e-6)      # test_lstm_step_matches_oracle's: products of bf16 operands are exact in fp32


def plain(a):
    return np.asarray(a, np.float64)


def rn(a):
    return rn_bf16(np.asarray(a, np.float32)).astype(np.float64)


def rel_l2(a, b):
    return np.linalg.norm(plain(a) - plain(b)) / max(np.linalg.norm(plain(b)), 1e-30)


def cell(x, h, c, w, b, r=rn):
    """(h', c', gates) of a = r([x, h]) r(w) + b on the already-masked h, c."""
    return Rc.lstm_cell(r(x), r(h), plain(c), r(w), plain(b))


def backward_seq(w, x, hp, cp, gates, c, terms, dh, r=rn):
    """lstm_backward_seq with d[x, hp] = r(da) r(w)^T and dw = r([x, hp])^T r(da); db sums the unrounded da.
    Returns (dx masked by x > 0, dw, db)."""
    n, E, _ = dh.shape
    W = r(w)
    dX, dW, db = np.zeros(x.shape), np.zeros(w.shape), np.zeros(w.shape[1])
    dh_next, dc_next = np.zeros((E, U)), np.zeros((E, U))
    for t in range(n - 1, -1, -1):
        keep = 1.0 - plain(terms[t])[:, None]
        d = plain(dh[t]) + dh_next * keep
        i, j, f, o = (plain(gates[t][:, k * U:(k + 1) * U]) for k in range(4))
        tc = np.tanh(plain(c[t]))
        dc = dc_next * keep + d * o * (1.0 - tc * tc)
        da = np.concatenate([dc * j * i * (1.0 - i), dc * i * (1.0 - j * j), dc * plain(cp[t]) * f * (1.0 - f),
                             d * tc * o * (1.0 - o)], axis=1)
        dW += r(np.concatenate([x[t], hp[t]], axis=1)).T @ r(da)
        db += da.sum(0)
        dxh = r(da) @ W.T
        dX[t], dh_next, dc_next = dxh[:, :256], dxh[:, 256:], dc * f
    return dX * (plain(x) > 0), dW, db


def step_case(B):
    """test_lstm_step_matches_oracle's inputs, plus the same x as 8 fc partials + bias (their fp32 fold in slice
    order, bias, ReLU is x_fold)."""
    rng = np.random.default_rng(B)
    w = (rng.standard_normal((512, 1024)) * 0.06).astype(np.float32)
    b = (rng.standard_normal(1024) * 0.1).astype(np.float32)
    x = np.maximum(rng.standard_normal((B, 256)), 0).astype(np.float32)
    h = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    c = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    terms = (rng.random(B) < 0.3).astype(np.uint8)
    part = (rng.standard_normal((8, B, 256)) * 0.4).astype(np.float32)
    fc_b = (rng.standard_normal(256) * 0.1).astype(np.float32)
    v = part[0].copy()
    for s in range(1, 8):
        v = v + part[s]
    return dict(w=w, b=b, x=x, h=h, c=c, terms=terms, fc_part=part, fc_bias=fc_b, x_fold=np.maximum(v + fc_b, 0))


def bptt_case(n, E):
    """tests/test_gpu_lstm.py _bptt_case's inputs: (w, x, hp, cp, gates, c, terms, dh)."""
    from test_gpu_lstm import _bptt_case
    return _bptt_case(n, E)[0]


STEP_B = (1, 17, 37)
BPTT_SHAPES = ((1, 16), (2, 17), (3, 87))
