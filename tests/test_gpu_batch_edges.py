"""The loss-and-backward path at the batch sizes where its launch plan forks.

The backward picks its launch shape from the batch size B = n * E alone (a3c_bwd_plan, nat_plan /
dw_split, lstm_ws and the two GEMM split helpers, restated in tests/_plan.py and tied to the
library by tests/test_plan_cpu.py).  The other suites cover action width, hyperparameters, episode
ends and the GEMM at their own forks; the batches here are the smallest that reach each fork of B.
Every case first asserts from _plan that its B reaches the fork it names, so moving a plan constant
fails a test instead of silently un-testing the fork.

Checks and bars are the shared ones, unchanged: check_forward / check_loss_backward
(tests/_net_parity.py), check_nature_forward_loss_backward (tests/test_gpu_action_width.py),
check_sync_vs_oracle / check_overlap_vs_oracle (tests/_engine_parity.py) and
check_lstm_sync_vs_oracle (tests/test_gpu_lstm.py): gradients 1e-4 relative-L2 against the oracle
backward on the kernels' own activations, 2e-2 against the independent fp64 pass, with the guard
checks on the z rows and the gradient buffer's gaps.  tests/test_batch_edges_cpu.py shows that a
lost or misplaced tail sample at B = 257 / 515 misses the 1e-4 bar at least 37-fold on every
tensor.

The largest rel-L2 each case saw on an MI355X (same-activation / independent) stands next to it."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _plan as P  # noqa: E402
from _engine_parity import check_overlap_vs_oracle, check_sync_vs_oracle  # noqa: E402
from _net_parity import check_forward, check_loss_backward  # noqa: E402
from test_gpu_action_width import check_nature_forward_loss_backward  # noqa: E402
from test_gpu_lstm import check_lstm_sync_vs_oracle  # noqa: E402

A = 6


@pytest.fixture(scope='module')
def K():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


def conv_shape(p):
    """(per_wg, nwg, samples of the last workgroup, slabs of the last slab group)."""
    return p.per_wg, p.nwg, P.wg_samples(p, p.nwg - 1), P.group_slabs(p, p.groups - 1)


def fc_slab_rows(B):
    """Valid rows of each K slab of the fc weight GEMM (K = B)."""
    p = P.bwd_plan(A, 'a3c', B)
    kc = P.gemm_kchunk(B, P.gemm_plan_split(P.FLAT, P.FC, B, 512))
    return [min(B, (s + 1) * kc) - s * kc for s in range(p.fc_split_slab)]


# what each batch reaches, asserted from the restated plan
def reaches_1(p):
    assert conv_shape(p) == (1, 1, 1, 1) and p.groups == 1 and (p.head_split, p.fc_split_slab) == (1, 1)


def reaches_16(p):       # the last B with one fc slab and one head slab (one full k-tile)
    assert (p.head_split, p.fc_split_slab) == (1, 1) and P.bwd_plan(A, 'a3c', 17).fc_split_slab == 2
    assert conv_shape(p) == (1, 16, 1, 1) and p.groups == 16


def reaches_33(p):       # the first 3-way fc split; 33 slabs in 16 groups of 3, the last 5 groups empty
    assert p.fc_split_slab == 3 and P.bwd_plan(A, 'a3c', 32).fc_split_slab == 2 and fc_slab_rows(33) == [16, 16, 1]
    assert p.head_split == 3 and p.per_group == 3 and conv_shape(p) == (1, 33, 1, 0)


def reaches_65(p):       # back to 3 slabs (2 at 49..64), the last one holding a single valid row
    assert p.fc_split_slab == 3 and P.bwd_plan(A, 'a3c', 64).fc_split_slab == 2 and fc_slab_rows(65) == [32, 32, 1]
    assert p.head_split == 5


def reaches_257(p):      # the smallest B with per_wg 2; the last workgroup is short, the last slab group empty
    assert P.bwd_plan(A, 'a3c', 256).per_wg == 1
    assert conv_shape(p) == (2, 129, 1, 0) and (p.groups, p.per_group) == (16, 9)
    assert P.group_slabs(p, 14) == 3


def reaches_515(p):      # per_wg 3 (the staging buffer index returns to 0) with a two-sample last workgroup
    assert P.bwd_plan(A, 'a3c', 512).per_wg == 2
    assert conv_shape(p) == (3, 172, 2, 7) and (p.groups, p.per_group) == (16, 11)
    # the head split saturates at 32 for B = 497..512 and drops to 17 at 513: 33 k-tiles in chunks of 2,
    # the 17th slab one tile
    assert P.bwd_plan(A, 'a3c', 512).head_split == 32 and p.head_split == 17
    assert P.cdiv(515, P.BK) == 33 and P.gemm_kchunk(515, 32) == 2 * P.BK


NIPS_BWD = [
    # (algo, B, fork)            largest rel-L2 seen over the tensors: same-activation / independent
    ('a3c', 1, reaches_1),        # 2.7e-07 / 3.6e-07
    ('a3c', 16, reaches_16),      # 2.1e-07 / 3.8e-07
    ('a3c', 33, reaches_33),      # 2.1e-07 / 3.0e-07
    ('a3c', 65, reaches_65),      # 1.9e-07 / 4.9e-07
    ('a3c', 257, reaches_257),    # 2.4e-06 / 1.9e-05
    ('a3c', 515, reaches_515),    # 1.1e-07 / 2.5e-07
    ('q', 257, reaches_257),      # 1.5e-07 / 2.0e-07
]


@pytest.mark.parametrize('algo,B,reaches', NIPS_BWD, ids=[f'{a}-{b}' for a, b, _ in NIPS_BWD])
def test_nips_loss_backward_at_plan_forks(K, algo, B, reaches):
    """Net.loss_backward (the per-op C-ABI launches alone: k_conv_bwd<true, 8, true>, the slab form
    of the fc weight GEMM, k_slab_group + k_finalize) against the fp64 oracle."""
    reaches(P.bwd_plan(A, algo, B))
    check_loss_backward(K, algo, A, B, False)


@pytest.mark.parametrize('B', [16, 17])
def test_nips_forward_at_fc_tile_edge(K, B):
    """Net.forward with the fc forward's 16-row tile exactly full and one row over."""
    assert B in (P.BK, P.BK + 1)
    check_forward(K, 'a3c', A, B)


def dw_rows(B):
    return B * P.NT1_P, B * P.NT2_P, B * P.NT3_P


# largest rel-L2 seen over the tensors, same-activation / independent:
#   B = 31    6.8e-07 / 1.1e-02  (a ReLU mask of the fc output differs between the fp32 and the fp64 forward:
#                                 the trunk's eight tensors l1..l4 are off by 0.8e-2..1.1e-2, the heads' four by 4e-07)
#   B = 103   7.1e-07 / 7.3e-07
@pytest.mark.parametrize('B,layer', [(31, 0), (103, 1)])
def test_nature_forward_loss_backward_at_dw_chunk_forks(K, B, layer):
    """NatureNet.forward / loss_backward where dw_split's chunk first leaves 32 rows: conv1's at
    B = 31 (one batch earlier it is 32), conv2's from B = 102 on, taken at 103 where the last chunk
    of all three dW passes is ragged (at 102 conv2's and conv3's hold 6 rows; at 103, 112 / 23 / 55)."""
    p = P.nat_plan(A, B)
    before = {0: 30, 1: 101}[layer]
    assert P.nat_plan(A, before).kc[layer] == 32 and p.kc[layer] > 32
    assert p.kc == {31: (64, 32, 32), 103: (128, 64, 64)}[B]
    assert all(r % kc for r, kc in zip(dw_rows(B), p.kc))          # a ragged last chunk in every pass
    assert all((ns - 1) * kc < r for r, ns, kc in zip(dw_rows(B), p.ns, p.kc))
    check_nature_forward_loss_backward(K, A, B, False)


# ------------------------------------------------------------------ the engine, against the replay oracle
def reaches_261(p):      # E = 87, n = 3
    assert conv_shape(p) == (2, 131, 1, 0) and p.head_split == 17 and p.fc_split_slab == 3
    assert p.B <= P.FC_WKS_MAXB         # overlap: the in-workgroup split-K fc GEMM over K = 261


def test_engine_sync_a3c_short_last_workgroup():
    """E = 87, n = 3: the sync engine's DMA 8-wave k_conv_bwd with per_wg 2 and a one-sample last
    workgroup, nwg = 131 inside an engine.
    Largest rel-L2 seen: same-activation 4.4e-07, independent 3.2e-06."""
    reaches_261(P.bwd_plan(A, 'a3c', 3 * 87))
    check_sync_vs_oracle('a3c', A, 87, 3, 3, iters=3)


@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_engine_overlap_short_last_workgroup(algo):
    """E = 87, n = 3 on the overlap pipeline: the compact k_conv_bwd<false, 4, true> and the
    in-workgroup split-K fc weight GEMM (wg_split = 4), forms the per-op C-ABI cannot reach; q runs
    its late target forward over the n * E rows.
    Largest rel-L2 seen, same-activation / independent: a3c 3.7e-07 / 4.2e-04, q 1.2e-07 / 1.9e-04."""
    reaches_261(P.bwd_plan(A, algo, 3 * 87))
    check_overlap_vs_oracle(A, 87, 3, 3, rollouts=3, algo=algo)


def test_engine_overlap_a3c_per_wg_3():
    """E = 103, n = 5 (B = 515) on the overlap pipeline: per_wg 3, a two-sample last workgroup.
    Largest rel-L2 seen: same-activation 2.4e-07, independent 1.2e-04."""
    p = P.bwd_plan(A, 'a3c', 5 * 103)
    reaches_515(p)
    assert p.B <= P.FC_WKS_MAXB
    check_overlap_vs_oracle(A, 103, 5, 3, rollouts=3)


def test_engine_lstm_sync_ragged_env_tile():
    """The LSTM engine at E = 87, n = 3: a ragged last env tile of k_lstm_fwd / k_lstm_bptt_step
    (87 = 5 * 16 + 7) and the gate matrix's dW GEMM split 4 ways over 17 k-tiles (5, 5, 5, 2).
    Largest rel-L2 seen: same-activation 5.5e-07, independent 1.8e-06."""
    w = P.lstm_ws(3, 87)
    assert 87 % P.LSTM_TILE == 7 and w.split_dw == 4 and P.cdiv(3 * 87, P.BK) == 17
    assert P.gemm_kchunk(3 * 87, 4) == 5 * P.BK
    reaches_261(P.bwd_plan(A, 'a3c', 3 * 87))
    check_lstm_sync_vs_oracle(A, 87, 3, 3, iters=3, learning_rate=2e-3)
