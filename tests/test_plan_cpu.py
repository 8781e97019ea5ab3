"""tests/_plan.py (the backward's launch plans restated in Python) tied to the library, no GPU.

The workspace-size entry points of the C-ABI touch no device: each returns the `total` of the
plan the launch itself computes (a3c_bwd_plan, nat_plan + a3c_nat_fwd_ws_floats, lstm_ws), and
every plan choice that changes a buffer's size -- the head and fc split-K counts, nwg, the nature
trunk's dW chunk counts, the LSTM dW split -- moves that total.  So equality over the whole range
pins the restatement, from which the GPU case tables derive (tests/test_gpu_batch_edges.py).  The
rest of the file asserts the invariants the kernels' loops rely on, for every B."""
import ctypes
import os
import sys

import pytest

import _plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'async-rl-tensorflow_amd', 'lib', 'liba3c_hip.so')

WIDTHS = (1, 3, 6, 7, 8, 18, 31)
B_MAX = 6000


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))
    from src import _lib
    _lib.lib()
    return _lib


def lib_bytes(L, fn, *args):
    n = L.c_i64()
    assert getattr(L.lib(), fn)(*args, ctypes.byref(n)) == 0, (fn, L.lib().a3c_last_error())
    return int(n.value)


@pytest.mark.parametrize('algo', ['a3c', 'q'])
@pytest.mark.parametrize('A', WIDTHS)
def test_nips_workspace_is_the_restated_plan(L, algo, A):
    desc = L.net_desc(A, algo)
    assert L.z_stride(desc) == P.zs(algo, A)
    bad = [B for B in range(1, B_MAX + 1)
           if lib_bytes(L, 'a3c_workspace_bytes', ctypes.byref(desc), B) != P.workspace_bytes(A, algo, B)]
    assert not bad, bad[:8]
    # the plan must exceed the forward's PREP_BYTES floor somewhere in the range, or the equality
    # above says nothing about it: it does from B = 1 on (cgroup alone is 16 slabs)
    assert P.bwd_plan(A, algo, 1).total < P.PREP_BYTES // 4 < P.bwd_plan(A, algo, 64).total


@pytest.mark.parametrize('A', WIDTHS)
def test_nature_workspace_is_the_restated_plan(L, A):
    """(The nature trunk carries the A3C heads only: a3c_make_layout rejects q.)"""
    desc = L.net_desc(A, 'a3c', dqn_type='nature')
    bad = [B for B in range(1, B_MAX + 1)
           if lib_bytes(L, 'a3c_nature_workspace_bytes', ctypes.byref(desc), B) != P.nature_workspace_bytes(A, B)]
    assert not bad, bad[:8]
    qdesc = L.net_desc(A, 'q', dqn_type='nature')
    assert L.lib().a3c_nature_workspace_bytes(ctypes.byref(qdesc), 1, ctypes.byref(L.c_i64())) != 0
    # the backward's plan is the larger leg of the max at every B (it holds the forward's prepared
    # weights too), so the equality above does not pin the forward's size; only this ordering does
    assert all(P.nat_fwd_ws_floats(B) < P.nat_plan(A, B).total for B in (1, 17, 513, B_MAX))


def test_lstm_workspace_is_the_restated_plan(L):
    bad = [(n, E) for n in range(1, 9) for E in range(1, 601)
           if lib_bytes(L, 'a3c_lstm_workspace_bytes', n, E) != P.lstm_workspace_bytes(n, E)]
    assert not bad, bad[:8]


def test_gemm_split_helpers():
    """The two helpers against what the issue's case table quotes (head: M = 256, N = zs = 8,
    target 128 -> 4 tiles; fc: M = 2592, N = 256, target 512 -> 164 tiles)."""
    head = lambda B: P.gemm_effective_split(B, P.gemm_plan_split(P.FC, 8, B, 128))      # noqa: E731
    fc = lambda B: P.gemm_effective_split(B, P.gemm_plan_split(P.FLAT, P.FC, B, 512))   # noqa: E731
    assert [head(B) for B in (1, 16, 17, 496, 497, 512, 513)] == [1, 1, 2, 31, 32, 32, 17]
    assert P.gemm_kchunk(513, 32) == 32 and P.cdiv(513, 16) == 33      # 17 slabs, the last one tile
    assert [fc(B) for B in (1, 16, 17, 32, 33, 48, 49, 64, 65)] == [1, 1, 2, 2, 3, 3, 2, 2, 3]
    assert P.gemm_kchunk(65, 3) == 32                                   # slabs of 32, 32, 1 rows
    for K in range(1, 2000):
        for ns in (1, 2, 3, 4, 17, 32):
            eff, kc = P.gemm_effective_split(K, ns), P.gemm_kchunk(K, ns)
            assert 1 <= eff <= ns and (eff - 1) * kc < K <= eff * kc, (K, ns)


def regions_disjoint(regions, total):
    end = 0
    for name, off, floats in regions:
        assert off % 64 == 0 and off >= end and floats >= 0, name
        end = off + floats
    assert end <= total


@pytest.mark.parametrize('algo', ['a3c', 'q'])
@pytest.mark.parametrize('A', WIDTHS)
def test_nips_plan_invariants(algo, A):
    for B in range(1, B_MAX + 1):
        p = P.bwd_plan(A, algo, B)
        # every sample belongs to exactly one workgroup and no workgroup is empty
        assert 1 <= p.nwg <= P.CB_NWG_MAX and (p.nwg - 1) * p.per_wg < B <= p.nwg * p.per_wg, B
        last = P.wg_samples(p, p.nwg - 1)
        assert 1 <= last <= p.per_wg and (p.nwg - 1) * p.per_wg + last == B, B
        assert all(P.wg_samples(p, w) == p.per_wg for w in (0, p.nwg - 2) if 0 <= w < p.nwg - 1), B
        # every slab belongs to exactly one group (trailing groups may be empty: k_slab_group
        # then sums nothing and the finalize adds a zero)
        assert 1 <= p.groups <= P.CB_GROUPS_MAX and p.groups * p.per_group >= p.nwg, B
        assert sum(P.group_slabs(p, g) for g in range(p.groups)) == p.nwg, B
        assert 1 <= p.head_split <= 32 and 1 <= p.fc_split_slab <= 3, B
        regions_disjoint(p.regions, p.total)


@pytest.mark.parametrize('A', (1, 6, 31))
def test_nature_plan_invariants(A):
    for B in range(1, B_MAX + 1):
        p = P.nat_plan(A, B)
        for ns, kc, rows in zip(p.ns, p.kc, (B * P.NT1_P, B * P.NT2_P, B * P.NT3_P)):
            assert kc % 32 == 0 and kc >= 32 and (ns - 1) * kc < rows <= ns * kc, B
        regions_disjoint(p.regions, p.total)


def test_lstm_plan_invariants():
    for n in range(1, 9):
        for E in range(1, 601):
            w = P.lstm_ws(n, E)
            assert 1 <= w.split_dw <= 4
            regions_disjoint(w.regions, w.total)
