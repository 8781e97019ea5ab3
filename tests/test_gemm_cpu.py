"""The check of test_gpu_gemm.py's check, without a GPU: the derived bar of tests/_gemm_ref.py admits
every legitimate fp32 summation order on the test's own inputs and rejects every single-product
mistake, at every shape the GPU test uses."""
import numpy as np
import pytest

import _gemm_ref as G


@pytest.fixture(scope='module')
def cases():
    out = {}
    for shape in G.ALL_SHAPES:
        inp = G.make_inputs(*shape)
        out[shape] = (inp, G.reference(inp))
    return out


IDS = ['x'.join(map(str, s)) for s in G.ALL_SHAPES]


@pytest.mark.parametrize('shape', G.ALL_SHAPES, ids=IDS)
def test_inputs_are_signed_half_to_one(cases, shape):
    inp, _ = cases[shape]
    for k in ('A', 'B', 'bias'):
        a = np.abs(inp[k])
        assert inp[k].dtype == np.float32 and a.min() >= 0.5 and a.max() <= 1.0
        assert (inp[k] < 0).any() or inp[k].size < 8
    m = inp['mask']
    if m.size >= 64:
        assert (m > 0).any() and (m < 0).any() and (m == 0).any()
    prod = np.abs(inp['A'].astype(np.float64))[:, :, None] * np.abs(inp['B'].astype(np.float64))[None] \
        if inp['A'].size * shape[1] < 1 << 22 else None
    if prod is not None:
        assert prod.min() >= G.MIN_PRODUCT


@pytest.mark.parametrize('shape', G.ALL_SHAPES, ids=IDS)
def test_largest_bar_is_below_half_the_smallest_product(cases, shape):
    inp, ref = cases[shape]
    K = shape[2]
    assert G.bar_c(ref, K, inp['bias']).max() < G.MIN_PRODUCT / 2
    assert G.bar_colsum(ref, K).max() < 0.5 / 2          # (a dropped |b| is >= 0.5)
    # whatever the draw: at most gamma_(K+2) (K + 1), 0.033 at K = 520
    assert G.gamma(K + 2) * (K + 1) < G.MIN_PRODUCT / 2


@pytest.mark.parametrize('order', sorted(G.ORDERS))
@pytest.mark.parametrize('shape', G.ALL_SHAPES, ids=IDS)
def test_fp32_summation_orders_stay_within_the_bar(cases, shape, order):
    inp, ref = cases[shape]
    K = shape[2]
    C = G.ORDERS[order](inp['A'], inp['B'])
    assert C.dtype == np.float32
    assert (np.abs(C.astype(np.float64) - ref['C']) <= G.bar_c(ref, K)).all()
    Cb = C + inp['bias'][None, :]
    assert Cb.dtype == np.float32
    assert (np.abs(Cb.astype(np.float64) - (ref['C'] + inp['bias'].astype(np.float64))) <= G.bar_c(ref, K, inp['bias'])).all()


def test_orders_differ_so_the_bar_is_not_vacuous(cases):
    inp, _ = cases[(132, 260, 520)]
    assert not np.array_equal(G.sum_sequential(inp['A'], inp['B']), G.sum_chunks(inp['A'], inp['B']))


@pytest.mark.parametrize('shape', G.ALL_SHAPES, ids=IDS)
def test_mutants_exceed_the_bar(cases, shape):
    inp, ref = cases[shape]
    M, N, K = shape
    bar = G.bar_c(ref, K)
    bar_b = G.bar_c(ref, K, inp['bias'])

    def over(C, b=bar, target=ref['C']):
        return np.abs(C - target) > b

    for k in sorted({0, K // 2, K - 1}):
        # every output element holds product k: each one must miss
        assert over(G.mutant_drop_k(inp, ref, k)).all()
        assert over(G.mutant_double_k(inp, ref, k)).all()
    for k0 in sorted({0, (K - 1) // 4 * 4}):
        if M > 1:
            assert over(G.mutant_quad_from_next_row(inp, ref, k0)).any()
    assert over(G.mutant_skip_last_ktile(inp, ref)).any()
    for n in sorted({0, N - 2, N - 1}):
        assert over(G.mutant_shift_column(inp, ref, n))[:, n].any()
    with_bias = ref['C'] + inp['bias'].astype(np.float64)[None, :]
    assert over(G.mutant_bias_twice(inp, ref), bar_b, with_bias).all()
    # the column sums: one dropped row of B
    cs = ref['colsum'] - inp['B'][K // 2].astype(np.float64)
    assert (np.abs(cs - ref['colsum']) > G.bar_colsum(ref, K)).all()


@pytest.mark.parametrize('N', [1, 31, 32, 33, 132, 260])
def test_maskbits_round_trip(N):
    rng = np.random.default_rng(N)
    mask = G.signed(rng, (7, N))
    mask[rng.random((7, N)) < 0.25] = 0.0
    keep = mask > 0
    for ldm in ((N + 31) // 32, (N + 31) // 32 + 1):
        bits = G.pack_maskbits(keep, ldm)
        assert bits.dtype == np.uint32 and bits.shape == (7, ldm)
        assert np.array_equal(G.unpack_maskbits(bits, N), keep)
        # nothing set past column N
        tail = np.arange(N, ldm * 32)
        assert not ((bits[:, tail >> 5] >> (tail & 31).astype(np.uint32)) & 1).any()


C_PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "a3c_hip.h"
#define F(m) printf(#m " %zu\n", offsetof(a3c_gemm_desc, m));
int main(void) {
  printf("sizeof %zu\n", sizeof(a3c_gemm_desc));
  F(A) F(lda) F(B) F(ldb) F(C) F(ldc) F(bias) F(mask) F(maskbits) F(ldm) F(colsum) F(M) F(N) F(K)
  F(a_kcontig) F(b_ncontig) F(epi) F(nsplit) F(wg_split) F(big) F(xcd) F(max_wgs)
  printf("codes %d %d %d %d %d\n", A3C_GEMM_STORE, A3C_GEMM_BIAS_RELU, A3C_GEMM_BIAS, A3C_GEMM_MASK, A3C_GEMM_MASKBITS);
  return 0;
}
'''


def test_gemm_desc_layout_matches_gcc(tmp_path):
    """the ctypes mirror of a3c_gemm_desc field by field, and the epilogue codes"""
    import ctypes
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / 'probe.c').write_text(C_PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(root, 'include'), str(tmp_path / 'probe.c'), '-o', str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    sys.path.insert(0, os.path.join(root, 'async-rl-tensorflow_amd'))
    from src import _lib
    got = dict(line.split(' ', 1) for line in out)
    assert int(got.pop('sizeof')) == ctypes.sizeof(_lib.GemmDesc)
    assert got.pop('codes').split() == [str(v) for v in (_lib.GEMM_STORE, _lib.GEMM_BIAS_RELU, _lib.GEMM_BIAS,
                                                        _lib.GEMM_MASK, _lib.GEMM_MASKBITS)]
    assert list(got) == [f[0] for f in _lib.GemmDesc._fields_]
    for name, off in got.items():
        assert getattr(_lib.GemmDesc, name).offset == int(off), name


def test_effective_split_rule():
    # 33 k-tiles: 5 asked keeps 5 (per = 7, the last chunk ragged), 6 keeps 6 (per = 6, the last chunk 3 tiles),
    # 8 asked drops to 7 (per = 5)
    assert [G.effective_split(520, s) for s in (5, 6, 8)] == [5, 6, 7]
    assert G.effective_split(36, 4) == 3 and G.effective_split(4, 5) == 1
    for K in (1, 15, 16, 17, 33, 200, 520):
        for ns in range(1, 41):
            eff = G.effective_split(K, ns)
            ktiles = (K + 15) // 16
            per = (ktiles + ns - 1) // ns
            assert 1 <= eff <= min(ns, ktiles) and (eff - 1) * per < ktiles <= eff * per
