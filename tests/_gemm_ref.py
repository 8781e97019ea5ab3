"""Inputs, float64 reference and the derived error bar of the direct GEMM tests (test_gpu_gemm.py on the
GPU, test_gemm_cpu.py for the bar's own power).  numpy only.

Inputs: every operand element is a random sign times a uniform draw from [0.5, 1], so every product
a_mk b_kn has magnitude >= 0.25.

Bar, per output element:  |C - C_ref| <= gamma_(K+2) (sum_k |a_mk| |b_kn| + |bias_n|),
gamma_n = n u / (1 - n u), u = 2^-23.  It is the standard bound of a length-K dot product summed in any
order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) with one more rounding for the bias;
u is one bit wider than fp32's unit roundoff so that nothing rests on how the matrix core rounds
inside an instruction.  While the largest bar of a case is below 0.125 -- half the smallest product --
one dropped, doubled or misplaced product cannot hide under it."""
import numpy as np

U = 2.0 ** -23
MIN_PRODUCT = 0.25

# (M, N, K): what each reaches is listed in DESIGN 4d-2
SHAPES = [(4, 4, 4), (68, 132, 36), (580, 72, 200), (132, 260, 520)]
# (a k-strided, b n-contiguous) only: K need not be a multiple of 4 there
SHAPES_K_ANY = [(68, 132, 1), (68, 132, 33)]
ALL_SHAPES = SHAPES + SHAPES_K_ANY
BK = 16                      # the kernels' k-tile


def gamma(n):
    return n * U / (1.0 - n * U)


def signed(rng, shape):
    """random sign times uniform [0.5, 1], float32"""
    mag = rng.uniform(0.5, 1.0, shape)
    return (np.where(rng.random(shape) < 0.5, -mag, mag)).astype(np.float32)


def make_inputs(M, N, K, seed=0):
    """dict: A [M,K], B [K,N], bias [N], mask [M,N] (positive, negative and exact-zero entries; keep where
    > 0), all float32"""
    rng = np.random.default_rng([seed, M, N, K])
    A, B, bias = signed(rng, (M, K)), signed(rng, (K, N)), signed(rng, (N,))
    mask = signed(rng, (M, N))
    mask[rng.random((M, N)) < 0.25] = 0.0
    return dict(A=A, B=B, bias=bias, mask=mask)


def reference(inp):
    """float64 from the same fp32 values: C = A B, absC = |A| |B|, colsum = sum_k B, abscol = sum_k |B|"""
    A, B = inp['A'].astype(np.float64), inp['B'].astype(np.float64)
    return dict(C=A @ B, absC=np.abs(A) @ np.abs(B), colsum=B.sum(0), abscol=np.abs(B).sum(0))


def bar_c(ref, K, bias=None):
    b = 0.0 if bias is None else np.abs(bias.astype(np.float64))[None, :]
    return gamma(K + 2) * (ref['absC'] + b)


def bar_colsum(ref, K):
    return gamma(K + 2) * ref['abscol']


def effective_split(K, nsplit):
    """the split a launch uses for `nsplit` requested: chunks of whole k-tiles, no empty chunk"""
    ktiles = (K + BK - 1) // BK
    per = (ktiles + nsplit - 1) // nsplit
    return (ktiles + per - 1) // per


def pack_maskbits(keep, ldm=None):
    """keep [M,N] bool -> uint32 [M, ldm] words, bit (n & 31) of word n >> 5 (ldm >= ceil(N/32) words)"""
    M, N = keep.shape
    words = (N + 31) // 32
    ldm = words if ldm is None else ldm
    assert ldm >= words
    out = np.zeros((M, ldm), np.uint32)
    for n in range(N):
        out[:, n >> 5] |= keep[:, n].astype(np.uint32) << np.uint32(n & 31)
    return out


def unpack_maskbits(bits, N):
    n = np.arange(N)
    return ((bits[:, n >> 5] >> (n & 31).astype(np.uint32)) & 1).astype(bool)


# ---- fp32 emulations of summation orders (product rounded to fp32, then every add rounded) ----------

def _outer(A, B, k):
    return A[:, k, None] * B[None, k, :]          # float32 x float32 -> float32


def sum_sequential(A, B, ks=None):
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in (range(A.shape[1]) if ks is None else ks):
        acc = acc + _outer(A, B, k)
    return acc


def sum_ktiles(A, B):
    """each 16-wide k-tile summed on its own, the tile sums then added in order"""
    K = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k0 in range(0, K, BK):
        acc = acc + sum_sequential(A, B, range(k0, min(K, k0 + BK)))
    return acc


def sum_chunks(A, B, nsplit=5):
    """split-K: K in `nsplit` chunks of whole k-tiles (the slabs), each sequential, folded in order"""
    K = A.shape[1]
    ktiles = (K + BK - 1) // BK
    per = (ktiles + nsplit - 1) // nsplit * BK
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k0 in range(0, K, per):
        acc = acc + sum_sequential(A, B, range(k0, min(K, k0 + per)))
    return acc


def sum_interleaved(A, B, groups=4):
    """group q sums k = q, q + groups, ...; the groups folded ((g0 + g1) + g2) + g3"""
    K = A.shape[1]
    acc = sum_sequential(A, B, range(0, K, groups))
    for q in range(1, groups):
        acc = acc + sum_sequential(A, B, range(q, K, groups))
    return acc


ORDERS = {'sequential': sum_sequential, 'ktiles16': sum_ktiles, 'chunks5': sum_chunks, 'interleaved4': sum_interleaved}


# ---- mutants: what a subtly wrong tile kernel computes (float64, so the mutation is the only error) -----

def mutant_drop_k(inp, ref, k):
    return ref['C'] - np.outer(inp['A'][:, k].astype(np.float64), inp['B'][k].astype(np.float64))


def mutant_double_k(inp, ref, k):
    return ref['C'] + np.outer(inp['A'][:, k].astype(np.float64), inp['B'][k].astype(np.float64))


def mutant_quad_from_next_row(inp, ref, k0):
    """the four A values of k-quad k0 .. k0+3 of every row read from the row below (last row: the first)"""
    A = inp['A'].astype(np.float64).copy()
    A[:, k0:k0 + 4] = np.roll(A, -1, axis=0)[:, k0:k0 + 4]
    return A @ inp['B'].astype(np.float64)


def mutant_skip_last_ktile(inp, ref):
    K = inp['A'].shape[1]
    k0 = (K - 1) // BK * BK
    return inp['A'][:, :k0].astype(np.float64) @ inp['B'][:k0].astype(np.float64)


def mutant_shift_column(inp, ref, n):
    """output column n holds its neighbour's value"""
    C = ref['C'].copy()
    C[:, n] = ref['C'][:, (n + 1) % C.shape[1]]
    return C


def mutant_bias_twice(inp, ref):
    return ref['C'] + 2.0 * inp['bias'].astype(np.float64)[None, :]
