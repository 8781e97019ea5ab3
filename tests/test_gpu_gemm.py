"""The fp32 matrix-core GEMM (csrc/gemm.hip) alone, through a3c_gemm_f32 / a3c_gemm3_f32: every tile
form (64x64, 128x128, XCD-grouped ids, capped grids, slab split-K with its fold kernel, in-workgroup
split-K), the four operand layouts, the five epilogues and the column sums, at the smallest shapes
that reach each index path.

Every output element is held to the derived bar of tests/_gemm_ref.py against A @ B in float64 --
gamma_(K+2) (sum_k |a||b| + |bias|), which is below half the smallest product, so one dropped,
doubled or misplaced product fails (test_gemm_cpu.py shows that of the bar itself) -- and the claims of
gemm.h are asserted: tile size, tile order and grid cap change no bit at the same effective split; the
in-workgroup split is deterministic and independent of the tile order; the three-GEMM launch equals
three single launches.  Every buffer carries guard rows (the sentinel of tests/_net_parity.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _gemm_ref as G  # noqa: E402
from _net_parity import GUARD  # noqa: E402

TAIL = 64              # guard floats behind every float buffer
WS_EXCESS = 256        # guard bytes behind a workspace
WS_FILL = 0x5A
BITS_FILL = np.uint32(0xA5A5A5A5)
STORE, BIAS_RELU, BIAS, MASK, MASKBITS = range(5)
EPI_NAMES = ['store', 'bias_relu', 'bias', 'mask', 'maskbits']
LAYOUTS = [(False, True), (True, False), (True, True), (False, False)]     # (a k-contiguous, b n-contiguous)

# name -> a3c_gemm_desc fields.  Identity classes: everything but wks at one effective split; wks alone.
VARIANTS = [
    ('plain', {}),
    ('split2', dict(nsplit=2)), ('split3', dict(nsplit=3)), ('split5', dict(nsplit=5)),
    ('split6', dict(nsplit=6)), ('split8', dict(nsplit=8)),
    ('big', dict(big=1)), ('big_split2', dict(big=1, nsplit=2)), ('big_split5', dict(big=1, nsplit=5)),
    ('xcd1', dict(xcd=1)), ('xcd2', dict(xcd=2)),
    ('xcd1_split2', dict(xcd=1, nsplit=2)), ('xcd2_split2', dict(xcd=2, nsplit=2)),
    ('xcd1_split5', dict(xcd=1, nsplit=5)), ('xcd2_split3', dict(xcd=2, nsplit=3)),
    ('wgs1', dict(max_wgs=1)), ('wgs5', dict(max_wgs=5)), ('wgs5_split5', dict(max_wgs=5, nsplit=5)),
    ('xcd1_wgs5', dict(xcd=1, max_wgs=5)), ('xcd2_wgs1', dict(xcd=2, max_wgs=1)),
    ('xcd2_wgs5_split3', dict(xcd=2, max_wgs=5, nsplit=3)),
    ('wks', dict(wg_split=4)), ('wks_xcd1', dict(wg_split=4, xcd=1)),
]

RATIO_C, RATIO_COLSUM = {}, {}        # (variant, shape) -> largest error / bar seen (a record, not a bar)


@pytest.fixture(scope='module')
def KM():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def host_case(shape):
    """inputs and float64 reference of a shape: computed once, read-only"""
    inp = G.make_inputs(*shape)
    ref = G.reference(inp)
    for d in (inp, ref):
        for v in d.values():
            v.setflags(write=False)
    K = shape[2]
    assert G.bar_c(ref, K, inp['bias']).max() < G.MIN_PRODUCT / 2
    assert G.bar_colsum(ref, K).max() < 0.25
    return inp, ref


def cu(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()     # (a copy: the cached host arrays are read-only)


def place(mat, ld, fill=GUARD):
    """mat [R, W] at leading dimension ld in a flat buffer, TAIL elements longer; the padding columns and the
    tail hold the fill"""
    R, W = mat.shape
    host = np.full(R * ld + TAIL, fill, mat.dtype)
    host[:R * ld].reshape(R, ld)[:, :W] = mat
    return cu(host)


class Operands:
    """device operands of one (shape, layout), padded leading dimensions or tight ones"""

    def __init__(self, shape, a_kc, b_nc, padded):
        self.shape, self.a_kc, self.b_nc = shape, a_kc, b_nc
        M, N, K = shape
        inp, _ = host_case(shape)
        A, B = inp['A'], inp['B']
        a_mat = A if a_kc else A.T
        b_mat = B if b_nc else B.T
        self.lda = a_mat.shape[1] + (8 if padded else 0)
        self.ldb = b_mat.shape[1] + (4 if padded else 0)
        self.ldc = N + (5 if padded else 0)
        self.ldm = N + (3 if padded else 0)
        self.ldmw = (N + 31) // 32 + (1 if padded else 0)
        self.A, self.B = place(a_mat, self.lda), place(b_mat, self.ldb)
        self.bias = place(inp['bias'][None, :], N)
        self.mask = place(inp['mask'], self.ldm)
        words = np.full(M * self.ldmw + TAIL, BITS_FILL, np.uint32)
        words[:M * self.ldmw] = G.pack_maskbits(inp['mask'] > 0, self.ldmw).reshape(-1)
        self.bits = cu(words.view(np.int32))
        self.read_only = [self.A, self.B, self.bias, self.mask, self.bits]
        self.pristine = [t.clone() for t in self.read_only]

    def read_only_intact(self):
        return all(torch.equal(a, b) for a, b in zip(self.read_only, self.pristine))


class Run:
    pass


def launch(KM, op, epi, colsum_on, var):
    """one a3c_gemm_f32 launch into fresh guarded buffers; asserts every guard, returns the buffers"""
    M, N, K = op.shape
    want = 1 if var.get('wg_split') else G.effective_split(K, var.get('nsplit', 1))
    q_eff, q_bytes = KM.gemm_workspace(M, N, K, var.get('nsplit', 1))
    assert q_eff == G.effective_split(K, var.get('nsplit', 1))
    assert q_bytes == (q_eff * M * N * 4 if q_eff > 1 else 0)
    need = 0 if var.get('wg_split') else q_bytes
    ws = torch.full((need + WS_EXCESS,), WS_FILL, dtype=torch.uint8, device='cuda')
    C = torch.full(((M + 1) * op.ldc,), GUARD, dtype=torch.float32, device='cuda')
    colsum = torch.full((want * N + TAIL,), GUARD, dtype=torch.float32, device='cuda') if colsum_on else None
    d = KM.gemm_desc(op.A, op.B, C, M, N, K, op.a_kc, op.b_nc, op.lda, op.ldb, op.ldc, epi=epi,
                     bias=op.bias if epi in (BIAS, BIAS_RELU) else None, mask=op.mask if epi == MASK else None,
                     maskbits=op.bits if epi == MASKBITS else None, ldm=op.ldmw if epi == MASKBITS else op.ldm,
                     colsum=colsum, **var)
    eff = KM.gemm(d, ws, workspace_bytes=need)
    assert eff == want, (eff, want)        # the launch's split == the query's (1 with wg_split)
    r = Run()
    r.C, r.colsum, r.eff = C, colsum, eff
    Ch = C.cpu().numpy().reshape(M + 1, op.ldc)
    assert np.array_equal(Ch[M], np.full(op.ldc, GUARD, np.float32)), 'row M of C written'
    assert np.array_equal(Ch[:M, N:], np.full((M, op.ldc - N), GUARD, np.float32)), 'columns N.. of C written'
    r.Ch = Ch[:M, :N]
    if colsum_on:
        ch = colsum.cpu().numpy()
        assert np.array_equal(ch[eff * N:], np.full(TAIL, GUARD, np.float32)), 'past the colsum rows written'
        r.colsum_rows = ch[:eff * N].reshape(eff, N)
    assert bool((ws[need:] == WS_FILL).all()), 'past the workspace written'
    assert op.read_only_intact(), 'a read-only operand buffer written'
    return r


def expected(shape, epi):
    """(float64 expectation, bar, keep or None) of an epilogue"""
    inp, ref = host_case(shape)
    K = shape[2]
    bias = inp['bias'].astype(np.float64)[None, :]
    if epi == STORE:
        return ref['C'], G.bar_c(ref, K), None
    if epi == BIAS:
        return ref['C'] + bias, G.bar_c(ref, K, inp['bias']), None
    if epi == BIAS_RELU:
        return np.maximum(ref['C'] + bias, 0.0), G.bar_c(ref, K, inp['bias']), None
    keep = inp['mask'] > 0
    return np.where(keep, ref['C'], 0.0), G.bar_c(ref, K), keep


def check_values(name, shape, epi, r):
    exp, bar, keep = expected(shape, epi)
    err = np.abs(r.Ch.astype(np.float64) - exp)
    ratio = float((err / bar).max())
    RATIO_C[name, shape] = max(RATIO_C.get((name, shape), 0.0), ratio)
    assert (err <= bar).all(), f'{name} {EPI_NAMES[epi]}: {int((err > bar).sum())} elements outside the bar, ' \
                               f'largest error / bar {ratio:.3g} at {np.unravel_index((err / bar).argmax(), err.shape)}'
    if keep is not None:
        assert not r.Ch[~keep].any(), f'{name}: masked-out elements must be exactly 0.0'
    if r.colsum is not None:
        _, ref = host_case(shape)
        cb = G.bar_colsum(ref, shape[2])
        cerr = np.abs(r.colsum_rows.astype(np.float64).sum(0) - ref['colsum'])
        RATIO_COLSUM[name, shape] = max(RATIO_COLSUM.get((name, shape), 0.0), float((cerr / cb).max()))
        assert (cerr <= cb).all(), f'{name}: colsum outside the bar, largest error / bar {float((cerr / cb).max()):.3g}'


CASES = [(s, l) for s in G.SHAPES for l in LAYOUTS] + [(s, LAYOUTS[0]) for s in G.SHAPES_K_ANY]
CASE_IDS = ['%dx%dx%d-a%s-b%s' % (*s, 'k' if l[0] else 'm', 'n' if l[1] else 'k') for s, l in CASES]
# leading dimensions larger than the logical widths at these shapes (every layout meets two of them)
PADDED = {(68, 132, 36), (132, 260, 520), (68, 132, 33)}


@pytest.mark.parametrize('shape,layout', CASES, ids=CASE_IDS)
def test_every_variant_and_epilogue(KM, shape, layout):
    op = Operands(shape, layout[0], layout[1], shape in PADDED)
    if shape == (68, 132, 36):
        exp, _, _ = expected(shape, BIAS_RELU)
        assert 0.3 < (exp == 0).mean() < 0.7            # about half the outputs are clipped
    for epi in range(5):
        first = {}                                      # effective split -> (variant, run): the identity class
        for name, var in VARIANTS:
            r = launch(KM, op, epi, True, var)
            check_values(name, shape, epi, r)
            if var.get('wg_split'):
                key = 'wks'
                again = launch(KM, op, epi, True, var)   # deterministic: equal to itself across two runs
                assert torch.equal(again.C, r.C) and torch.equal(again.colsum, r.colsum), f'{name}: two runs differ'
            else:
                key = r.eff
            if key in first:
                n0, r0 = first[key]
                assert torch.equal(r.C, r0.C), f'{name} != {n0} bit for bit ({EPI_NAMES[epi]}, split {key})'
                assert torch.equal(r.colsum, r0.colsum), f'colsum: {name} != {n0} bit for bit (split {key})'
            else:
                first[key] = (name, r)
            if epi == STORE:                            # the column sums change no bit of C
                bare = launch(KM, op, epi, False, var)
                assert torch.equal(bare.C, r.C), f'{name}: C differs with colsum off'
        assert set(first) >= {1, 'wks'}


def test_effective_split_query_host_only():
    """(e) the workspace query's split is gemm_setup's rule, and its bytes the slabs', with no launch"""
    from src import kernels as KM
    for Kd in (1, 15, 16, 17, 33, 200, 520):
        for ns in range(1, 41):
            eff, nbytes = KM.gemm_workspace(68, 132, Kd, ns)
            assert eff == G.effective_split(Kd, ns), (Kd, ns)
            assert nbytes == (eff * 68 * 132 * 4 if eff > 1 else 0)


def test_launch_reports_the_query_split(KM):
    """(e) with launches: what gemm_setup chose == the query, requested splits 1..40, on one 4 x 4 tile"""
    M = N = 4
    rng = np.random.default_rng(7)
    for Kd in (1, 15, 16, 17, 33, 200, 520):
        A, B = G.signed(rng, (M, Kd)), G.signed(rng, (Kd, N))
        ref = A.astype(np.float64) @ B.astype(np.float64)
        bar = G.gamma(Kd + 2) * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
        dA, dB = cu(A.T), cu(B)
        ws = torch.empty(40 * M * N, dtype=torch.float32, device='cuda')
        C = torch.empty(M, N, dtype=torch.float32, device='cuda')
        for ns in range(1, 41):
            q_eff, q_bytes = KM.gemm_workspace(M, N, Kd, ns)
            C.fill_(GUARD)
            eff = KM.gemm(KM.gemm_desc(dA, dB, C, M, N, Kd, False, True, M, N, N, nsplit=ns), ws, workspace_bytes=q_bytes)
            assert eff == q_eff, (Kd, ns, eff, q_eff)
            assert (np.abs(C.cpu().numpy().astype(np.float64) - ref) <= bar).all(), (Kd, ns)


@pytest.mark.parametrize('splits', [(1, 1, 1), (2, 5, 2), (3, 8, 13)])
def test_three_gemm_launch_equals_three_launches(KM, splits):
    """(c) a3c_gemm3_f32 (one launch, then the folds) == three a3c_gemm_f32, bit for bit"""
    # the synchronous backward's forms: two weight gradients with column sums, dl2 with the ReLU mask
    specs = [((68, 132, 33), LAYOUTS[0], STORE, True), ((132, 260, 520), LAYOUTS[0], STORE, True),
             ((580, 72, 200), LAYOUTS[1], MASKBITS, False)]
    ops = [Operands(s, l[0], l[1], True) for s, l, _, _ in specs]

    def buffers():
        out = []
        for (shape, _, epi, cs), op, ns in zip(specs, ops, splits):
            M, N, K = shape
            eff, nbytes = KM.gemm_workspace(M, N, K, ns)
            ws = torch.full((nbytes + WS_EXCESS,), WS_FILL, dtype=torch.uint8, device='cuda')
            C = torch.full(((M + 1) * op.ldc,), GUARD, dtype=torch.float32, device='cuda')
            colsum = torch.full((eff * N + TAIL,), GUARD, dtype=torch.float32, device='cuda') if cs else None
            d = KM.gemm_desc(op.A, op.B, C, M, N, K, op.a_kc, op.b_nc, op.lda, op.ldb, op.ldc, epi=epi,
                             maskbits=op.bits if epi == MASKBITS else None, ldm=op.ldmw, colsum=colsum, nsplit=ns)
            out.append((d, ws, C, colsum, eff, nbytes))
        return out

    one = buffers()
    effs = KM.gemm3([b[0] for b in one], [b[1] for b in one])
    three = buffers()
    for (d, ws, _, _, eff, nbytes), e3 in zip(three, effs):
        assert KM.gemm(d, ws, workspace_bytes=nbytes) == eff == e3
    for (shape, _, epi, cs), op, a, b in zip(specs, ops, one, three):
        M, N, K = shape
        assert torch.equal(a[2], b[2]), f'{shape}: C of the three-GEMM launch differs'
        assert bool((a[1][a[5]:] == WS_FILL).all()) and op.read_only_intact()
        r = Run()
        r.C, r.colsum, r.eff = a[2], a[3], a[4]
        Ch = a[2].cpu().numpy().reshape(M + 1, op.ldc)
        assert (Ch[M] == GUARD).all() and (Ch[:M, N:] == GUARD).all()
        r.Ch = Ch[:M, :N]
        if cs:
            assert torch.equal(a[3], b[3]), f'{shape}: colsum of the three-GEMM launch differs'
            ch = a[3].cpu().numpy()
            assert (ch[a[4] * N:] == GUARD).all()
            r.colsum_rows = ch[:a[4] * N].reshape(a[4], N)
        check_values('gemm3', shape, epi, r)


def test_rejections_launch_nothing(KM):
    """(g) every documented rejection: A3C_ERR_INVALID, a3c_last_error names the entry point, and neither C nor
    the column sums are touched"""
    from src import _lib
    M, N, K = 68, 132, 36
    inp, _ = host_case((M, N, K))
    big = cu(np.concatenate([inp['A'].reshape(-1), inp['B'].reshape(-1), np.zeros(4096, np.float32)]))
    C = torch.full((M * N + TAIL,), GUARD, dtype=torch.float32, device='cuda')
    colsum = torch.full((8 * N,), GUARD, dtype=torch.float32, device='cuda')
    ws = torch.empty(8 * M * N, dtype=torch.float32, device='cuda')
    bias, mask = cu(inp['bias']), cu(inp['mask'])
    bits = cu(G.pack_maskbits(inp['mask'] > 0).view(np.int32))

    def desc(akc=True, bnc=True, **kw):
        f = dict(A=big, B=big[M * K:], C=C, M=M, N=N, K=K, a_kcontig=akc, b_ncontig=bnc, colsum=colsum)
        f.update(kw)
        f.setdefault('lda', f['K'] if akc else f['M'])
        f.setdefault('ldb', f['N'] if bnc else f['K'])
        f.setdefault('ldc', f['N'])
        return KM.gemm_desc(**f)

    def rejected(d, workspace=ws, fn='a3c_gemm_f32', why='', **kw):
        with pytest.raises(_lib.A3CError) as e:
            KM.gemm(d, workspace, **kw) if fn == 'a3c_gemm_f32' else KM.gemm3(d, workspace)
        assert e.value.rc == _lib.ERR_INVALID
        msg = _lib.lib().a3c_last_error().decode()
        assert msg.startswith(fn + ':') and why in msg, msg

    KM.gemm(desc(), ws)                                   # the base description is valid ...
    torch.cuda.synchronize()
    assert not bool((C[:M * N] == GUARD).any())
    C.fill_(GUARD)
    colsum.fill_(GUARD)                                   # ... and from here on nothing may be written
    for null in ('A', 'B', 'C'):
        rejected(desc(**{null: None}))
    rejected(desc(A=big[1:]), why='16-byte')                             # 4-byte aligned operands
    rejected(desc(B=big[M * K + 2:]), why='16-byte')
    # (leading dimensions kept legal, so that each of these meets its own % 4 rule)
    rejected(desc(True, True, K=34, lda=36), why='K must')           # K % 4 unless (a k-strided, b n-contiguous)
    rejected(desc(True, False, K=34, lda=36, ldb=36), why='K must')
    rejected(desc(False, False, K=34, ldb=36), why='K must')
    rejected(desc(False, True, M=66, lda=68), why='M must')           # M % 4 when a is k-strided
    rejected(desc(False, True, N=130, ldb=132, ldc=132), why='N must')  # N % 4 when b is n-contiguous
    rejected(desc(True, True, N=130, ldb=132, ldc=132), why='N must')
    rejected(desc(lda=K + 1), why='multiples of 4')
    rejected(desc(ldb=N + 2), why='multiples of 4')
    rejected(desc(lda=K - 4))                             # shorter than a row
    rejected(desc(ldc=N - 1))
    rejected(desc(nsplit=2), None, why='needs a workspace')                        # split-K without a workspace
    rejected(desc(nsplit=3), ws, workspace_bytes=3 * M * N * 4 - 4, why='too small')
    rejected(desc(nsplit=0))
    for w in (1, 2, 3, 8, -4):
        rejected(desc(wg_split=w), why='wg_split: 0 or 4')
    rejected(desc(wg_split=4, xcd=2), why='wg_split: xcd')
    rejected(desc(xcd=3))
    rejected(desc(max_wgs=-1))
    for k in (0, -4):
        rejected(desc(K=k, lda=4, ldb=N), why='K < 1')
        rejected(desc(False, True, K=k), why='K < 1')
        rejected(desc(K=k, wg_split=4, lda=4), why='K < 1')
    rejected(desc(M=0))
    rejected(desc(N=0, ldb=4, ldc=4))
    rejected(desc(epi=5))
    rejected(desc(epi=BIAS))
    rejected(desc(epi=BIAS_RELU))
    rejected(desc(epi=MASK, ldm=N))
    rejected(desc(epi=MASKBITS, ldm=5))
    rejected(desc(epi=MASK, mask=mask, ldm=N - 1))
    rejected(desc(epi=MASKBITS, maskbits=bits, ldm=4))    # 132 columns are 5 words
    with pytest.raises(_lib.A3CError):
        KM.gemm_workspace(M, N, 0, 2)
    assert _lib.lib().a3c_last_error().decode().startswith('a3c_gemm_workspace_bytes:')
    # the three-GEMM launch: its fixed layouts, its own name, and one bad GEMM stops all three
    g = [desc(False, True), desc(False, True), desc(True, False)]
    rejected([g[0], g[1], desc(True, True)], [ws, ws, ws], fn='a3c_gemm3_f32')
    rejected([g[2], g[1], g[2]], [ws, ws, ws], fn='a3c_gemm3_f32')
    rejected([g[0], desc(False, True, K=0), g[2]], [ws, ws, ws], fn='a3c_gemm3_f32')
    rejected([g[0], desc(False, True, xcd=1), g[2]], [ws, ws, ws], fn='a3c_gemm3_f32')
    rejected([g[0], g[1], desc(True, False, nsplit=2)], [ws, ws, None], fn='a3c_gemm3_f32')
    torch.cuda.synchronize()
    assert bool((C == GUARD).all()) and bool((colsum == GUARD).all())
    KM.gemm(desc(bias=bias, epi=BIAS), ws)                # and the entry point still works afterwards
    torch.cuda.synchronize()
    assert not bool((C[:M * N] == GUARD).any()) and bool((C[M * N:] == GUARD).all())


def test_zz_error_over_bar_table():
    """the record for DESIGN 4d-2 (run with -s): largest error / bar per variant and shape, over every layout and
    epilogue above; C, then the column sums"""
    for title, rec in (('C', RATIO_C), ('colsum', RATIO_COLSUM)):
        shapes = sorted({s for _, s in rec}, key=lambda s: (s[2], s))
        print('\n%-18s' % (title + ' error / bar') + ''.join('%14s' % 'x'.join(map(str, s)) for s in shapes))
        for name in [n for n, _ in VARIANTS] + ['gemm3']:
            if any(n == name for n, _ in rec):
                print('%-18s' % name + ''.join('%14s' % ('%.4f' % rec[name, s] if (name, s) in rec else '-') for s in shapes))
    assert RATIO_C and all(v <= 1.0 for v in RATIO_C.values()) and all(v <= 1.0 for v in RATIO_COLSUM.values())
