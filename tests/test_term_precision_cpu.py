"""The bf16 term-split scheme in emulation (tests/_term_split.py), without a GPU: the number format
against torch's, the split's exactness, and -- on the short-chain inputs the GPU tests use -- for
every pass the honest fp32 chain's error, the mildest mutant's, the condition e_mut >= 9 e_honest
that makes sqrt(e_honest e_mut) a bar, and that the full product list passes the bar while every
mutant fails it.  Run with -s for the table."""
import functools

import numpy as np
import pytest

import _term_split as T
from oracle import ref_cpu as R

torch = pytest.importorskip('torch')

# (trunk, algo, A): the GPU tests' configurations
CONFIGS = [('nips', 'a3c', 6), ('nips', 'q', 6), ('nips', 'a3c', 18), ('nature', 'a3c', 6)]
IDS = ['-'.join(map(str, c)) for c in CONFIGS]
SEED = 7


def test_bf16_rn_matches_torch():
    """1e6 random bit patterns (NaNs and infinities among them) plus the edges: +-0, subnormals,
    ties to even in both directions, roundings that carry into the exponent and up to infinity."""
    rng = np.random.default_rng(0)
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00007FFF, 0x00008000, 0x00008001,
                     0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0x3F808000, 0x3F818000,
                     0x3F808001, 0x3FFFFFFF, 0x3FFF8000, 0xBFFF8000, 0x3F7FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)
    sub = rng.integers(0, 1 << 23, 50_000, dtype=np.uint32) | (rng.integers(0, 2, 50_000, dtype=np.uint32) << 31)
    # mantissa 1111111.1x: rounds up into the exponent (0 -> the smallest normal, 254 -> infinity)
    sign = rng.integers(0, 2, 50_000, dtype=np.uint32) << 31
    carry = sign | (rng.integers(0, 255, 50_000, dtype=np.uint32) << 23) | np.uint32(0x007F8000) | \
        rng.integers(0, 1 << 15, 50_000, dtype=np.uint32)
    bits = np.concatenate([edge, sub, carry, rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = T.bf16_bits(x).astype(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(T.bf16_rn(x)[nan]).all()
    assert np.isnan(torch.from_numpy(x[nan].copy()).to(torch.bfloat16).float().numpy()).all()
    assert nan.sum() > 1000 and (np.abs(x[~nan]) < 1.2e-38).sum() > 50_000
    # the carry cases did carry: the rounded exponent is the input's + 1
    c = carry.view(np.float32)
    assert (((T.bf16_bits(c) >> 7) & 0xFF) == ((carry >> 23) & 0xFF) + 1).all()
    assert np.array_equal(T.bf16_rn(x[~nan]).view(np.uint32) >> 16, T.bf16_bits(x[~nan]))


def test_split3_carries_fp32():
    """|x - (hi + mid + lo)| <= 2^-24 |x| on normal inputs (in fact 0: three signed 8-bit terms
    hold 24 bits), the terms are bf16 values, and each is at most half an ulp of the one above."""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(400_000) * np.exp2(rng.integers(-60, 60, 400_000))).astype(np.float32)
    x = np.concatenate([x, np.float32([1.0, -1.0, 255.0, 1.0 / 255.0, 0.0, 3.0e38, 1.5e-30])])
    hi, mid, lo = T.split3(x)
    for t in (hi, mid, lo):
        assert np.array_equal(T.bf16_rn(t), t)
    s = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert (np.abs(x.astype(np.float64) - s) <= 2.0 ** -24 * np.abs(x)).all()
    assert (np.abs(mid) <= 2.0 ** -8 * np.abs(hi)).all() and (np.abs(lo) <= 2.0 ** -8 * np.abs(mid) + 1e-45).all()
    assert np.array_equal(s, x.astype(np.float64))


def test_emulate_sums_the_listed_products():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((5, 37)).astype(np.float32)
    B = rng.standard_normal((37, 3)).astype(np.float32)
    At, Bt = T.terms_of(A, 3), T.terms_of(B, 3)
    all9 = [(i, j) for i in range(3) for j in range(3)]
    np.testing.assert_allclose(T.emulate(At, Bt, all9), A.astype(np.float64) @ B.astype(np.float64), rtol=0, atol=1e-13)
    six = T.emulate(At, Bt, T.PRODUCTS6)
    assert T.rel_l2(six, A.astype(np.float64) @ B.astype(np.float64)) < 2.0 ** -23
    for m, ij in T.mutants_of(3).items():
        rest = [p for p in T.PRODUCTS6 if p != ij]
        np.testing.assert_array_equal(T.emulate(At, Bt, rest), six - At[ij[0]] @ Bt[ij[1]])
    pix = rng.integers(0, 256, (4, 16)).astype(np.float32)
    assert len(T.terms_of(pix, 1)) == 1
    with pytest.raises(AssertionError):
        T.terms_of(A, 1)
    # the honest chain is the sequential fp32 FMA chain
    acc = np.zeros((5, 3), np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for k in range(37):
        acc = (acc.astype(np.float64) + np.outer(A64[:, k], B64[k])).astype(np.float32)
    np.testing.assert_array_equal(T.chain_fp32(A, B), acc)


@functools.lru_cache(maxsize=None)
def setup(dqn_type, algo, A):
    ns = R.param_shapes(A, algo, dqn_type)
    P = T.sparse_params(ns, algo, dqn_type, SEED)
    return ns, P


def test_sparse_params_are_short_chains():
    for dqn_type, algo, A in CONFIGS:
        ns, P = setup(dqn_type, algo, A)
        convs, flat, fc = R.trunk_spec(dqn_type)
        for i, c in enumerate(convs):
            w = P[f'l{i + 1}_w'].reshape(-1, c['cout'])
            assert ((w != 0).sum(0) == T.NNZ).all()
        w = P[T.fc_name(algo) + '_w']
        assert ((w != 0).sum(0) == T.NNZ).all()
        rows = np.flatnonzero((w != 0).any(1))
        assert len(set(rows // convs[-1]['cout'])) == 2              # two spatial positions
        for k, shp in ns:
            assert P[k].shape == tuple(shp) and P[k].dtype == np.float32
        assert (T.head_wb(P, algo)[0] != 0).all()


@pytest.mark.parametrize('dqn_type,algo,A', CONFIGS, ids=IDS)
def test_forward_bars(dqn_type, algo, A):
    """B = 2.  Per layer: the activation is alive; per term-split layer e_mut >= 9 e_honest, the
    full scheme inside the bar and every mutant outside."""
    ns, P = setup(dqn_type, algo, A)
    states = R.states_nhwc(T.dense_states(2, SEED + 1))
    _, outs = T.forward_emulated(P, states, algo, dqn_type)
    res = T.forward_check(P, states, outs, algo, dqn_type)
    for layer, (b, err, case) in res.items():
        print(T.fmt(f'{dqn_type} {layer}', b))
        T.assert_alive(layer, outs[layer])
        T.assert_design((dqn_type, algo, layer), b)
        assert err == b['e_honest']
        assert case.real == (layer in T.REAL_PASSES[dqn_type]['fwd'])
        assert case.na == (1 if layer == 'conv1' else 3)
    # the per-layer fp64 references chain up to ref_cpu.forward
    ref = R.forward(P, states, algo, dqn_type)
    assert T.rel_l2(outs['head'], ref['z']) < 1e-5


@functools.lru_cache(maxsize=None)
def backward_setup(dqn_type, algo, A):
    ns, P = setup(dqn_type, algo, A)
    planes = T.dense_states(1, SEED + 2)
    states = R.states_nhwc(planes)
    _, outs = T.forward_emulated(P, states, algo, dqn_type)
    z = outs['head'].astype(np.float64)
    if algo == 'a3c':
        _, dz = R.a3c_loss_and_dz(z, np.array([1]), np.array([0.7]))
    else:
        _, dz = R.q_loss_and_dz(z, np.array([1]), np.array([0.7]))
    return P, states, outs, T.backward_check(P, states, outs, dz, algo, dqn_type)


@pytest.mark.parametrize('dqn_type,algo,A', CONFIGS, ids=IDS)
def test_backward_chain_is_the_oracle(dqn_type, algo, A):
    P, states, outs, chk = backward_setup(dqn_type, algo, A)
    g = T.backward_chain(P, chk['fwd'], chk['dz'], algo, dqn_type, T.mm_fp64)
    assert set(g) == set(T.grad_feeds(algo, dqn_type))
    for k in g:
        assert T.rel_l2(g[k].reshape(-1), chk['g_ref'][k].reshape(-1)) < 1e-13, k
        assert np.linalg.norm(g[k]) > 0, k


@pytest.mark.parametrize('dqn_type,algo,A', CONFIGS, ids=IDS)
def test_backward_bars(dqn_type, algo, A):
    """B = 1.  Per term-split pass in isolation: e_mut >= 9 e_honest, full inside, mutants outside.
    Per gradient tensor (bar: the smallest among the term-split passes that feed it, else 3 x its
    honest-chain error): the whole chain evaluated with the full product lists, and as honest fp32
    chains, stays inside; every mutant of every term-split pass, propagated through the layers
    below, moves some tensor outside."""
    P, states, outs, chk = backward_setup(dqn_type, algo, A)
    assert set(chk['pass_bars']) == set(T.bwd_pass_names(dqn_type))
    for name in T.bwd_pass_names(dqn_type):
        b = chk['pass_bars'][name]
        print(T.fmt(f'{dqn_type} {name}', b))
        T.assert_design((dqn_type, algo, name), b)
    g_full = T.backward_chain(P, chk['fwd'], chk['dz'], algo, dqn_type, T.mm_full(dqn_type), rnd=T.f32r)
    e_full, e_hon = T.grads_err(g_full, chk['g_ref']), chk['tensor_honest']
    for t, bar in chk['tensor_bar'].items():
        print(f'{dqn_type} {t:<6} bar {bar:.2e}  chain full {e_full[t]:.2e}  chain honest {e_hon[t]:.2e}')
        assert e_full[t] <= bar, (t, e_full[t], bar)
        assert e_hon[t] <= bar, (t, e_hon[t], bar)
    assert {p for p, _ in chk['mutants']} == set(T.REAL_PASSES[dqn_type]['bwd'])
    T.assert_mutants_caught(chk, (dqn_type, algo))
    for (name, m), errs in chk['mutants'].items():
        print(f'{dqn_type} {name} -{m}: ' + ' '.join(f'{t}={e:.1e}' for t, e in sorted(errs.items()) if e > 0))
