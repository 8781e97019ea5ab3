"""Parity of each HIP kernel (through the C-ABI) against the CPU oracle and the reference goldens.

Bars: bit-exact for u8 / integer / index work (preprocess, history, returns, TD target, action
draws away from fp boundaries); floating point against the fp64 oracle with the tolerance
written in each test (north star: loss within 1e-3 relative; we hold 1e-4 / 1e-5).
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from make_goldens import frame_from_spec  # noqa: E402
from oracle import philox as px  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from _net_parity import check_forward, check_loss_backward, cu, make_params  # noqa: E402


@pytest.fixture(scope='module')
def K():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


@pytest.fixture(scope='module')
def screen_golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'screen_golden.npz'))


# ---------------------------------------------------------------------------------- K1
def test_preprocess_matches_reference_goldens(K, screen_golden):
    g = screen_golden
    frames = np.stack([frame_from_spec(str(k), int(s)) for k, s in zip(g['kinds'], g['seeds'])])
    out = K.preprocess(cu(frames)).cpu().numpy()
    assert np.array_equal(out, g['screens'])


def test_preprocess_other_geometries(K, screen_golden):
    g = screen_golden
    for i in range(len(g['extra_h'])):
        h, w, oh, ow, sd = (int(g['extra_' + k][i]) for k in ('h', 'w', 'oh', 'ow', 'seed'))
        out = K.preprocess(cu(frame_from_spec('noise', sd, h, w)[None]), out_hw=(oh, ow)).cpu().numpy()[0]
        assert np.array_equal(out, g[f'extra_out{i}']), (h, w, oh, ow)


def test_preprocess_full_luminance_table(K, screen_golden):
    """All 2^24 RGB triples as 16384 frames of 32x32 with an identity resize: the truncated
    fp64 luminance must reproduce the reference's table (sha256)."""
    rgb = np.arange(1 << 24, dtype=np.uint32)
    fr = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], -1).astype(np.uint8)
    out = K.preprocess(cu(fr.reshape(16384, 32, 32, 3)), out_hw=(32, 32)).cpu().numpy().reshape(-1)
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(screen_golden['lum_sha256'])


def test_luminance_exact_integer_form_all_rgb(K, screen_golden):
    """The Atari screen kernel's integer luminance over all 2^24 RGB triples == the reference table."""
    rgb = np.arange(1 << 24, dtype=np.uint32)
    fr = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], -1).astype(np.uint8)
    out = K.luminance(cu(fr)).cpu().numpy()
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(screen_golden['lum_sha256'])


def test_preprocess_gather_stride_and_unaligned(K):
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, (7, 210, 160, 3), dtype=np.uint8)
    idx = np.array([3, 0, 6, 3], np.int32)
    ring = torch.zeros((4, 3, 84, 84), dtype=torch.uint8, device='cuda')
    # write into slot 1 of each ring entry via out_stride = 3*84*84
    from src import _lib
    pool_d, idx_d = cu(pool), cu(idx)        # keep the device tensors alive across the launch
    _lib.check(_lib.lib().a3c_preprocess_u8(_lib.ptr(pool_d), _lib.ptr(idx_d), 4, 210, 160,
                                            _lib.c_void_p(ring.data_ptr() + 84 * 84), 3 * 84 * 84, 84, 84,
                                            _lib.stream_handle()), 'pre')
    got = ring.cpu().numpy()
    for i, f in enumerate(idx):
        assert np.array_equal(got[i, 1], R.screen(pool[f]))
        assert not got[i, 0].any() and not got[i, 2].any()
    # unaligned source (scalar path) and a size whose pixel count is not a multiple of 16
    buf = torch.zeros(1 + 13 * 7 * 3, dtype=torch.uint8, device='cuda')
    fr = rng.integers(0, 256, (13, 7, 3), dtype=np.uint8)
    buf[1:] = cu(fr.reshape(-1))
    out = K.preprocess(buf[1:].view(1, 13, 7, 3), out_hw=(5, 9)).cpu().numpy()[0]
    assert np.array_equal(out, R.resize_bilinear_u8(R.luminance_u8(fr), 5, 9))


def _at_offset(arr, off):
    """arr's bytes on the device `off` bytes behind a fresh allocation's start (itself 256-aligned)."""
    flat = np.ascontiguousarray(arr).reshape(-1)
    buf = torch.zeros(off + flat.size, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    buf[off:] = cu(flat)
    return buf[off:].view(arr.shape)


@pytest.mark.parametrize('off', [0, 1, 8])
def test_preprocess_painted_frames(K, off):
    """The 48 painted frames (tests/_painted.py: the reference's goldens, then saturated, flat and
    hard-edged frames) through the standalone entry point.  A 16-byte-aligned source takes k_screen_atari
    (atari::screen_band); a source 1 or 8 bytes off takes k_preprocess (a3c_preprocess_part) at the Atari
    geometry, with its scalar staging loop."""
    import _painted as P
    src = _at_offset(P.painted_frames(), off)
    assert src.data_ptr() % 16 == off
    out = K.preprocess(src).cpu().numpy()
    bad = [f for f in range(P.N_FRAMES) if not np.array_equal(out[f], P.painted_screens()[f])]
    assert not bad, (off, bad)


@pytest.mark.parametrize('off', [0, 1])
def test_luminance_flat_greys(K, off):
    """R = G = B frames: every group of four pixels takes lum4's multiple-of-10^4 branch (aligned), every
    pixel the scalar lum_exact (1 byte off).  Greys 1, 236 and 254 of the painted set."""
    import _painted as P
    fr = P.painted_frames()[[P.GREYS[v] for v in (1, 236, 254)]]
    out = K.luminance(_at_offset(fr, off)).cpu().numpy()
    assert np.array_equal(out, np.stack([R.luminance_u8(f) for f in fr]))
    assert [int(o[0, 0]) for o in out] == [1, 235, 254] and all((o == o[0, 0]).all() for o in out)


@pytest.mark.parametrize('gather', [False, True], ids=['frames', 'frame_idx'])
def test_preprocess_more_frames_than_one_grid(K, gather):
    """n = 65537 frames of 4x4 -> 2x2: a3c_launch_preprocess splits n > 65535 (the grid's y limit) into
    chunks, advancing the source (or frame_idx) and the output per chunk.  Frame i is pool frame i % 7;
    every output against the oracle's seven screens -- frames 0, 65534, 65535 (the second chunk's
    first) and 65536 among them -- and the guard row behind the output intact."""
    n = 65537
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 256, (7, 4, 4, 3), dtype=np.uint8)
    want = np.stack([R.resize_bilinear_u8(R.luminance_u8(f), 2, 2) for f in pool])
    assert len({w.tobytes() for w in want}) == 7
    idx = (np.arange(n) % 7).astype(np.int32)
    buf = torch.full((n + 1, 2, 2), 0xA5, dtype=torch.uint8, device='cuda')
    if gather:
        out = K.preprocess(cu(pool), frame_idx=cu(idx), out_hw=(2, 2), out=buf[:n])
    else:
        out = K.preprocess(cu(pool[idx]), out_hw=(2, 2), out=buf[:n])
    got = buf.cpu().numpy()
    assert out.data_ptr() == buf.data_ptr()
    for i in (0, 65534, 65535, 65536):
        assert np.array_equal(got[i], want[i % 7]), (i, got[i], want[i % 7])
    assert np.array_equal(got[:n], want[idx])
    assert (got[n] == 0xA5).all()


# ---------------------------------------------------------------------------------- K2
def test_history_push_get(K, screen_golden, golden_dir):
    hg = np.load(os.path.join(golden_dir, 'history_golden.npz'))
    seq = screen_golden['screens'][:7]
    for fmt, nhwc in (('NHWC', True), ('NCHW', False)):
        hist = torch.zeros((1, 4, 84, 84), dtype=torch.uint8, device='cuda')
        gets = []
        for i, s in enumerate(seq):
            K.history_push(hist, cu(s[None]))
            gets.append(K.history_get(hist, nhwc).cpu().numpy()[0])
            if i == 4:
                K.history_push(hist, cu(s[None]), reset_mask=cu(np.ones(1, np.uint8)))
                # reset then add == zeros with s in the newest plane; the reference golden
                # records the pure reset, so check the reset part against History.reset
                h = R.History(cnn_format=fmt)
                h.reset()
                h.add(s)
                assert np.array_equal(K.history_get(hist, nhwc).cpu().numpy()[0], h.get())
                hist.zero_()
                gets.append(K.history_get(hist, nhwc).cpu().numpy()[0])
        assert np.array_equal(np.stack(gets), hg[f'gets_{fmt}'].astype(np.float32)), fmt


# ---------------------------------------------------------------------------------- net
@pytest.mark.parametrize('algo,A,B', [('a3c', 6, 1), ('a3c', 6, 37), ('a3c', 4, 256), ('q', 6, 19), ('q', 4, 64)])
def test_forward_matches_oracle(K, algo, A, B):
    check_forward(K, algo, A, B)


def test_select_action_categorical_and_eps_greedy(K):
    rng = np.random.default_rng(3)
    B, A = 4096, 6
    z = np.zeros((B, 8), np.float32)
    z[:, :A] = rng.standard_normal((B, A)).astype(np.float32) * 2
    seed, tau = 123, 77
    ids = np.arange(B, dtype=np.uint32)
    x = px.philox4x32(tau, 0, ids, px.P_ACTION, *px.seed_key(seed))
    a_gpu = K.select_action(0, cu(z), A, seed, tau).cpu().numpy()
    pi, _, _ = R.softmax_stats(z[:, :A].astype(np.float64))
    u = px.u01(x[0])
    a_ref = R.sample_categorical(pi.astype(np.float32), u)
    cdf = np.cumsum(pi, axis=1)
    near = np.min(np.abs(cdf - u[:, None].astype(np.float64)), axis=1) < 1e-5
    assert np.array_equal(a_gpu[~near], a_ref[~near])
    assert np.bincount(a_gpu, minlength=A).min() > 100          # all actions drawn
    eps = rng.random(B).astype(np.float32)
    a_gpu = K.select_action(1, cu(z), A, seed, tau, eps=cu(eps)).cpu().numpy()
    greedy = np.argmax(z[:, :A], axis=1)
    rnd = x[1] % A
    a_ref = np.where(px.u01(x[0]) < eps, rnd, greedy)
    assert np.array_equal(a_gpu, a_ref)


def test_returns_and_td_target_bit_exact(K):
    rng = np.random.default_rng(4)
    n, E, A = 5, 300, 6
    rew = rng.choice(np.array([-1, 0, 0, 0, 1], np.float32), (n, E))
    term = (rng.random((n, E)) < 0.2).astype(np.uint8)
    boot = rng.standard_normal(E).astype(np.float32)
    got = K.returns(cu(rew), cu(term), cu(boot)).cpu().numpy()
    ref = R.nstep_returns(rew, term, boot, 0.99).astype(np.float32)
    assert np.array_equal(got, ref)
    qn = rng.standard_normal((n * E, 8)).astype(np.float32)
    got = K.td_target(cu(rew.reshape(-1)), cu(term.reshape(-1)), cu(qn), A).cpu().numpy()
    ref = R.td_target(rew.reshape(-1), term.reshape(-1), qn[:, :A], 0.99).astype(np.float32)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize('algo,A,B,literal', [('a3c', 6, 40, False), ('a3c', 6, 300, False),
                                              ('a3c', 4, 13, True), ('q', 6, 64, False), ('q', 4, 7, False)])
def test_loss_backward_matches_oracle(K, algo, A, B, literal):
    check_loss_backward(K, algo, A, B, literal)


def test_clip_rmsprop_matches_oracle(K):
    net = K.Net(6, 'a3c')
    rng = np.random.default_rng(9)
    p = make_params(net, seed=9)
    g = {k: (rng.standard_normal(v.shape) * (0.5 if k == 'l4_w' else 20.0)).astype(np.float32) for k, v in p.items()}
    flat_w, flat_g = net.flatten(p), net.flatten(g)
    ms = torch.ones_like(flat_w)
    mom = torch.zeros_like(flat_w)
    sumsq = torch.zeros(len(net.sizes), dtype=torch.float32, device='cuda')
    for it in range(3):
        net.clip_rmsprop_apply(flat_w, ms, mom, flat_g, lr=7e-4, clip=40.0, sumsq=sumsq)
    pw = {k: v.copy() for k, v in p.items()}
    pms = {k: np.ones_like(v) for k, v in p.items()}
    pmo = {k: np.zeros_like(v) for k, v in p.items()}
    for it in range(3):
        for k in pw:
            R.rmsprop_apply(pw[k], pms[k], pmo[k], R.clip_by_norm(g[k], 40.0), 7e-4)
    W, MS, MO = net.unflatten(flat_w), net.unflatten(ms), net.unflatten(mom)
    for k in pw:
        np.testing.assert_allclose(W[k].cpu().numpy(), pw[k], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(MS[k].cpu().numpy(), pms[k], rtol=1e-6)
        np.testing.assert_allclose(MO[k].cpu().numpy(), pmo[k], rtol=1e-5, atol=1e-12)
    ss = sumsq.cpu().numpy()
    for i, (k, _) in enumerate(net.names_shapes):
        assert np.isclose(ss[i], np.sum(g[k].astype(np.float64) ** 2), rtol=1e-6)
    # clip-only path leaves small tensors (norm < 40) unchanged up to TF's clip arithmetic
    gg = net.flatten(g)
    net.clip_grads(gg, 40.0)
    G = net.unflatten(gg)
    for k in g:
        np.testing.assert_allclose(G[k].cpu().numpy(), R.clip_by_norm(g[k], 40.0), rtol=1e-6, atol=1e-12)
