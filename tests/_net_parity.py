"""Shared per-op checks of the NIPS trunk + head kernels (kernels.Net through the C-ABI) against the
fp64 CPU oracle (oracle/ref_cpu.py).

Test infrastructure only (imported by tests/test_gpu_kernels.py and tests/test_gpu_action_width.py).
Bars: forward rtol 1e-4 with an absolute floor of 1e-5 x the tensor's max; gradients 1e-4
relative-L2 against the oracle backward on the GPU's own activations and 2e-2 against the fully
independent fp64 forward + backward; losses 1e-5 and 1e-4 of max(1, |loss|).  Beside the values,
both checks watch the memory around what the kernels own: the head rows' padding columns, the row
after the last one, and the alignment gaps between the tensors of the gradient buffer."""
import numpy as np
import torch

from oracle import ref_cpu as R

GUARD = 12345.0        # sentinel in memory the kernels must leave alone


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_params(net, seed=0, scale=1.0):
    from src.initializers import init_params
    p = init_params(net.names_shapes, seed=seed, stddev=0.02 * scale)
    rng = np.random.default_rng(seed + 1)
    for k in p:
        if k.endswith('_b'):
            p[k] = (rng.standard_normal(p[k].shape) * 0.01).astype(np.float32)
    return p


def oracle_fwd_from_gpu(planes, fwd, zw):
    """The oracle's forward record built from the GPU activations, so the oracle backward uses
    exactly the GPU's ReLU masks (a pre-activation within fp32 rounding of 0 may flip a mask
    between an fp64 and an fp32 forward; that is forward, not backward, error)."""
    B = planes.shape[0]
    l1 = fwd['l1'].cpu().numpy().astype(np.float64).reshape(B, 20, 20, 16)
    l2 = fwd['l2'].cpu().numpy().astype(np.float64)
    return dict(z=fwd['z'].cpu().numpy().astype(np.float64)[:, :zw], h3=fwd['l3'].cpu().numpy().astype(np.float64),
                flat=l2, acts=[R.states_nhwc(planes).astype(np.float64) / 255.0, l1, l2.reshape(B, 9, 9, 32)])


def close(a, b):
    """fp32 accumulation vs fp64: rtol 1e-4, plus an absolute floor of 1e-5 x the tensor's max
    (entries that cancel to ~0 after K = 256..2592 products carry absolute, not relative, error)."""
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * max(np.abs(b).max(), 1e-30))


def guarded_z(B, zs):
    """Head rows [B + 1, zs] filled with GUARD: the forward owns rows 0..B-1 (padding columns
    included, which it zeroes); row B shows a write one row or, where zs has no padding column,
    one lane past the end."""
    return torch.full((B + 1, zs), GUARD, dtype=torch.float32, device='cuda')


def check_forward(K, algo, A, B):
    net = K.Net(A, algo)
    p = make_params(net, seed=B, scale=4.0)
    rng = np.random.default_rng(B)
    planes = rng.integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)
    zbuf = guarded_z(B, net.zs)
    out = net.forward(net.flatten(p), cu(planes), z=zbuf)
    ref = R.forward(p, R.states_nhwc(planes), algo, dtype=np.float64)
    zw = A + 1 if algo == 'a3c' else A
    z = out['z'].cpu().numpy()
    assert z.shape == (B, net.zs) and net.zs == (zw + 3) // 4 * 4
    close(z[:, :zw], ref['z'])
    assert not z[:, zw:].any()
    assert np.array_equal(zbuf[B].cpu().numpy(), np.full(net.zs, GUARD, np.float32))
    close(out['l1'].cpu().numpy().reshape(B, 20, 20, 16), ref['acts'][1])
    close(out['l2'].cpu().numpy(), ref['flat'])
    close(out['l3'].cpu().numpy(), ref['h3'])


def gap_mask(net):
    """True at the floats of the flat buffer that belong to no tensor (64-float alignment gaps)."""
    gap = np.ones(net.total, bool)
    for off, n in zip(net.offsets, net.sizes):
        gap[off:off + n] = False
    return gap


def check_loss_backward(K, algo, A, B, literal, beta=0.01):
    net = K.Net(A, algo)
    p = make_params(net, seed=B + 11, scale=4.0)
    rng = np.random.default_rng(B + 7)
    planes = rng.integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)
    actions = rng.integers(0, A, B).astype(np.int32)
    target = rng.standard_normal(B).astype(np.float32)
    flat = net.flatten(p)
    states = cu(planes)
    fwd = net.forward(flat, states)
    gap = gap_mask(net)
    assert gap.any()
    grads0 = cu(np.where(gap, np.float32(GUARD), np.float32(0.0)))
    grads, loss = net.loss_backward(flat, states, fwd, cu(actions), cu(target), beta=beta, literal_adv=literal,
                                    grads=grads0)
    zw = A + 1 if algo == 'a3c' else A
    # the gradient buffer between the tensors is not the backward's to write
    assert np.array_equal(grads.cpu().numpy()[gap], np.full(int(gap.sum()), GUARD, np.float32))

    def oracle(ref_f):
        if algo == 'a3c':
            losses, dz = R.a3c_loss_and_dz(ref_f['z'], actions, target.astype(np.float64), beta, literal)
            ref_loss = [losses['policy'], losses['value'], losses['entropy'], losses['total']]
        else:
            l, dz = R.q_loss_and_dz(ref_f['z'], actions, target.astype(np.float64))
            ref_loss = [l, ref_f['z'][np.arange(B), actions].mean()]
        return R.backward(p, ref_f, dz, algo), ref_loss

    gv = net.unflatten(grads)
    lg = loss.cpu().numpy()
    # (1) backward arithmetic: oracle on the GPU's activations -> 1e-4 relative per tensor
    g_ref, ref_loss = oracle(oracle_fwd_from_gpu(planes, fwd, zw))
    for name, _ in net.names_shapes:
        err = rel_l2(gv[name].cpu().numpy(), g_ref[name].reshape(gv[name].shape))
        assert err < 1e-4, (name, err)
    for i, r in enumerate(ref_loss):
        assert abs(lg[i] - r) <= 1e-5 * max(1.0, abs(r)), (i, lg[i], r)
    # (2) fully independent fp64 oracle: losses 1e-4 (north star 1e-3); grads 2e-2 (ReLU mask flips)
    g_ref, ref_loss = oracle(R.forward(p, R.states_nhwc(planes), algo, dtype=np.float64))
    for name, _ in net.names_shapes:
        err = rel_l2(gv[name].cpu().numpy(), g_ref[name].reshape(gv[name].shape))
        assert err < 2e-2, (name, err)
    for i, r in enumerate(ref_loss):
        assert abs(lg[i] - r) <= 1e-4 * max(1.0, abs(r)), (i, lg[i], r)
