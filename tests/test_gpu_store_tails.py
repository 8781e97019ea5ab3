"""Tails of the converted store sites (write-through stores of the bulk cross-kernel outputs,
a3c_common.h st_wt): a site with a wrong address, a wrong width or a lost tail predicate
(row < M, q < C2_Q, pos < 400, the last float4 of a tensor) shows as a parity miss at shapes that
end inside a tile, or as a write into memory the kernels do not own.

Engine parity at E in {1, 33}, n in {1, 5}: E = 33 puts one row past a 32-row fc block; n E = 33
and 165 are no multiples of the 64-wide GEMM tiles, and do not divide evenly over the conv
backward's workgroups.  The helpers of tests/_engine_parity.py apply their usual bars (forward
1e-4, same-activation gradients 1e-4, parameters 1e-5, zero unexplained action draws).

Guard rows: the per-op path (kernels.Net) on caller-owned buffers that are one row / one 64-float
block / 256 bytes longer than needed; the excess holds a sentinel that must stay bit-intact, and
the used part meets the bars of tests/_net_parity.py and of test_clip_rmsprop_matches_oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import ref_cpu as R  # noqa: E402
from _engine_parity import check_overlap_vs_oracle, check_sync_vs_oracle  # noqa: E402
from _net_parity import GUARD, close, cu, make_params, oracle_fwd_from_gpu, rel_l2  # noqa: E402

A = 6


@pytest.mark.parametrize('E', [1, 33])
@pytest.mark.parametrize('n', [1, 5])
def test_sync_tails_match_oracle(E, n):
    check_sync_vs_oracle('a3c', A, E, n, 0, iters=3)


@pytest.mark.parametrize('E', [1, 33])
@pytest.mark.parametrize('n', [1, 5])
def test_overlap_tails_match_oracle(E, n):
    check_overlap_vs_oracle(A, E, n, 0, rollouts=4)


BLOCK = 64             # floats of excess behind a flat parameter-sized buffer
WS_EXCESS = 256        # bytes of excess behind a workspace
WS_FILL = 0x5A         # (0x5A5A5A5A as fp32 is a finite number)


def _longer(flat):
    """flat [total] copied into a buffer BLOCK floats longer, the excess = GUARD; (buffer, view)."""
    buf = torch.full((flat.numel() + BLOCK,), GUARD, dtype=torch.float32, device='cuda')
    buf[:flat.numel()] = flat
    return buf, buf[:flat.numel()]


def _excess_intact(buf, total):
    return np.array_equal(buf[total:].cpu().numpy(), np.full(BLOCK, GUARD, np.float32))


def test_guard_rows_stay_intact_at_B33():
    from src import _lib
    _lib.require_device()
    from src import kernels as K
    B = 33
    net = K.Net(A, 'a3c')
    zw = A + 1
    p = make_params(net, seed=B + 3, scale=4.0)
    rng = np.random.default_rng(B + 5)
    planes = rng.integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)
    actions = rng.integers(0, A, B).astype(np.int32)
    target = rng.standard_normal(B).astype(np.float32)
    states = cu(planes)

    w_buf, w = _longer(net.flatten(p))
    ws_bytes = int(net.workspace(B).numel())
    ws_buf = torch.full((ws_bytes + WS_EXCESS,), WS_FILL, dtype=torch.uint8, device='cuda')
    ws = ws_buf[:ws_bytes]
    z_buf = torch.full((B + 1, net.zs), GUARD, dtype=torch.float32, device='cuda')

    def ws_intact():
        return bool((ws_buf[ws_bytes:] == WS_FILL).all().item())

    # forward
    fwd = net.forward(w, states, workspace=ws, z=z_buf)
    torch.cuda.synchronize()
    assert np.array_equal(z_buf[B].cpu().numpy(), np.full(net.zs, GUARD, np.float32))
    assert ws_intact() and _excess_intact(w_buf, net.total)
    ref = R.forward(p, R.states_nhwc(planes), 'a3c', dtype=np.float64)
    z = fwd['z'].cpu().numpy()
    close(z[:, :zw], ref['z'])
    assert not z[:, zw:].any()
    close(fwd['l1'].cpu().numpy().reshape(B, 20, 20, 16), ref['acts'][1])
    close(fwd['l2'].cpu().numpy(), ref['flat'])
    close(fwd['l3'].cpu().numpy(), ref['h3'])

    # loss + backward
    g_buf, g = _longer(torch.zeros(net.total, dtype=torch.float32, device='cuda'))
    grads, loss = net.loss_backward(w, states, fwd, cu(actions), cu(target), grads=g, workspace=ws)
    torch.cuda.synchronize()
    assert _excess_intact(g_buf, net.total) and _excess_intact(w_buf, net.total) and ws_intact()
    assert np.array_equal(z_buf[B].cpu().numpy(), np.full(net.zs, GUARD, np.float32))
    losses, dz = R.a3c_loss_and_dz(oracle_fwd_from_gpu(planes, fwd, zw)['z'], actions, target.astype(np.float64),
                                   0.01, False)
    g_ref = R.backward(p, oracle_fwd_from_gpu(planes, fwd, zw), dz, 'a3c')
    gv = net.unflatten(grads)
    for name, _ in net.names_shapes:
        err = rel_l2(gv[name].cpu().numpy(), g_ref[name].reshape(gv[name].shape))
        assert err < 1e-4, (name, err)
    lg = loss.cpu().numpy()
    for i, k in enumerate(('policy', 'value', 'entropy', 'total')):
        assert abs(lg[i] - losses[k]) <= 1e-5 * max(1.0, abs(losses[k])), (k, lg[i], losses[k])

    # clip + RMSProp on the backward's gradient, three steps
    g_host = {k: v.cpu().numpy().copy() for k, v in gv.items()}
    ms_buf, ms = _longer(torch.ones(net.total, dtype=torch.float32, device='cuda'))
    mom_buf, mom = _longer(torch.zeros(net.total, dtype=torch.float32, device='cuda'))
    for _ in range(3):
        net.clip_rmsprop_apply(w, ms, mom, g, lr=7e-4, clip=40.0)
    torch.cuda.synchronize()
    for buf in (w_buf, ms_buf, mom_buf, g_buf):
        assert _excess_intact(buf, net.total)
    pw = {k: v.copy() for k, v in p.items()}
    pms = {k: np.ones_like(v) for k, v in p.items()}
    pmo = {k: np.zeros_like(v) for k, v in p.items()}
    for _ in range(3):
        for k in pw:
            R.rmsprop_apply(pw[k], pms[k], pmo[k], R.clip_by_norm(g_host[k].reshape(pw[k].shape), 40.0), 7e-4)
    W, MS, MO = net.unflatten(w), net.unflatten(ms), net.unflatten(mom)
    for k in pw:
        np.testing.assert_allclose(W[k].cpu().numpy(), pw[k], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(MS[k].cpu().numpy(), pms[k], rtol=1e-6)
        np.testing.assert_allclose(MO[k].cpu().numpy(), pmo[k], rtol=1e-5, atol=1e-12)
