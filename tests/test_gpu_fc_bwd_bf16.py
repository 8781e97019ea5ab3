"""The nips fc backward's bf16 mode (k_fc_dw_bf, k_fc_dx_bf) on the GPU: the two passes alone and the
per-op backward against the rounded fp64 references of tests/_fc_bwd_bf16.py, and the engine in that mode against the
per-op entry on its own saved rollout.  tests/test_fc_bwd_bf16_cpu.py shows the bars see a lost K index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _conv_bwd_bf16 as C  # noqa: E402
import _fc_bwd_bf16 as F  # noqa: E402
import _term_split as T  # noqa: E402
from _net_parity import cu  # noqa: E402
from test_gpu_term_precision import flatten, net_of, outs_of, unflatten  # noqa: E402


@pytest.mark.parametrize('form', ['f32', 'bits'])
@pytest.mark.parametrize('B', [1, 5, 65, 259])     # 259: 9 slices of 32 over 4 waves -- 3, 2, 2, 2, the last ragged
def test_passes_alone(B, form):
    from src import kernels
    net_of('nips', 'a3c', C.A)
    l2, dl3, W = F.passes_inputs(B)
    ref = F.passes_ref(l2, dl3, W)
    plain = F.passes_ref(l2, dl3, W, rnd=lambda x: x)
    assert min(T.rel_l2(plain[0], ref[0]), T.rel_l2(plain[2], ref[2])) >= 1e-4     # (the fp32 GEMM is no pass)
    g = [cu(x) for x in (l2, dl3, W)]
    masks = dict(f32=dict(mask=g[0]), bits=dict(maskbits=cu(F.bits_of(l2))))
    out = [t.cpu().numpy() for t in kernels.fc_bwd_bf16(*g, **masks[form])]
    errs = [T.rel_l2(o, r) for o, r in zip(out, ref)]
    print(f'B={B} {form}: dW {errs[0]:.3e}  colsum {errs[1]:.3e}  dl2 {errs[2]:.3e}  bar 1.000e-05')
    assert max(errs) <= 1e-5, errs
    assert not out[2][l2 <= 0].any()
    if form == 'bits':
        assert np.array_equal(out[2], kernels.fc_bwd_bf16(*g, **masks['f32'])[2].cpu().numpy())


@pytest.mark.parametrize('algo,B,conv', [c + (False,) for c in C.CASES] + [('a3c', 5, True), ('a3c', 259, True)])
def test_per_op_matches_rounded_backward(algo, B, conv):
    """conv: both backward switches in bf16.  Measured err, d and bar per case and tensor on one MI355X: DESIGN §4s."""
    net = net_of('nips', algo, C.A)
    _, P, planes, actions, target = C.case(algo, B)
    flat, states = flatten(net, P), cu(planes)
    fwd = net.forward(flat, states)
    ga, la = net.loss_backward(flat, states, fwd, cu(actions), cu(target))
    gb, lb = net.loss_backward(flat, states, fwd, cu(actions), cu(target), fc_bwd_precision='bf16',
                               conv_bwd_precision='bf16' if conv else None)
    torch.cuda.synchronize()
    outs = outs_of(lambda k: fwd[k], 'nips', algo, C.A, B)
    rounded, plain = F.refs(P, planes, outs, C.dz_of(algo, outs['head'], actions, target), algo, conv=conv)
    G32, G = unflatten(net, ga), unflatten(net, gb)
    fcw, fcb = T.fc_name(algo) + '_w', T.fc_name(algo) + '_b'
    bad = []
    for t in (fcw,) + F.CONV:
        err, (d, bar) = T.rel_l2(G[t], rounded[t]), F.bar(plain, rounded, t)
        print(f'{algo} B={B} conv={conv} {t}: err {err:.3e}  d {d:.3e}  bar {bar:.3e}')
        if not err <= bar:
            bad.append((t, err, d, bar))
    err = T.rel_l2(G[fcb], plain[fcb])
    print(f'{algo} B={B} conv={conv} {fcb}: err {err:.3e}  bar 1.000e-05')
    assert not bad and err <= 1e-5, (bad, err)
    assert torch.equal(la, lb) and all(np.array_equal(G[t], G32[t]) for t in G if t not in (fcw, fcb) + F.CONV)


def make_engine(E, overlap, mode, lstm=False, n=3, seed=11):
    from src.engine import Engine
    from src.initializers import init_params, flatten_host
    from src.kernels import param_names_shapes
    eng = Engine(num_envs=E, n_step=n, action_size=C.A, algo='a3c', start_lives=3, num_frames=48, seed=seed, lstm=lstm,
                 overlap=overlap, fc_bwd_precision=mode, learning_rate=2e-3, clip_norm=1e9)
    ns = param_names_shapes(C.A, 'a3c', lstm=lstm)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=seed, stddev=0.08)))
    return eng, ns


@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)])
def test_engine_bf16_equals_per_op_on_its_saved_rollout(E, overlap):
    n = 3
    net = net_of('nips', 'a3c', C.A)
    eng, ns = make_engine(E, overlap, 'bf16')
    ref, _ = make_engine(E, overlap, 'fp32')
    assert eng.fc_bwd_precision == 'bf16'
    fcw, fcb = T.fc_name('a3c') + '_w', T.fc_name('a3c') + '_b'
    tau0, R, snaps = int(eng.counters[0].item()), eng.ring_slots, []
    for k in range(3):
        snaps.append(eng.params.clone())
        eng.iterate()
        torch.cuda.synchronize()
        if k == 0:                                       # the forward is untouched: the first rollout, bit for bit
            ref.iterate()
            torch.cuda.synchronize()
            assert torch.equal(eng.slot(0)['actions'], ref.slot(0)['actions'])
            assert torch.equal(eng.slot(0)['z'], ref.slot(0)['z'])
        j = k - 1 if overlap else k                      # the rollout this call back-propagated
        if j < 0:
            continue
        sl = eng.slot(j & 1 if overlap else 0)
        ring = eng.frame_ring                            # state (t, e): frames tau - 3 .. tau, tau = tau0 + n j + t
        states = torch.stack([ring[:, [(tau0 + n * j + t - 3 + c) % R for c in range(4)]] for t in range(n)])
        fwd = dict(l1=sl['act_l1'], l2=sl['act_l2'], l3=sl['act_l3'], z=sl['z'][:n].reshape(n * E, -1).contiguous())
        g, _ = net.loss_backward(snaps[j], states.reshape(n * E, 4, 84, 84).contiguous(), fwd,
                                 sl['actions'].reshape(-1).contiguous(), sl['returns'].reshape(-1).contiguous(),
                                 fc_bwd_precision='bf16')
        torch.cuda.synchronize()
        G, Gop = unflatten(net, eng.grads), unflatten(net, g)
        errs = {t: T.rel_l2(G[t], Gop[t]) for t in F.CONV}
        print(f'E={E} overlap={overlap} rollout {j}:', ' '.join(f'{t} {e:.2e}' for t, e in errs.items()))
        assert np.array_equal(G[fcw], Gop[fcw]) and np.array_equal(G[fcb], Gop[fcb]), k
        assert max(errs.values()) < 1e-5, (k, errs)
    assert torch.isfinite(eng.params).all()
    eng.close()
    ref.close()


def test_lstm_engine_moves_fc_w_only_a_little():
    P = {}
    for mode in ('fp32', 'bf16'):
        eng, ns = make_engine(8, False, mode, lstm=True)
        eng.iterate()
        torch.cuda.synchronize()
        f = eng.params.cpu().numpy()
        P[mode] = {name: f[off:off + sz] for (name, _), off, sz in zip(ns, eng.offsets, eng.sizes)}
        eng.close()
    t = T.fc_name('a3c') + '_w'
    dist = T.rel_l2(P['bf16'][t], P['fp32'][t])
    print(f'lstm {t}: bf16 against fp32 params {dist:.3e}')
    assert 0 < dist < 0.05, dist              # a sanity cap, far above one rounding of 2^-9 per operand


def test_setter_rejected_on_a_nature_engine():
    from src import _lib
    from src.engine import Engine
    eng = Engine(num_envs=4, n_step=2, action_size=6, num_frames=32, seed=5, dqn_type='nature')
    with pytest.raises(_lib.A3CError, match='nips trunk') as ei:
        _lib.check(_lib.lib().a3c_engine_set_fc_bwd_precision(eng._h, _lib.PREC_BF16), 'a3c_engine_set_fc_bwd_precision')
    assert ei.value.rc == _lib.ERR_INVALID
    eng.close()
