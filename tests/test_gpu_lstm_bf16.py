"""The LSTM head's bf16 compute mode on the GPU: the per-op entries against the rounded fp64
reference of tests/_lstm_bf16.py, and the engine in that mode against the per-op entries on its own saved
sequence.  tests/test_lstm_bf16_cpu.py shows that the unrounded reference lies outside every bar used here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _lstm_bf16 as LB  # noqa: E402
from oracle import ref_cpu as Rc  # noqa: E402


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('form', ['x', 'fc_part'])
@pytest.mark.parametrize('B', LB.STEP_B)
def test_step_matches_rounded_cell(B, form):
    from src import kernels as K
    k = LB.step_case(B)
    src = dict(x=dev(k['x'])) if form == 'x' else dict(x=None, fc_part=dev(k['fc_part']), fc_bias=dev(k['fc_bias']))
    out = K.lstm_step(dev(k['w']), dev(k['b']), src.pop('x'), dev(k['h']), dev(k['c']), dev(k['terms']),
                      precision='bf16', **src)
    torch.cuda.synchronize()
    out = {name: v.cpu().numpy() for name, v in out.items()}
    x = k['x']
    if form == 'fc_part':
        x = k['x_fold']
        assert np.array_equal(out['l3'], x)              # slice order, bias, ReLU; written unrounded
    keep = (1 - k['terms'].astype(np.float32))[:, None]
    hr, cr, gr = LB.cell(x, k['h'] * keep, k['c'] * keep, k['w'], k['b'])
    for name, want in (('h', hr), ('c', cr), ('gates', gr)):
        print(f'B={B} {form} {name}: max abs err {np.abs(out[name] - want).max():.2e}')
        np.testing.assert_allclose(out[name], want, err_msg=name, **LB.STEP_BAR)
    assert np.array_equal(out['hp'], k['h'] * keep) and np.array_equal(out['cp'], k['c'] * keep)


@pytest.mark.parametrize('n,E', LB.BPTT_SHAPES)
def test_bptt_matches_rounded_backward(n, E):
    """Measured rel-L2 errors against the rounded reference, and d (rounded against unrounded), on one MI355X:
    see DESIGN §4q."""
    from src import kernels as K
    case = LB.bptt_case(n, E)
    got = K.lstm_bptt(*[dev(a) for a in case], precision='bf16')
    torch.cuda.synchronize()
    ref, off = LB.backward_seq(*case), LB.backward_seq(*case, r=LB.plain)
    for name, g, r, o in zip(('dx', 'dw', 'db'), got, ref, off):
        err, d = LB.rel_l2(g.cpu().numpy(), r), LB.rel_l2(o, r)
        print(f'n={n} E={E} {name}: err {err:.3e}  d {d:.3e}  bar {max(d / 8, 1e-5):.3e}')
        assert err <= max(d / 8, 1e-5), (name, err, d)


def make_engine(E, overlap, lstm_precision, A=6, n=3, seed=11):
    from src.engine import Engine
    from src.initializers import init_params, flatten_host
    from src.kernels import param_names_shapes
    eng = Engine(num_envs=E, n_step=n, action_size=A, algo='a3c', start_lives=3, num_frames=48, seed=seed, lstm=True,
                 overlap=overlap, lstm_precision=lstm_precision, learning_rate=2e-3)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=seed, stddev=0.08)))
    return eng, ns


@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)])
def test_engine_bf16_equals_per_op_on_its_saved_sequence(E, overlap):
    from src import kernels as K
    A, n = 6, 3
    eng, ns = make_engine(E, overlap, 'bf16')
    assert eng.lstm_precision == 'bf16'
    snaps = []
    for k in range(3):
        snaps.append(eng.params.clone())
        eng.iterate()
        torch.cuda.synchronize()
        j = k - 1 if overlap else k                      # the rollout this call back-propagated
        if j < 0:
            continue
        sl = eng.slot(j & 1 if overlap else 0)
        P = {name: snaps[j][off:off + sz].reshape(shp) for (name, shp), off, sz in zip(ns, eng.offsets, eng.sizes)}
        G = {name: eng.grads[off:off + sz].reshape(shp) for (name, shp), off, sz in zip(ns, eng.offsets, eng.sizes)}
        x = sl['act_l3'].reshape(n, E, 256)
        for t in range(n):
            out = K.lstm_step(P['lstm_w'], P['lstm_b'], x[t].contiguous(), sl['lstm_hp'][t], sl['lstm_cp'][t],
                              precision='bf16')
            for name in ('h', 'c', 'gates'):
                np.testing.assert_allclose(sl['lstm_' + name][t].cpu().numpy(), out[name].cpu().numpy(),
                                           err_msg=f'{k} {t} {name}', **LB.STEP_BAR)
        z = sl['z'].cpu().numpy()[:n].reshape(n * E, -1)[:, :A + 1].astype(np.float64)
        _, dz = Rc.a3c_loss_and_dz(z, sl['actions'].cpu().numpy().reshape(-1),
                                   sl['returns'].cpu().numpy().reshape(-1).astype(np.float64), 0.01, False)
        dh = dz[:, :A] @ LB.plain(P['p_w'].cpu().numpy()).T + dz[:, A:] @ LB.plain(P['q_w'].cpu().numpy()).T
        _, dw, db = K.lstm_bptt(P['lstm_w'], x.contiguous(), sl['lstm_hp'], sl['lstm_cp'], sl['lstm_gates'], sl['lstm_c'],
                                sl['terminals'], dev(dh.reshape(n, E, -1).astype(np.float32)), precision='bf16')
        errs = LB.rel_l2(G['lstm_w'].cpu().numpy(), dw.cpu().numpy()), LB.rel_l2(G['lstm_b'].cpu().numpy(), db.cpu().numpy())
        print(f'E={E} overlap={overlap} rollout {j}: lstm_w {errs[0]:.2e} lstm_b {errs[1]:.2e}')
        assert max(errs) < 1e-5, (k, errs)
    assert torch.isfinite(eng.params).all()
    eng.close()


def test_play_bf16_finite_and_on_the_fp32_schedule():
    runs = {}
    for mode in ('fp32', 'bf16'):
        eng, _ = make_engine(8, False, mode)
        runs[mode] = eng.play(n_episode=16, n_step=6)
        eng.close()
    assert np.isfinite(runs['bf16']['returns']).all() and (runs['bf16']['lengths'] > 0).all()
    for key in ('episode_env', 'episode_tau0', 'steps'):
        assert np.array_equal(runs['bf16'][key], runs['fp32'][key]), key


def test_set_lstm_precision_rejected_on_a_feed_forward_engine():
    from src import _lib
    from src.engine import Engine
    eng = Engine(num_envs=4, n_step=2, action_size=6, num_frames=32, seed=5)
    with pytest.raises(_lib.A3CError, match='feed-forward head') as ei:
        _lib.check(_lib.lib().a3c_engine_set_lstm_precision(eng._h, _lib.PREC_BF16), 'a3c_engine_set_lstm_precision')
    assert ei.value.rc == _lib.ERR_INVALID
    eng.close()
