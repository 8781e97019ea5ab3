"""The nature trunk's bf16 fc mode on the GPU (fc_precision='bf16', DESIGN §4p, with the measured figures) against the
float64 references of tests/_nat_bf16.py and tests/test_nat_fc_bf16_cpu.py; make_params(seed=2, scale=4), dense states,
A = 6, relative L2 of whole tensors, both precisions bf16 unless stated.  Forward: the fc on the kernel's own l3 within
3 x the rounded-operand layer's sequential fp32 chain, a bar 30 x below the unrounded layer.  Backward, last target 50:
A = fp64 with conv and fc passes rounded, C = conv passes only, d = |A - C|; every tensor an fc pass reaches within
d / 8 of A, l4_b and the heads at 1e-4.  B = 1, 3: one ragged m tile (forward, dX), one ragged K slice (dW), the
forward's 7 K chunks and fold.  B = 65: the smallest batch with a second 64-row m tile (forward: rows 0 and 64; dX) and
at which the dW K loop runs a second slice (of one row: the `more` branch, the zero-filled pair rows)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _nat_bf16 as N  # noqa: E402
import _term_split as T  # noqa: E402
from _net_parity import cu, make_params  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_gpu_nat_bf16 import CFG, ENGINES, engine_of, rollout_planes, slot_forward  # noqa: E402
from test_gpu_term_precision import check_layer as fp32_check_layer, flatten, net_of, outs_of, unflatten  # noqa: E402
from test_nat_fc_bf16_cpu import REACHED, chain  # noqa: E402


@functools.lru_cache(maxsize=None)
def forward(B, precision='bf16', fc_precision='bf16'):
    net = net_of(*CFG)
    P = make_params(net, seed=2, scale=4.0)
    planes = T.dense_states(B, 20 + B)
    flat, states = flatten(net, P), cu(planes)
    fwd = net.forward(flat, states, precision=precision, fc_precision=fc_precision)
    torch.cuda.synchronize()
    return net, P, planes, flat, states, fwd, outs_of(lambda k: fwd[k], *CFG, B)


def fc_error(tag, P, l3, l4):
    ref, bar, gap = N.layer_figures(P, 'fc', np.ascontiguousarray(l3, np.float32))
    err = T.rel_l2(l4.reshape(ref.shape), ref)
    print(f'{tag} fc gpu {err:.3e}  bar {bar:.3e}  unrounded layer at {gap:.3e}')
    assert gap >= 30 * bar, (tag, bar, gap)
    return err, bar


def check_fc(tag, P, l3, l4):
    err, bar = fc_error(tag, P, l3, l4)
    assert err <= bar, (tag, err, bar)


@pytest.mark.parametrize('B', [1, 3, 65])
def test_forward_fc(B):
    _, P, _, _, _, _, outs = forward(B)
    rows = [0, B - 1] if B > 3 else list(range(B))
    check_fc(f'per-op B={B} rows {rows}', P, outs['conv3'][rows], outs['fc'][rows])


def targets(B):
    return (np.arange(B) % 6).astype(np.int32), N.tail_heavy_targets(B)


@pytest.mark.parametrize('B', [1, 3, 65])
def test_backward(B):
    net, P, planes, flat, states, fwd, outs = forward(B)
    actions, target = targets(B)
    grads, _ = net.loss_backward(flat, states, fwd, cu(actions), cu(target), precision='bf16', fc_precision='bf16')
    torch.cuda.synchronize()
    G = unflatten(net, grads)
    _, dz = R.a3c_loss_and_dz(outs['head'].astype(np.float64), actions, target.astype(np.float64))
    s = R.states_nhwc(planes)
    A, C = chain(P, s, outs, dz, ('conv', 'fc')), chain(P, s, outs, dz, ('conv',))
    full = R.backward(P, T.fwd_record(P, s, outs, *N.NET), dz, *N.NET)
    bad = []
    for t in full:
        d = T.rel_l2(A[t], C[t]) if t in REACHED else 0.0
        err, bar = T.rel_l2(G[t], A[t] if t in REACHED else full[t]), d / 8 if t in REACHED else 1e-4
        print(f'B={B} {t:<5} d {d:.3e}  gpu-A {err:.3e}  bar {bar:.3e}')
        if not err <= bar:
            bad.append((t, err, bar))
    assert not bad, bad


def test_fp32_convs_with_the_bf16_fc():
    _, P, planes, _, _, _, outs = forward(3, 'fp32', 'bf16')
    for layer in N.LAYERS:
        fp32_check_layer('fp32 convs, bf16 fc', P, R.states_nhwc(planes), outs, CFG, layer, sparse=False)
    check_fc('fp32 convs, bf16 fc', P, outs['conv3'], outs['fc'])


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_fc_fp32_is_the_prec_entry_bit_for_bit(precision):
    net, _, _, flat, states, new, _ = forward(3, precision, 'fp32')
    old = net.forward(flat, states, precision=precision)
    assert all(torch.equal(old[k], new[k]) for k in old)
    actions, target = (cu(x) for x in targets(3))
    g_old, l_old = net.loss_backward(flat, states, old, actions, target, precision=precision)
    g_new, l_new = net.loss_backward(flat, states, new, actions, target, precision=precision, fc_precision='fp32')
    assert torch.equal(g_old, g_new) and torch.equal(l_old, l_new) and bool(g_old.abs().sum() > 0)


def rollout(eng, E, n, overlap=False):
    tau0 = int(eng.counters[0].item())
    (eng.iterate if overlap else eng.rollout_grad)()
    torch.cuda.synchronize()
    sl = eng.slot(0)
    return sl, rollout_planes(eng, tau0, E, n)[0]


def step_errors(tag, P, outs, E, n):
    return [fc_error(f'{tag} step {t}', P, outs['conv3'][t * E:(t + 1) * E], outs['fc'][t * E:(t + 1) * E])
            for t in range(n)]


@pytest.mark.parametrize('overlap,E,n', ENGINES)
def test_engine_activations_and_gradient(overlap, E, n):
    from src._lib import ERR_INVALID, ERR_STATE, PREC_BF16, PREC_FP32, lib
    eng, net, P = engine_of(overlap, E, n, learning_rate=0.0, clip_norm=1e9)
    eng.set_fc_precision('bf16')
    sl, planes = rollout(eng, E, n, overlap)
    if overlap:                       # the backward of rollout 0 runs in the second iteration
        eng.iterate()
        torch.cuda.synchronize()
    else:
        assert lib().a3c_engine_set_fc_precision(eng._h, PREC_FP32) == ERR_STATE       # a gradient is pending
    fwd, outs = slot_forward(sl, E, n)
    assert all(err <= bar for err, bar in step_errors(f'engine {E}x{n}', P, outs, E, n))
    ref, _ = net.loss_backward(eng.params.clone(), planes, fwd, sl['actions'].reshape(-1), sl['returns'].reshape(-1),
                               precision='bf16', fc_precision='bf16')
    G = unflatten(net, eng.grads)
    errs = {t: T.rel_l2(G[t], g) for t, g in unflatten(net, ref).items()}
    print(f'engine {E}x{n} gradient to the per-op entry: largest {max(errs.values()):.3e}')
    assert max(errs.values()) <= 1e-4, errs
    assert lib().a3c_engine_set_fc_precision(eng._h, 7) == ERR_INVALID
    assert lib().a3c_engine_set_fc_precision(None, PREC_BF16) == ERR_INVALID
    eng.close()
    from src.engine import Engine
    nips = Engine(num_envs=4, n_step=2, action_size=6, num_frames=48, seed=1)
    assert lib().a3c_engine_set_fc_precision(nips._h, PREC_BF16) == ERR_INVALID
    nips.close()


def test_engine_switch_between_iterations():
    """bf16, then fp32 for one rollout -- its fc rows miss the bf16 bar and are the fp32 entry's (1e-5: the same fp32
    GEMM at another split, rounding noise of sqrt(3136) 2^-24 = 3e-6 at most, 200 x below what separates the modes)
    -- then bf16 again."""
    E, n = ENGINES[0].values[1:]
    eng, net, P = engine_of(False, E, n, learning_rate=0.0, clip_norm=1e9)
    eng.set_fc_precision('bf16')
    eng.iterate()
    eng.set_fc_precision('fp32')
    sl, planes = rollout(eng, E, n)
    outs = slot_forward(sl, E, n)[1]
    assert all(err > bar for err, bar in step_errors('fp32 after bf16', P, outs, E, n))
    ref = net.forward(eng.params.clone(), planes, precision='bf16', fc_precision='fp32')['l4'].cpu().numpy()
    assert T.rel_l2(outs['fc'], ref) <= 1e-5
    eng.apply()
    eng.set_fc_precision('bf16')
    sl, _ = rollout(eng, E, n)
    assert all(err <= bar for err, bar in step_errors('bf16 again', P, slot_forward(sl, E, n)[1], E, n))
    eng.close()
