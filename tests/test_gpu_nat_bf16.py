"""The nature trunk's bf16 compute mode on the GPU (A3C_PREC_BF16, DESIGN §4n, with the measured figures) against
tests/_nat_bf16.py's float64 reference: dense u8 states, make_params(scale=4), A = 6, relative L2 of whole tensors.
Forward, layer-isolated on the kernel's own input: within 3 x the rounded-operand layer's sequential fp32 chain, a bar
at least 30 x below the unrounded layer (so the FP32 kernels miss it).  Backward, B = 1 and 3 (a sample boundary in a
dW slab, a ragged last dX m-tile): A = fp64 with every conv pass's operands rounded, B = unrounded, d = |A - B|; a
conv tensor within d / 8 of A.  l3_b is fed by the fc's dX alone (d = 0), so it is held with the fc and head tensors
at the suite's 1e-4.  Engine: the same bars on a slot, its gradient against the per-op entry (1e-4, the
same-activation bar of tests/_engine_parity.py), graph = eager and a switch back = never switched, bit for bit."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _nat_bf16 as N  # noqa: E402
import _term_split as T  # noqa: E402
from _net_parity import cu, make_params  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_gpu_term_precision import flatten, net_of, outs_of, unflatten  # noqa: E402

CFG = ('nature', 'a3c', 6)
ENGINES = [pytest.param(False, 8, 2, id='sync'), pytest.param(True, 16, 3, id='overlap')]


@functools.lru_cache(maxsize=None)
def forward(B):
    net = net_of(*CFG)
    P = make_params(net, seed=2, scale=4.0)
    planes = T.dense_states(B, 20 + B)
    flat, states = flatten(net, P), cu(planes)
    fwd = net.forward(flat, states, precision='bf16')
    torch.cuda.synchronize()
    return net, P, planes, flat, states, fwd, outs_of(lambda k: fwd[k], *CFG, B)


def check_layer(tag, P, states_nhwc, outs, layer):
    x_in = dict(conv1=states_nhwc, conv2=outs['conv1'], conv3=outs['conv2'])[layer]
    ref, bar, gap = N.layer_figures(P, layer, x_in)
    err = T.rel_l2(outs[layer].reshape(ref.shape), ref)
    print(f'{tag} {layer} gpu {err:.3e}  bar {bar:.3e}  unrounded layer at {gap:.3e}')
    assert gap >= 30 * bar and err <= bar, (tag, layer, err, bar, gap)


@pytest.mark.parametrize('layer', N.LAYERS)
def test_forward_layer(layer):
    _, P, planes, _, _, _, outs = forward(2)
    check_layer('per-op', P, R.states_nhwc(planes), outs, layer)


def test_forward_fc_head_and_fp32_entry():
    net, P, planes, flat, states, _, outs = forward(2)
    l4 = np.maximum(outs['conv3'].astype(np.float64) @ P['l4_w'] + P['l4_b'], 0)
    W, b = T.head_wb(P, 'a3c')
    assert T.rel_l2(outs['fc'], l4) <= 1e-4 and T.rel_l2(outs['head'], outs['fc'].astype(np.float64) @ W + b) <= 1e-4
    old, new = net.forward(flat, states), net.forward(flat, states, precision='fp32')
    assert all(torch.equal(old[k], new[k]) for k in old)


@pytest.mark.parametrize('B', [1, 3])
def test_backward(B):
    net, P, planes, flat, states, fwd, outs = forward(B)
    actions = (np.arange(B) % 6).astype(np.int32)
    target = np.linspace(0.7, -0.4, B).astype(np.float32)
    grads, _ = net.loss_backward(flat, states, fwd, cu(actions), cu(target), precision='bf16')
    torch.cuda.synchronize()
    G = unflatten(net, grads)
    _, dz = R.a3c_loss_and_dz(outs['head'].astype(np.float64), actions, target.astype(np.float64))
    A, Bref = N.backward_refs(P, R.states_nhwc(planes), outs, dz)
    bad = []
    for t in Bref:
        reached = t in N.CONV_TENSORS and t != 'l3_b'
        d = T.rel_l2(A[t], Bref[t]) if reached else 0.0
        ea, eb = T.rel_l2(G[t], A[t] if reached else Bref[t]), T.rel_l2(G[t], Bref[t])
        bar = d / 8 if reached else 1e-4
        print(f'B={B} {t:<5} d {d:.3e}  gpu-A {ea:.3e}  gpu-B {eb:.3e}  bar {bar:.3e}')
        if not ea <= bar:
            bad.append((t, ea, bar))
    assert not bad, bad


def engine_of(overlap, E, n, precision='bf16', **kw):
    from src.engine import Engine
    from src.initializers import flatten_host
    net = net_of(*CFG)
    eng = Engine(num_envs=E, n_step=n, action_size=6, num_frames=48, seed=77, overlap=overlap, dqn_type='nature', **kw)
    eng.set_precision(precision)
    P = make_params(net, seed=2, scale=4.0)
    eng.reset(flatten_host(net.names_shapes, eng.offsets, eng.params.numel(), P))
    return eng, net, P


@pytest.mark.parametrize('overlap,E,n', ENGINES)
def test_engine_activations_and_gradient(overlap, E, n):
    from src._lib import ERR_INVALID, ERR_STATE, PREC_BF16, PREC_FP32, lib
    eng, net, P = engine_of(overlap, E, n, learning_rate=0.0, clip_norm=1e9)
    tau0 = int(eng.counters[0].item())
    (eng.iterate if overlap else eng.rollout_grad)()
    torch.cuda.synchronize()
    ring, sl = eng.frame_ring, eng.slot(0)
    idx = [(tau0 + t - 3 + c) % eng.ring_slots for t in range(n) for c in range(4)]     # state t: frames t-3 .. t
    planes = ring[:, idx].reshape(E, n, 4, 84, 84).transpose(0, 1).reshape(n * E, 4, 84, 84).contiguous()
    if overlap:                       # the backward of rollout 0 runs in the second iteration
        eng.iterate()
        torch.cuda.synchronize()
    else:
        assert lib().a3c_engine_set_precision(eng._h, PREC_FP32) == ERR_STATE       # a gradient is pending
    fwd = dict(z=sl['z'][:n].reshape(n * E, -1), **{k: sl['act_' + k] for k in ('l1', 'l2', 'l3', 'l4')})
    rows = slice((n - 1) * E, n * E)                                               # the rollout's last step
    outs = {k: v[rows] for k, v in outs_of(lambda k: fwd[k], *CFG, n * E).items()}
    for layer in N.LAYERS:
        check_layer(f'engine {E}x{n}', P, R.states_nhwc(planes[rows].cpu().numpy()), outs, layer)
    G = unflatten(net, eng.grads)
    ref, _ = net.loss_backward(eng.params.clone(), planes, fwd, sl['actions'].reshape(-1), sl['returns'].reshape(-1),
                               precision='bf16')
    for t, g in unflatten(net, ref).items():
        assert T.rel_l2(G[t], g) <= 1e-4, (t, T.rel_l2(G[t], g))
    assert lib().a3c_engine_set_precision(eng._h, 7) == ERR_INVALID
    assert lib().a3c_engine_set_precision(None, PREC_BF16) == ERR_INVALID
    eng.close()
    from src.engine import Engine
    nips = Engine(num_envs=4, n_step=2, action_size=6, num_frames=48, seed=1)
    assert lib().a3c_engine_set_precision(nips._h, PREC_BF16) == ERR_INVALID
    nips.close()


@pytest.mark.parametrize('what', ['graph', 'switch-back'])
@pytest.mark.parametrize('overlap,E,n', ENGINES)
def test_engine_bit_for_bit(overlap, E, n, what):
    """graph: replays of the captured bf16 iteration = eager; switch-back: BF16 then FP32 = an engine never switched."""
    if what == 'graph':
        a, b = engine_of(overlap, E, n, use_graph=True)[0], engine_of(overlap, E, n)[0]
    else:
        a, b = engine_of(overlap, E, n)[0], engine_of(overlap, E, n, precision='fp32')[0]
        a.set_precision('fp32')
    p0 = a.params.clone()
    for k in range(4):
        for eng in (a, b):
            eng.iterate()
        torch.cuda.synchronize()
        assert torch.equal(a.params, b.params) and torch.equal(a.grads, b.grads), (what, k)
    assert not torch.equal(a.params, p0)       # the iterations moved the parameters
    a.close()
    b.close()
