"""The nature trunk's bf16 compute mode on the GPU (A3C_PREC_BF16, DESIGN §4n, with the measured figures) against
tests/_nat_bf16.py's float64 reference: dense u8 states, make_params(scale=4), A = 6, relative L2 of whole tensors.
Forward, layer-isolated on the kernel's own input: within 3 x the rounded-operand layer's sequential fp32 chain, a bar
at least 30 x below the unrounded layer (so the FP32 kernels miss it).  Backward, B = 1 and 3 (a sample boundary in a
dW slab, a ragged last dX m-tile): A = fp64 with every conv pass's operands rounded, B = unrounded, d = |A - B|; a
conv tensor within d / 8 of A.  l3_b is fed by the fc's dX alone (d = 0), so it is held with the fc and head tensors
at the suite's 1e-4.  B = 31, 103, 123 at the same bars: the smallest batches at which the dW passes' K loops run
two, four and five slices (tests/_plan.py nat_dw_slices; up to B = 30 every dW workgroup runs one slice and leaves),
with the last sample's target at 50 so that the bars see a lost row (tests/test_nat_bf16_cpu.py).  Engine: the same
bars on every step of a slot, the bootstrap row within 1 / 30 of the distance between the modes' per-op rows, the
gradient against the per-op entry (1e-4, the same-activation bar of tests/_engine_parity.py), a switch between
iterations, graph = eager and a switch back = never switched, bit for bit."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _nat_bf16 as N  # noqa: E402
import _plan as P_  # noqa: E402
import _term_split as T  # noqa: E402
from _net_parity import cu, make_params  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from test_gpu_term_precision import check_layer as fp32_check_layer  # noqa: E402
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


def layer_error(tag, P, states_nhwc, outs, layer):
    x_in = dict(conv1=states_nhwc, conv2=outs['conv1'], conv3=outs['conv2'])[layer]
    ref, bar, gap = N.layer_figures(P, layer, x_in)
    err = T.rel_l2(outs[layer].reshape(ref.shape), ref)
    print(f'{tag} {layer} gpu {err:.3e}  bar {bar:.3e}  unrounded layer at {gap:.3e}')
    assert gap >= 30 * bar, (tag, layer, bar, gap)
    return err, bar


def check_layer(tag, P, states_nhwc, outs, layer):
    err, bar = layer_error(tag, P, states_nhwc, outs, layer)
    assert err <= bar, (tag, layer, err, bar)
    return err


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


def check_backward(B, target):
    net, P, planes, flat, states, fwd, outs = forward(B)
    actions = (np.arange(B) % 6).astype(np.int32)
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


@pytest.mark.parametrize('B', [1, 3])
def test_backward(B):
    check_backward(B, np.linspace(0.7, -0.4, B).astype(np.float32))


def reaches_31(s, before):
    """conv1 dW (<NG_DW1, 1, 32, 1, 1>, NBUF = 2, PF = 2) with two slices a chunk, the smallest batch that has them:
    the second register set's load before the loop, store(NBUF - 1, ..), compute(NBUF - 1), and a last chunk of
    48 rows whose second slice holds 16 (`r >= kend` inside a slice that is not the chunk's first)."""
    assert [x.slices for x in before] == [1, 1, 1] and [x.slices for x in s] == [2, 1, 1]
    assert [x.last_rows for x in s] == [48, 15, 15] and s[0].last_slice_rows == 16


def reaches_103(s, before):
    """conv2 and conv3 dW (<NG_DW, 2|3, 64, 1, 1>, NBUF = 1, PF = 1) with two slices: the `more` branch, a store
    into the one buffer between two barriers (conv2 first leaves one slice at B = 102, where its last chunk holds
    6 rows; here 23 and 55, the second slice ragged); conv1 with four slices: the load of k0 + 3 BK."""
    assert [x.slices for x in s] == [4, 2, 2] and [x.last_rows for x in s] == [112, 23, 55]
    assert P_.nat_dw_slices(6, 101)[1].slices == 1 and P_.nat_dw_slices(6, 92)[0].slices == 3
    assert [x.last_slice_rows for x in s] == [16, 23, 23]


def reaches_123(s, before):
    """conv1 dW with five slices, the smallest batch that has them: the load of k0 + 4 BK, the second trip of the
    `for`, the exit by `break` on the odd count, a last chunk of two and a half slices; conv3 with three."""
    assert before[0].slices == 4 and [x.slices for x in s] == [5, 2, 3]
    assert [x.last_rows for x in s] == [80, 43, 75] and [x.last_slice_rows for x in s] == [16, 11, 11]


# largest kernel-to-A error over the conv tensors / largest error over l3_b, the fc and the heads, on an MI355X:
SLICES = [
    (31, reaches_31, (64, 32, 32)),         # 2.0e-05 (l1_w) / 2.4e-07
    (103, reaches_103, (128, 64, 64)),      # 6.8e-05 (l1_w) / 1.6e-07
    (123, reaches_123, (160, 64, 96)),      # 3.7e-05 (l1_w) / 1.4e-07
]


@pytest.mark.parametrize('B,reaches,kc', SLICES, ids=[str(c[0]) for c in SLICES])
def test_backward_dw_slices(B, reaches, kc):
    """The dW passes' K loops past their first slice (tests/_plan.py nat_dw_slices; up to B = 30 every dW workgroup
    runs one slice and leaves), at test_backward's bars.  The last sample's target is 50: with the flat ramp a lost
    tail row would stay under d / 8 (tests/test_nat_bf16_cpu.py, which also shows that these bars see a lost tail
    row, a lost ragged slice and a lost interior slice of every pass at least 3-fold)."""
    assert P_.nat_plan(6, B).kc == kc
    reaches(P_.nat_dw_slices(6, B), P_.nat_dw_slices(6, B - 1))
    check_backward(B, N.tail_heavy_targets(B))


def test_forward_first_and_last_state_of_123():
    """One workgroup per state: the first and the last of the largest batch here, at test_forward_layer's bars."""
    B = SLICES[-1][0]
    _, P, planes, _, _, _, outs = forward(B)
    rows = [0, B - 1]
    for layer in N.LAYERS:
        check_layer(f'per-op B={B} states 0, {B - 1}', P, R.states_nhwc(planes[rows]),
                    {k: v[rows] for k, v in outs.items()}, layer)


def engine_of(overlap, E, n, precision='bf16', **kw):
    from src.engine import Engine
    from src.initializers import flatten_host
    net = net_of(*CFG)
    eng = Engine(num_envs=E, n_step=n, action_size=6, num_frames=48, seed=77, overlap=overlap, dqn_type='nature', **kw)
    eng.set_precision(precision)
    P = make_params(net, seed=2, scale=4.0)
    eng.reset(flatten_host(net.names_shapes, eng.offsets, eng.params.numel(), P))
    return eng, net, P


def rollout_planes(eng, tau0, E, n):
    """The rollout that started at frame tau0, from the engine's ring: the planes of s_0 .. s_{n-1} [n E, 4, 84, 84]
    (row t E + e) and of the bootstrap state s_n [E, 4, 84, 84]; state t holds frames tau0 + t - 3 .. tau0 + t."""
    idx = [(tau0 + t - 3 + c) % eng.ring_slots for t in range(n + 1) for c in range(4)]
    p = eng.frame_ring[:, idx].reshape(E, n + 1, 4, 84, 84).transpose(0, 1).contiguous()
    return p[:n].reshape(n * E, 4, 84, 84), p[n].contiguous()


def slot_forward(sl, E, n):
    """(the per-op entry's `fwd` of the slot's n E rows, their {conv1.., fc, head} arrays)."""
    fwd = dict(z=sl['z'][:n].reshape(n * E, -1), **{k: sl['act_' + k] for k in ('l1', 'l2', 'l3', 'l4')})
    return fwd, outs_of(lambda k: fwd[k], *CFG, n * E)


def check_steps(tag, P, planes, outs, E, n, check=check_layer):
    """check(..) on every step's rows of a slot -> {layer: what it returned, per step}."""
    got = {layer: [] for layer in N.LAYERS}
    for t in range(n):
        rows = slice(t * E, (t + 1) * E)
        step = {k: v[rows] for k, v in outs.items()}
        for layer in N.LAYERS:
            got[layer].append(check(f'{tag} step {t}', P, R.states_nhwc(planes[rows].cpu().numpy()), step, layer))
    return got


# largest error seen on an MI355X, sync 8 x 2 / overlap 16 x 3:
#   every step's conv1 / conv2 / conv3 against check_layer's bars   8.5e-08, 1.2e-07, 1.0e-07 in both
#   the bootstrap row to the bf16 per-op row                        0 / 0 (gap 4.1e-03 / 3.8e-03, bar 1.4e-04 / 1.3e-04)
#   the gradient to the per-op bf16 entry                           0 / 0 (the same kernels on the same rows)
@pytest.mark.parametrize('overlap,E,n', ENGINES)
def test_engine_activations_and_gradient(overlap, E, n):
    from src._lib import ERR_INVALID, ERR_STATE, PREC_BF16, PREC_FP32, lib
    eng, net, P = engine_of(overlap, E, n, learning_rate=0.0, clip_norm=1e9)
    tau0 = int(eng.counters[0].item())
    (eng.iterate if overlap else eng.rollout_grad)()
    torch.cuda.synchronize()
    sl = eng.slot(0)
    planes, boot = rollout_planes(eng, tau0, E, n)
    if overlap:                       # the backward of rollout 0 runs in the second iteration
        eng.iterate()
        torch.cuda.synchronize()
    else:
        assert lib().a3c_engine_set_precision(eng._h, PREC_FP32) == ERR_STATE       # a gradient is pending
    fwd, outs = slot_forward(sl, E, n)
    check_steps(f'engine {E}x{n}', P, planes, outs, E, n)
    # the bootstrap state follows the mode too: its row against the per-op forward of s_n's planes in both modes.
    # gap is what an FP32 bootstrap forward would be off by; what is left between the engine and the per-op entry
    # in the same mode is the fc's split-K order in fp32
    z = {m: net.forward(eng.params.clone(), boot, precision=m)['z'][:, :7].cpu().numpy() for m in ('fp32', 'bf16')}
    gap = T.rel_l2(z['fp32'], z['bf16'])
    err = T.rel_l2(sl['z'][n][:, :7].cpu().numpy(), z['bf16'])
    print(f'engine {E}x{n} bootstrap row: fp32 to bf16 per-op {gap:.3e}  engine to bf16 per-op {err:.3e}  '
          f'bar {gap / 30:.3e}')
    assert gap > 0 and err <= gap / 30, (err, gap)
    G = unflatten(net, eng.grads)
    ref, _ = net.loss_backward(eng.params.clone(), planes, fwd, sl['actions'].reshape(-1), sl['returns'].reshape(-1),
                               precision='bf16')
    errs = {t: T.rel_l2(G[t], g) for t, g in unflatten(net, ref).items()}
    print(f'engine {E}x{n} gradient to the per-op bf16 entry: largest {max(errs.values()):.3e}')
    for t, e in errs.items():
        assert e <= 1e-4, (t, e)
    assert lib().a3c_engine_set_precision(eng._h, 7) == ERR_INVALID
    assert lib().a3c_engine_set_precision(None, PREC_BF16) == ERR_INVALID
    eng.close()
    from src.engine import Engine
    nips = Engine(num_envs=4, n_step=2, action_size=6, num_frames=48, seed=1)
    assert lib().a3c_engine_set_precision(nips._h, PREC_BF16) == ERR_INVALID
    nips.close()


# largest error seen on an MI355X, conv1 / conv2 / conv3: the FP32 slot 1.7e-07, 3.7e-07, 3.2e-07 (half the mildest lost
# product: 1.9e-06, 1.4e-06, 1.1e-06), 2.3e-03 .. 2.6e-03 against check_layer's 2.6e-07 .. 4.3e-07; its gradient to the
# per-op fp32 entry 0; bf16 again 8.5e-08, 1.2e-07, 1.0e-07
def test_engine_switch_between_iterations():
    """The sync engine, two bf16 iterations, then FP32 for one rollout, then bf16 again: each rollout follows the
    mode set before it.  The FP32 slot passes the term-split forward bars of tests/_term_split.py (dense data: under
    half the mildest lost product, as tests/test_gpu_term_precision.py holds make_params(scale=4)) and misses
    check_layer's; its gradient is the per-op FP32 entry's on the slot's own activations (1e-4)."""
    E, n = ENGINES[0].values[1:]
    eng, net, P = engine_of(False, E, n, learning_rate=0.0, clip_norm=1e9)
    for _ in range(2):
        eng.iterate()
    eng.set_precision('fp32')
    tau0 = int(eng.counters[0].item())
    eng.rollout_grad()
    torch.cuda.synchronize()
    sl = eng.slot(0)
    planes, _ = rollout_planes(eng, tau0, E, n)
    fwd, outs = slot_forward(sl, E, n)
    check_steps('fp32 after bf16, term-split bars', P, planes, outs, E, n,
                check=lambda tag, P, s, o, layer: fp32_check_layer(tag, P, s, o, CFG, layer, sparse=False)[1])
    for layer, steps in check_steps('fp32 after bf16, the bf16 bar', P, planes, outs, E, n, check=layer_error).items():
        assert all(err > bar for err, bar in steps), (layer, steps)
    G = unflatten(net, eng.grads)
    ref, _ = net.loss_backward(eng.params.clone(), planes, fwd, sl['actions'].reshape(-1), sl['returns'].reshape(-1))
    errs = {t: T.rel_l2(G[t], g) for t, g in unflatten(net, ref).items()}
    print(f'fp32 after bf16: gradient to the per-op fp32 entry, largest {max(errs.values()):.3e}')
    assert max(errs.values()) <= 1e-4, errs
    eng.apply()
    eng.set_precision('bf16')
    tau0 = int(eng.counters[0].item())
    eng.rollout_grad()
    torch.cuda.synchronize()
    planes, _ = rollout_planes(eng, tau0, E, n)
    check_steps('bf16 again', P, planes, slot_forward(sl, E, n)[1], E, n)
    eng.close()


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
