"""End-to-end parity of the batched actor-learner engine (graph-captured HIP path) against the
CPU replay oracle/engine_ref.py on fixed seeds: env dynamics and frames bit-exact, action draws
consistent, returns / losses within 1e-5 relative (north star bar: 1e-3), gradients within 1e-4,
parameters after RMSProp within 1e-5 over several iterations."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from _engine_parity import (build, check_hogwild1_vs_oracle, check_overlap_vs_oracle,  # noqa: E402
                            check_sync_vs_oracle, rel_l2)


@pytest.mark.parametrize('algo,A,E,n,lives', [('a3c', 6, 8, 5, 0), ('a3c', 4, 6, 3, 5), ('q', 6, 4, 8, 3),
                                               ('a3c', 6, 1, 5, 0), ('a3c', 6, 37, 2, 3)])
def test_engine_matches_oracle(algo, A, E, n, lives):
    check_sync_vs_oracle(algo, A, E, n, lives)


@pytest.mark.parametrize('algo,A,E,n,lives', [('a3c', 6, 8, 5, 0), ('q', 6, 4, 8, 3)])
def test_frame84_mode_matches_oracle(algo, A, E, n, lives):
    """Measurement mode M2: pre-sized 84x84 pool frames copied into the history
    ring instead of Environment.screen of RGB frames; the same parity bar as the RGB mode."""
    check_sync_vs_oracle(algo, A, E, n, lives, frame84=1)


@pytest.mark.parametrize('overlap', [False, True])
def test_engine_deterministic_and_graph_equals_eager(overlap):
    a, _, ns = build('a3c', 6, 16, 5, 0, seed=7, use_graph=True, overlap=overlap)
    b, _, _ = build('a3c', 6, 16, 5, 0, seed=7, use_graph=False, overlap=overlap)
    for _ in range(4):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.frame_ring, b.frame_ring)
    assert torch.equal(a.loss, b.loss)


@pytest.mark.parametrize('overlap', [False, True])
def test_fused_iterate_equals_rollout_grad_then_apply(overlap):
    """a3c_engine_iterate (apply captured into the graphs) == a3c_engine_rollout_grad +
    a3c_engine_apply, bit for bit (params, RMSProp slots, frames, losses, counters)."""
    a, _, _ = build('a3c', 6, 16, 5, 0, seed=11, overlap=overlap)
    b, _, _ = build('a3c', 6, 16, 5, 0, seed=11, overlap=overlap)
    for _ in range(5):
        a.iterate()                       # fused path
        b.rollout_grad()                  # split path
        assert a.grad_ready == b.grad_ready
        if b.grad_ready:
            b.apply()
        a.apply()                         # no-op: the fused iterate applied already
    torch.cuda.synchronize()
    for name in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('overlap', [False, True])
def test_conv_fusion_is_bit_exact(overlap, monkeypatch):
    """k_head_screen_conv12 (step t+1's conv1 + conv2 inside step t's head + screen kernel) gives
    the same rollouts, activations and updates as the separate kernels, bit for bit."""
    engs = []
    monkeypatch.setenv('A3C_FC_SPLIT', '0')     # the same fc kernel in both (see the next test)
    for fuse in ('0', '1'):
        monkeypatch.setenv('A3C_FUSE_CONV', fuse)
        engs.append(build('a3c', 6, 16, 5, 0, seed=13, overlap=overlap)[0])
    a, b = engs
    for _ in range(4):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters', 'actions', 'act_l1', 'act_l2', 'z'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('E', [16, 256])
def test_fc_split_matches_monolithic_fc(E, monkeypatch):
    """Fused overlap rollout: the fc as K-slice partials (k_fc_part) folded by the head of
    k_head_screen_conv12 equals the single-pass fc kernel up to fp32 summation order -- same
    rollouts (actions, frames, rewards), layer outputs and updates to 1e-5."""
    engs = []
    for split in ('0', '1'):
        monkeypatch.setenv('A3C_FC_SPLIT', split)
        engs.append(build('a3c', 6, E, 5, 0, seed=21, overlap=True, frames=512)[0])
    a, b = engs
    for _ in range(4):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('actions', 'frame_ring', 'counters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ('act_l3', 'z', 'params', 'ms', 'mom', 'loss'):
        x, y = getattr(a, name).double(), getattr(b, name).double()
        err = (x - y).norm() / max(y.norm().item(), 1e-30)
        assert err < 1e-5, (name, float(err))


def test_engine_bench_shape_runs():
    """The bench configuration (Pong, 256 envs, n=5) runs and stays finite."""
    eng, _, ns = build('a3c', 6, 256, 5, 0, seed=123, frames=256, scale=1.0)
    for _ in range(3):
        eng.iterate()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.params).all()
    assert torch.isfinite(eng.loss).all()
    acts = eng.actions.cpu().numpy()
    assert acts.min() >= 0 and acts.max() < 6


# ------------------------------------------------------------------ overlap (stale-1) pipeline
def test_overlap_with_zero_lr_equals_sync():
    """With learning_rate 0 staleness is invisible: the pipelined engine must reproduce the
    synchronous engine's rollouts exactly (actions, rewards) one call later, and its returns,
    losses and gradients to fp32 summation order (the two modes run different-footprint kernel
    variants: LaunchMode::shared_gpu in csrc/net.h, which each engine fixes at create)."""
    s, _, _ = build('a3c', 6, 16, 5, 0, seed=31, learning_rate=0.0)
    o, _, _ = build('a3c', 6, 16, 5, 0, seed=31, learning_rate=0.0, overlap=True)
    assert o.ring_slots == 2 * 5 + 4 and s.ring_slots == 5 + 4
    o.iterate()
    torch.cuda.synchronize()
    assert not o.grad_ready
    for k in range(1, 5):
        s.iterate()
        o.iterate()
        torch.cuda.synchronize()
        assert o.grad_ready
        prev = o.slot((k - 1) & 1)
        assert torch.equal(prev['actions'], s.actions), k
        assert torch.equal(prev['rewards'], s.rewards), k
        torch.testing.assert_close(prev['returns'], s.returns, rtol=1e-5, atol=1e-6)
        # the loss terms are sums over n*E samples with cancellation (policy term): fp32
        # summation-order differences between the modes' kernel variants show at ~2e-5 relative
        torch.testing.assert_close(o.loss, s.loss, rtol=1e-4, atol=1e-4)
        # (the conv backward partitions the samples differently per mode: 256 vs 224 workgroup
        # slabs, so dW1's cancelling sums differ in fp32 order, ~1e-5 relative-L2)
        assert rel_l2(o.grads.cpu().numpy(), s.grads.cpu().numpy()) < 5e-5, k
        assert torch.equal(o.params, s.params), k          # lr = 0: parameters never move
    assert int(o.counters[0].item()) == int(s.counters[0].item()) + 5     # one rollout ahead
    assert int(o.counters[1].item()) == int(s.counters[1].item())


@pytest.mark.parametrize('E,frame84', [(8, 0), (8, 1), (1, 0), (37, 0)])
def test_overlap_stale_semantics_match_oracle(E, frame84):
    """Rollout k uses the parameters after update k-2 (staleness 1): replay that order on the
    oracle with the engine's own actions and activations; parameters agree at 1e-5 (RGB frames,
    and the pre-sized 84x84 frames of measurement mode M2; one env, and a ragged 37 that leaves
    partial row blocks in the partial fc, the bootstrap head and the conv backward's groups)."""
    check_overlap_vs_oracle(6, E, 5, 0, rollouts=5, seed=77, learning_rate=3e-3, frame84=frame84)


@pytest.mark.parametrize('E,tq', [(8, 100), (37, 2000)])
def test_q_overlap_stale_semantics_match_oracle(E, tq):
    """Async Q-learning on the stale-1 pipeline: rollout k acts epsilon-greedily with the
    parameters after update k-2, and rollout k-1's TD targets are formed by its backward (after
    rollout k) with the target network as it stands then; the target copy follows the apply's
    global step (agent.py:166-167).  tq=100 at 40 env steps per update syncs on irregular updates."""
    check_overlap_vs_oracle(6, E, 5, 0, rollouts=6, seed=55, learning_rate=3e-3, algo='q',
                            target_q_update_step=tq)


@pytest.mark.parametrize('overlap', [False, True], ids=['sync', 'overlap'])
def test_double_q_matches_oracle(overlap):
    """--double_q (agent.py:176-184): the TD target takes the target net's q of s_{t+1} at the
    online net's argmax -- the engine's own q rows of the rollout plus one online forward of the
    bootstrap state s_n -- checked against the oracle's double-Q targets, then losses, gradients
    and parameters as for the vanilla target (overlap: the online net is the one the rollout ran)."""
    if overlap:
        check_overlap_vs_oracle(6, 8, 5, 3, rollouts=6, seed=57, learning_rate=3e-3, algo='q',
                                target_q_update_step=100, double_q=1)
    else:
        check_sync_vs_oracle('q', 6, 4, 8, 3, iters=4, learning_rate=3e-3, double_q=1)


@pytest.mark.parametrize('E', [8, 37])
@pytest.mark.parametrize('mode', ['overlap', 'sync'])
def test_hogwild_world1_matches_oracle(mode, E):
    """Hogwild at world 1 (src/hogwild.py: per-worker clip, unlocked RMSProp push into the sharded
    PS, pull) at small shapes, overlapped with the next rollout at staleness 1 or after each rollout:
    every bar of the plain update modes, the saved activations and the clipped independent gradient
    included (E = 37: a ragged row block, as in the a3c overlap test)."""
    if mode == 'overlap':
        check_overlap_vs_oracle(6, E, 5, 0, rollouts=5, seed=81, learning_rate=3e-3, hogwild=True)
    else:
        check_hogwild1_vs_oracle(6, E, 5, 0, iters=3, seed=83, learning_rate=3e-3)


def test_stream_ordering_modes_are_bit_identical(monkeypatch):
    """Overlap pipeline: ordering the rollout and backward streams by stream wait-value operations
    on device counters (default) or by HIP events gives the same training, bit for bit."""
    engs = []
    for wv in ('0', '1'):
        monkeypatch.setenv('A3C_WAIT_VALUE', wv)
        engs.append(build('a3c', 6, 32, 5, 0, seed=17, overlap=True, frames=256)[0])
    a, b = engs
    for _ in range(6):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters', 'actions', 'z'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('frame84', [0, 1])
def test_relu_bits_equal_l2_reread(monkeypatch, frame84):
    """The dl2 GEMM's ReLU mask from the forward's ballot bits (EPI_MASKBITS, the default where the
    backward bounds: M2) and from re-reading l2 (EPI_MASK, the default in M1) train bit for bit
    alike: the same mask, the same sums."""
    engs = []
    for bits in ('1', '0'):
        monkeypatch.setenv('A3C_L2BITS', bits)
        engs.append(build('a3c', 6, 64, 5, 0, seed=23, overlap=True, frames=256, frame84=frame84)[0])
    a, b = engs
    for _ in range(5):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('params', 'ms', 'mom', 'grads', 'loss', 'actions', 'z'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('overlap,frame84', [(False, 0), (True, 0), (True, 1)])
def test_bench_shape_is_deterministic(overlap, frame84):
    """At the bench configuration (Pong, 256 envs, n=5) two engines from the same seed train bit for
    bit alike: every reduction is fixed-order (slab folds, sum of squares), no atomics."""
    engs = [build('a3c', 6, 256, 5, 0, seed=29, frames=512, scale=1.0, overlap=overlap, frame84=frame84)[0]
            for _ in range(2)]
    for _ in range(4):
        for e in engs:
            e.iterate()
    torch.cuda.synchronize()
    a, b = engs
    for name in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters', 'actions', 'z', 'act_l3'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.isfinite(a.params).all() and torch.isfinite(a.loss).all()


def test_engines_of_both_modes_interleave_bit_exact():
    """The kernel variants a launch takes (LaunchMode, csrc/net.h) belong to the engine, not to the
    calling thread: a sync and an overlap engine driven in turn from one thread, with a play() and a
    time_kernel() between their iterations, train bit for bit as their twins (same seed, same mode)
    do when each runs on its own.  Both sides are the same build: no tolerance."""
    from src import _lib

    def pair():
        return (build('a3c', 6, 16, 5, 0, seed=41, frames=256)[0],
                build('a3c', 6, 16, 5, 0, seed=43, frames=256, overlap=True)[0])
    a_sync, a_over = pair()
    b_sync, b_over = pair()
    for eng in (a_sync, a_over):
        for _ in range(5):
            eng.iterate()
    for r in range(5):
        b_sync.iterate()
        b_over.iterate()
        if r == 2:
            # neither touches the training state that outlives the next rollout: play() has a context of
            # its own, the timed head + screen launches write what rollout step 0 writes again
            b_over.play(n_episode=16, n_step=8)
            b_sync.time_kernel(_lib.KER_HEAD_SCREEN, 2)
    torch.cuda.synchronize()
    for a, b, mode in ((a_sync, b_sync, 'sync'), (a_over, b_over, 'overlap')):
        for name in ('params', 'ms', 'mom', 'frame_ring', 'loss', 'counters', 'actions', 'z'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (mode, name)
