"""Shared Adam (Engine(optimizer='adam'), a3c_clip_adam_apply) on the GPU: the stand-alone op and
the engine in every mode against the numpy restatement tests/_adam_ref.py; the partitioned PS's sequential
steps; graph against eager, resume, the default path untouched, and learning on Catch at the reference's
learning rate, where RMSProp stays at the random policy (§4h).

Engine parity runs the existing checks (_engine_parity, test_gpu_lstm) as they stand -- forward, draws, targets,
losses, gradients, env state -- with the oracle's update replaced: the restated Adam applied on the host to the
engine's own gradient buffer, clipped with the oracle's clip_by_norm.  The oracle's same-activation gradient is
not used for that leg: it differs from the engine's by up to 1e-4 of a tensor's maximum, and for elements that
small Adam turns an O(1) relative difference into an O(lr) difference of the step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import _adam_ref as AR  # noqa: E402
import _catch_ref as C  # noqa: E402
import _engine_parity as EP  # noqa: E402
from oracle import ref_cpu as Rc  # noqa: E402
from oracle.engine_ref import EngineRef  # noqa: E402


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. a3c_clip_adam_apply
SIZES = [3, 4099, 1030]            # under one float4; past one SS_CHUNK (4096) with a tail; padding between tensors


def table():
    offs, off = [], 0
    for s in SIZES:
        offs.append(off)
        off = -(-(off + s) // 64) * 64
    return offs, off


@pytest.mark.parametrize('clip', [0.5, 0.0], ids=['clip', 'noclip'])
def test_adam_op_equals_the_restatement(clip):
    """Three steps; rtol 1e-6, atol 1e-7 (the RMSProp op's bars); the padding between the tensors (random
    parameters, zero gradients, zero slots) is untouched in w, m and v."""
    from src import _lib
    from src._lib import check, lib, ptr, stream_handle
    offs, total = table()
    rng = np.random.default_rng(7)
    w = rng.standard_normal(total).astype(np.float32)
    m, v = np.zeros(total, np.float32), np.zeros(total, np.float32)
    pad = np.ones(total, bool)
    for o, s in zip(offs, SIZES):
        pad[o:o + s] = False
    W, M, V = dev(w), dev(m), dev(v)
    b = _lib.c_i64()
    check(lib().a3c_optim_workspace_bytes(total, ctypes.byref(b)), 'ws')
    ws = torch.empty(int(b.value), dtype=torch.uint8, device='cuda')
    ss = torch.zeros(len(SIZES), device='cuda')
    ref = AR.Adam()
    want = {i: w[o:o + s].copy() for i, (o, s) in enumerate(zip(offs, SIZES))}
    clipped_any = False
    for step in range(3):
        g = np.zeros(total, np.float32)
        for o, s in zip(offs, SIZES):                     # norms on both sides of the clip at 0.5
            g[o:o + s] = rng.standard_normal(s).astype(np.float32) * np.float32(0.05 if s == 1030 else 1.0)
        p1, p2 = ref.advance()
        a = AR.alpha(7e-4, p1, p2)
        check(lib().a3c_clip_adam_apply(ptr(W), ptr(M), ptr(V), ptr(dev(g)), len(SIZES), _lib.i64_array(offs),
                                        _lib.i64_array(SIZES), float(a), AR.BETA1, AR.BETA2, AR.EPS, clip, ptr(ss),
                                        ptr(ws), stream_handle()), 'a3c_clip_adam_apply')
        torch.cuda.synchronize()
        for i, (o, s) in enumerate(zip(offs, SIZES)):
            gi = g[o:o + s]
            assert np.isclose(float(ss[i]), np.sum(gi.astype(np.float64) ** 2), rtol=1e-5)
            gc = Rc.clip_by_norm(gi, clip) if clip > 0 else gi
            clipped_any |= clip > 0 and not np.array_equal(gc, gi)
            ref.update(i, want[i], gc, a)
        got, gm, gv = W.cpu().numpy(), M.cpu().numpy(), V.cpu().numpy()
        for i, (o, s) in enumerate(zip(offs, SIZES)):
            np.testing.assert_allclose(got[o:o + s], want[i], rtol=1e-6, atol=1e-7, err_msg=str((step, i)))
            np.testing.assert_allclose(gm[o:o + s], ref.m[i], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(gv[o:o + s], ref.v[i], rtol=1e-6, atol=1e-7)
        # the pass covers the padding too, as k_apply's does, with its zero gradients and zero slots: nothing moves
        assert pad.sum() > 0 and np.array_equal(got[pad], w[pad]) and (gm[pad] == 0).all() and (gv[pad] == 0).all()
    assert clipped_any == (clip > 0)
    assert np.abs(got[~pad] - w[~pad]).min() > 0


def test_adam_op_rejects_invalid_arguments():
    from src import _lib
    from src._lib import lib, ptr, stream_handle
    offs, total = table()
    t = torch.zeros(total, device='cuda')
    ws = torch.empty(8192, dtype=torch.uint8, device='cuda')
    good = dict(params=ptr(t), m=ptr(t), v=ptr(t), grads=ptr(t), n=len(SIZES), offs=_lib.i64_array(offs),
                sizes=_lib.i64_array(SIZES), ws=ptr(ws))

    def call(**kw):
        a = dict(good, **kw)
        return lib().a3c_clip_adam_apply(a['params'], a['m'], a['v'], a['grads'], a['n'], a['offs'], a['sizes'], 1e-3,
                                         0.9, 0.999, 1e-8, 40.0, None, a['ws'], stream_handle())
    for kw in (dict(params=None), dict(m=None), dict(v=None), dict(grads=None), dict(ws=None), dict(n=0),
               dict(n=_lib.MAX_TENSORS + 1), dict(offs=_lib.i64_array([0, 66, 4224])),          # not 4-aligned
               dict(offs=_lib.i64_array([0, 4224, 64])), dict(offs=_lib.i64_array([0, 0, 4224]))):    # not ascending
        assert call(**kw) == _lib.ERR_INVALID, kw
    assert b'a3c_clip_adam_apply' in lib().a3c_last_error()
    assert call() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. engine parity
def adam_oracle(base, holder):
    """`base` with its update replaced (module docstring).  holder: {'eng', 'ns'}, filled by the start hook."""
    class AdamEngineRef(base):
        def apply_sequence(self, clipped_seq, advance_tau=True, tau=None):
            assert len(clipped_seq) == 1
            if not hasattr(self, 'adam'):
                self.adam = AR.Adam()
            lr = self.next_lr(tau)
            G = EP.unflat(holder['eng'], holder['ns'], holder['eng'].grads)
            self.adam.step(self.params, {k: Rc.clip_by_norm(G[k], self.h['clip_norm']) for k in self.params}, lr)
            self.finish_update(advance_tau)
            return lr
    return AdamEngineRef


class Hooks:
    def __init__(self, A, algo, lstm=False, dqn_type='nips', then=None):
        from src.kernels import param_names_shapes
        self.holder = dict(ns=param_names_shapes(A, algo, lstm=lstm, dqn_type=dqn_type))
        self.then, self.updates = then, 0

    def start(self, eng, ref):
        self.holder['eng'] = eng
        assert eng.optimizer == 'adam' and eng.adam_powers == (1.0, 1.0)
        assert float(eng.ms.abs().max()) == 0.0 and float(eng.mom.abs().max()) == 0.0       # v = m = 0
        self.first_target = {k: v.copy() for k, v in ref.tparams.items()}.get('l3_w') if ref.algo == 'q' else None
        if self.then is not None:
            self.then(eng, ref)

    def on_update(self, it, eng, ref, lr):
        """The products to the last bit, and the step size the schedule left on the device."""
        self.updates += 1
        assert eng.adam_powers == (ref.adam.p1, ref.adam.p2), (it, eng.adam_powers)
        sched = sched_words(eng)                # [0] the schedule's float lr, [2] the alpha formed from it
        assert np.isclose(sched[0], lr, rtol=1e-6) and sched[2] == AR.alpha(sched[0], ref.adam.p1, ref.adam.p2), (it, sched)


def sched_words(eng):
    from src.engine import _view
    return _view(eng.sched_ptr, (4,), torch.float32).cpu().numpy()


CASES = {
    'a3c-sync': dict(check='sync', algo='a3c', A=6, E=8, n=5, lives=0, iters=3),
    'a3c-overlap': dict(check='overlap', algo='a3c', A=6, E=8, n=5, lives=0, iters=5, kw=dict(learning_rate=3e-3)),
    'q-overlap-target-sync': dict(check='overlap', algo='q', A=6, E=8, n=5, lives=3, iters=6,
                                  kw=dict(learning_rate=3e-3, target_q_update_step=40)),
    'nature': dict(check='sync', algo='a3c', A=6, E=8, n=3, lives=0, iters=3,
                   kw=dict(dqn_type='nature', scale=2.0, learning_rate=2e-3, seed=508)),
    'action-repeat-2': dict(check='sync', algo='a3c', A=6, E=8, n=5, lives=3, iters=3, kw=dict(action_repeat=2)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_engine_matches_restated_adam(name, monkeypatch):
    """Three or more updates: parameters within 1e-5 max(1, |w|max) (assert_params, inside the checks), the
    products equal to the last bit, everything else as the existing checks assert it."""
    c = CASES[name]
    kw = dict(c.get('kw', {}), optimizer='adam')
    hooks = Hooks(c['A'], c['algo'], dqn_type=kw.get('dqn_type', 'nips'))
    monkeypatch.setattr(EP, 'EngineRef', adam_oracle(EngineRef, hooks.holder))
    if c['check'] == 'sync':
        eng, ref = EP.check_sync_vs_oracle(c['algo'], c['A'], c['E'], c['n'], c['lives'], iters=c['iters'],
                                           start=hooks.start, on_update=hooks.on_update, **kw)
        assert hooks.updates == c['iters'] >= 3
    else:
        eng, ref = EP.check_overlap_vs_oracle(c['A'], c['E'], c['n'], c['lives'], rollouts=c['iters'], algo=c['algo'],
                                              start=hooks.start, on_update=hooks.on_update, **kw)
        assert hooks.updates == c['iters'] - 1 >= 3
    p1 = 1.0
    for _ in range(hooks.updates):
        p1 *= AR.BETA1
    assert eng.adam_powers[0] == p1 and float(eng.ms.max()) > 0            # v moved
    if c['algo'] == 'q':                       # 40 env steps per update: a target sync fell inside the run
        assert eng.cfg.target_q_update_step == 40 and ref.global_step >= 80
        assert not np.array_equal(ref.tparams['l3_w'], hooks.first_target)


def test_engine_lstm_matches_restated_adam(monkeypatch):
    import test_gpu_lstm as TL
    hooks = Hooks(6, 'a3c', lstm=True)
    monkeypatch.setattr(TL, 'EngineRef', adam_oracle(EngineRef, hooks.holder))
    eng, ref = TL.check_lstm_sync_vs_oracle(6, 8, 5, 3, iters=3, start=hooks.start, on_update=hooks.on_update,
                                            learning_rate=2e-3, optimizer='adam')
    assert hooks.updates == 3 and eng.lstm


def test_engine_with_host_envs_matches_restated_adam(monkeypatch):
    from src.host_env import HostEnvPool
    from test_gpu_host_env import HostSynthEnv
    A, E, n, lives, P = 6, 8, 5, 3, 40
    hooks = Hooks(A, 'a3c')
    monkeypatch.setattr(EP, 'EngineRef', adam_oracle(EngineRef, hooks.holder))

    def pool(seed):
        return HostEnvPool([HostSynthEnv(seed, e, P, A, lives) for e in range(E)], threads=2)
    eng, _ = EP.check_sync_vs_oracle('a3c', A, E, n, lives, iters=3, seed=500 + E, frames=P, host_pool=pool,
                                     start=hooks.start, on_update=hooks.on_update, learning_rate=2e-3, optimizer='adam')
    assert eng.external_env and hooks.updates == 3


# ------------------------------------------------------------------ 3. the partitioned PS's sequential steps
def test_apply_shard_takes_sequential_adam_steps():
    """World 2 on one GPU, the exchange by hand (tests/test_gpu_multirank.py's replay): every rank's per-worker
    clipped gradient is an Adam step of its own, in rank order, step q with the alpha of the products advanced
    q + 1 times; the commit advances them by 2.  Against the sequential restatement on the engines' own
    gradients, at assert_params' bar; the replicas bit-identical."""
    from src.distributed import shard_ranges
    from src.engine import Engine
    from src.initializers import flatten_host, init_params
    from src.kernels import param_names_shapes
    world, E, n, A = 2, 8, 5, 6
    ns = param_names_shapes(A, 'a3c')
    p0 = init_params(ns, seed=4, stddev=0.05)
    engs = []
    for r in range(world):
        eng = Engine(num_envs=E, n_step=n, action_size=A, num_frames=64, seed=11, env_id_base=r * E, world_size=world,
                     split_exchange=0, optimizer='adam', learning_rate=2e-3)
        eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), p0))
        engs.append(eng)
    total = engs[0].params.numel()
    shard, lo, cnt = shard_ranges(total, world)
    w_out = [torch.zeros(shard, device='cuda') for _ in range(world)]
    ref = AR.Adam()
    P = {k: v.copy() for k, v in p0.items()}
    for it in range(3):
        for e in engs:
            e.rollout_grad()
        torch.cuda.synchronize()
        lr = sched_words(engs[0])[0]
        assert lr == sched_words(engs[1])[0]
        grads = [EP.unflat(e, ns, e.grads) for e in engs]                   # clipped per worker by the engine
        assert not np.array_equal(grads[0]['l4_w'], grads[1]['l4_w'])
        for r, e in enumerate(engs):
            recv = torch.cat([engs[x].grads[lo[r]:lo[r] + cnt[r]] for x in range(world)])
            e.apply_shard(recv, world, lo[r], cnt[r], w_out[r])
        gathered = torch.cat(w_out)
        for e in engs:
            e.apply_commit(gathered)
        torch.cuda.synchronize()
        alphas = ref.sequence(P, grads, lr)
        assert alphas[0] != alphas[1]
        for e in engs:
            got = EP.unflat(e, ns, e.params)
            for name, _ in ns:
                d = np.abs(got[name] - P[name]).max()
                assert d <= 1e-5 * max(1.0, np.abs(P[name]).max()), (it, name, d)
            assert e.adam_powers == (ref.p1, ref.p2), it
        assert torch.equal(engs[0].params, engs[1].params)
    p1 = 1.0
    for _ in range(3 * world):
        p1 *= AR.BETA1
    assert ref.p1 == p1
    for e in engs:
        e.close()


def loopback_engine(split, overlap, world=4, E=8):
    return EP.build('a3c', 6, E, 5, 0, seed=31, frames=48, overlap=overlap, world_size=world, split_exchange=split,
                    learning_rate=3e-3, optimizer='adam')


def test_two_phase_partitioned_ps_takes_sequential_adam_steps():
    """The two-phase exchange at world 4 on one GPU (LoopbackPS(split=True): the fc / head part of every range
    on the comm stream behind wait_grad_head, the conv prefix on the caller's stream, one commit): eight
    a3c_engine_apply_shard launches per iteration read the products and the one commit advances them by 4.
    Against the sequential restatement -- the engine's own per-worker-clipped gradient as 4 rank-ordered Adam
    steps -- at assert_params' bar, the products to the last bit."""
    from src.distributed import LoopbackPS
    world = 4
    eng, ref0, ns = loopback_engine(1, False, world)
    assert eng.split_point > 0
    ps = LoopbackPS(eng.params.numel(), world, split=True)
    ref = AR.Adam()
    P = {k: v.copy() for k, v in EP.unflat(eng, ns, eng.params).items()}
    for it in range(3):
        eng.rollout_grad()
        torch.cuda.synchronize()
        G = EP.unflat(eng, ns, eng.grads)
        lr = sched_words(eng)[0]
        ps.apply(eng)
        torch.cuda.synchronize()
        alphas = ref.sequence(P, [G] * world, lr)
        assert len(set(float(a) for a in alphas)) == world
        got = EP.unflat(eng, ns, eng.params)
        for name, _ in ns:
            d = np.abs(got[name] - P[name]).max()
            assert d <= 1e-5 * max(1.0, np.abs(P[name]).max()), (it, name, d)
        assert eng.adam_powers == (ref.p1, ref.p2), it
        assert int(eng.counters[1].item()) == (it + 1) * 5 * 8 * world
    p1 = 1.0
    for _ in range(3 * world):
        p1 *= AR.BETA1
    assert ref.p1 == p1


@pytest.mark.parametrize('overlap', [False, True], ids=['sync', 'overlap'])
def test_two_phase_exchange_equals_one_phase(overlap):
    """Five iterations of Engine.iterate(exchange=LoopbackPS) with Adam: the two-phase exchange, whose shard
    launches run on the comm stream under the conv backward, leaves what the one-phase exchange leaves."""
    from src.distributed import LoopbackPS
    runs = []
    for split in (1, 0):
        eng, _, _ = loopback_engine(split, overlap)
        ps = LoopbackPS(eng.params.numel(), 4, split=bool(split))
        for _ in range(5):
            eng.iterate(exchange=ps)
        torch.cuda.synchronize()
        runs.append(eng)
    a, b = runs
    for name in ('params', 'ms', 'mom', 'grads', 'counters', 'loss', 'frame_ring'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    steps = (4 if overlap else 5) * 4
    p1 = 1.0
    for _ in range(steps):
        p1 *= AR.BETA1
    assert a.adam_powers == b.adam_powers and a.adam_powers[0] == p1


def test_commit_without_shard_is_refused():
    """a3c_engine_apply_commit of a pending gradient with no a3c_engine_apply_shard before it (Hogwild's path)
    has no step count to advance: A3C_ERR_STATE on an Adam engine, and nothing applied."""
    from src import _lib
    eng, _, _ = loopback_engine(0, False, world=2)
    eng.rollout_grad()
    torch.cuda.synchronize()
    before = eng.params.clone()
    with pytest.raises(_lib.A3CError) as ei:
        eng.apply_commit(None)
    assert ei.value.rc == _lib.ERR_STATE and torch.equal(before, eng.params) and eng.adam_powers == (1.0, 1.0)


# ------------------------------------------------------------------ 4. graph equals eager, resume
STATE = ('params', 'target_params', 'ms', 'mom', 'grads', 'loss')
EPS = dict(ep_end_t=12, learn_start=0)
RUN = dict(optimizer='adam', target_q_update_step=40, learning_rate=3e-3, **EPS)


@pytest.mark.parametrize('overlap', [False, True], ids=['sync', 'overlap'])
def test_graph_equals_eager(overlap):
    engs = [EP.build('q', 6, 16, 5, 0, seed=4701, overlap=overlap, use_graph=g, **RUN)[0] for g in (True, False)]
    assert engs[0].cfg.use_graph == 1 and engs[1].cfg.use_graph == 0
    for _ in range(4):
        for eng in engs:
            eng.iterate()
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(engs[0], name), getattr(engs[1], name)), name
    assert engs[0].adam_powers == engs[1].adam_powers != (1.0, 1.0)
    assert float(engs[0].loss[0]) > 0


@pytest.mark.parametrize('algo,overlap', [('a3c', False), ('q', True)], ids=['sync', 'overlap'])
def test_resume_is_bit_for_bit(algo, overlap):
    """3 iterations + save_state + load_state into a fresh engine + 3 iterations = 6 uninterrupted; the state
    carries the products.  An RMSProp engine does not take an Adam engine's state."""
    from src import _lib
    kw = dict(RUN) if algo == 'q' else dict(optimizer='adam', learning_rate=3e-3)

    def make(**over):
        return EP.build(algo, 6, 8, 3, 5, seed=4801, overlap=overlap, **dict(kw, **over))[0]
    a, b = make(), make()
    for _ in range(6):
        a.iterate()
    for _ in range(3):
        b.iterate()
    torch.cuda.synchronize()
    blob = b.save_state()
    c = make()
    c.load_state(blob)
    assert c.adam_powers == b.adam_powers != (1.0, 1.0)
    for _ in range(3):
        c.iterate()
    torch.cuda.synchronize()
    for name in STATE + ('counters', 'frame_ring'):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    assert a.adam_powers == c.adam_powers
    other = make(optimizer='rmsprop')
    with pytest.raises(_lib.A3CError) as ei:
        other.load_state(blob)
    assert ei.value.rc == _lib.ERR_INVALID


def test_checkpoint_restores_slots_and_products_and_falls_back_between_optimizers(tmp_path, capsys):
    """src/checkpoint.py on real engines, without the state blob (the parameters + slots + products path):
    an Adam engine restored from an Adam checkpoint holds the same parameters, m, v and products to the last
    bit; an RMSProp engine restored from the same file takes parameters and step, keeps fresh slots and says so."""
    from src import checkpoint as CK
    kw = dict(optimizer='adam', learning_rate=3e-3)

    def make(**over):
        return EP.build('a3c', 6, 8, 3, 0, seed=4901, **dict(kw, **over))
    a, _, ns = make()
    for _ in range(3):
        a.iterate()
    torch.cuda.synchronize()
    arrays = CK.engine_arrays(a, ns, with_state=False)
    assert 'l4_linear/Matrix/Adam' in arrays and float(arrays['beta1_power']) == a.adam_powers[0]
    b, _, _ = make()
    CK.engine_restore(b, ns, arrays)
    for name in ('params', 'ms', 'mom'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.adam_powers == b.adam_powers and 'slots fresh' not in capsys.readouterr().err
    r, _, _ = make(optimizer='rmsprop')
    CK.engine_restore(r, ns, arrays)
    assert torch.equal(r.params, a.params) and float(r.ms.min()) == 1.0 and float(r.mom.abs().max()) == 0.0
    assert 'slots fresh' in capsys.readouterr().err


# ------------------------------------------------------------------ 5. Adam off changes nothing; 6. Adam is not RMSProp
@pytest.mark.parametrize('E,overlap', [(8, False), (16, True)], ids=['sync', 'overlap'])
def test_adam_off_changes_nothing(E, overlap):
    """Engine(optimizer='rmsprop'), which calls a3c_engine_set_optimizer, against an engine built without the
    argument, which does not: four iterations leave the same parameters, slots, gradient and loss."""
    kw = dict(overlap=overlap, learning_rate=3e-3)
    a, _, _ = EP.build('a3c', 6, E, 5, 5, seed=5001 + E, optimizer='rmsprop', **kw)
    b, _, _ = EP.build('a3c', 6, E, 5, 5, seed=5001 + E, **kw)
    assert a.optimizer == b.optimizer == 'rmsprop' and a.adam_powers == b.adam_powers == (1.0, 1.0)
    for _ in range(4):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('params', 'ms', 'mom', 'grads', 'loss', 'counters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.loss[3]) != 0 and a.adam_powers == (1.0, 1.0)


def test_adam_is_not_rmsprop():
    kw = dict(learning_rate=3e-3)
    a, _, _ = EP.build('a3c', 6, 8, 5, 0, seed=5101, optimizer='adam', **kw)
    b, _, _ = EP.build('a3c', 6, 8, 5, 0, seed=5101, **kw)
    assert torch.equal(a.params, b.params)
    a.iterate()
    b.iterate()
    torch.cuda.synchronize()
    assert torch.equal(a.grads, b.grads) and not torch.equal(a.params, b.params)
    assert float(a.ms.max()) < 0.9 < float(b.ms.min())            # v starts at 0, RMSProp's rms at 1


def test_setter_states_and_rejections():
    from src import _lib
    from src.engine import Engine
    L = _lib.lib()
    eng = Engine(num_envs=4, n_step=2, num_frames=8)
    for args in ((2, 0.9, 0.999, 1e-8), (1, 1.0, 0.999, 1e-8), (1, 0.9, -0.5, 1e-8), (1, 0.9, 0.999, 0.0)):
        assert L.a3c_engine_set_optimizer(eng._h, *args) == _lib.ERR_INVALID, args
    assert L.a3c_engine_set_adam_powers(eng._h, 0.5, 0.5, None) == _lib.ERR_INVALID        # an RMSProp engine
    eng.reset()
    eng.rollout_grad()                                     # a gradient pending
    assert L.a3c_engine_set_optimizer(eng._h, 1, 0.9, 0.999, 1e-8) == _lib.ERR_STATE
    eng.apply()
    assert L.a3c_engine_set_optimizer(eng._h, 1, 0.9, 0.999, 1e-8) == 0
    torch.cuda.synchronize()
    assert float(eng.ms.abs().max()) == 0.0 and float(eng.mom.abs().max()) == 0.0 and eng.adam_powers == (1.0, 1.0)
    eng.iterate()
    assert eng.adam_powers == (0.9, 0.999)
    eng.reset()
    assert eng.adam_powers == (1.0, 1.0) and float(eng.ms.abs().max()) == 0.0
    eng.adam_powers = (0.81, 0.998001)
    assert eng.adam_powers == (0.81, 0.998001)
    assert L.a3c_engine_set_optimizer(eng._h, 0, 0.9, 0.999, 1e-8) == 0
    torch.cuda.synchronize()
    assert float(eng.ms.min()) == 1.0 and eng.adam_powers == (1.0, 1.0)
    eng.close()
    with pytest.raises(ValueError, match='unknown optimizer'):
        Engine(num_envs=4, n_step=2, num_frames=8, optimizer='adagrad')
    adam = Engine(num_envs=4, n_step=2, num_frames=8, optimizer='adam')
    adam.reset()
    with pytest.raises(ValueError, match='Hogwild'):       # out of scope: refused before the rollout
        adam.iterate_hogwild(None)
    assert int(adam.counters[0]) == 3 and not adam.grad_ready
    adam.close()


def test_drop_in_optimizer_through_network():
    """AdamOptimizer behind Network.apply_gradients (the drop-in API takes it unchanged): two steps against the
    restatement, the products kept per parameter buffer."""
    from src.network import Network
    from src.optim import AdamOptimizer
    opt = AdamOptimizer(7e-4, clip_norm=40.0)
    glob_net = Network(None, 'NHWC', 4, 84, 84, 6, beta=0.01, DQN_type='nips')
    local = Network(None, 'NHWC', 4, 84, 84, 6, beta=0.01, DQN_type='nips', global_network=glob_net, global_optim=opt)
    local.copy_from_global()
    rng = np.random.default_rng(5)
    planes = torch.as_tensor(rng.integers(0, 256, (5, 4, 84, 84), dtype=np.uint8)).cuda()
    ref = AR.Adam()
    w = glob_net.flat.cpu().numpy().copy()
    for step in range(2):
        grads, _ = local.loss_backward(planes, [0, 1, 2, 3, 4], [1.0, -1.0, 0.5, 0.0, 2.0])
        g = grads.cpu().numpy().copy()
        local.apply_gradients(grads, lr=1e-3)
        a = AR.alpha(1e-3, *ref.advance())
        got = glob_net.flat.cpu().numpy()
        for (name, shp), o, n in zip(local.names_shapes, local.offsets, local.sizes):
            ref.update(name, w[o:o + n], Rc.clip_by_norm(g[o:o + n], 40.0), a)
            np.testing.assert_allclose(got[o:o + n], w[o:o + n], rtol=1e-6, atol=1e-7, err_msg=name)
        local.copy_from_global()
    assert opt.powers(glob_net.flat) == [ref.p1, ref.p2]


# ------------------------------------------------------------------ 7. learning
# §4h's epsilon schedule and target period, the reference's learning rate
LEARN = dict(learn_start=0, ep_end_t=1000, target_q_update_step=12800, learning_rate=7e-4)
LEARN_K = 1024       # measured: see the docstring


def test_adam_learns_catch_at_the_reference_learning_rate():
    """The setting in which §4h records that RMSProp stays at the random policy: the overlapped Q engine with
    q_nstep = 1 (n-step Q-learning) on Catch, 256 envs, n = 5, the reference initialisers, §4h's epsilon schedule
    (annealed over 1000 env steps per env) and target period (a sync every 10 iterations), and the reference's
    learning_rate = 7e-4 -- with optimizer='adam' at its defaults.  Trained LEARN_K iterations on seed 1, then
    1024 greedy episodes with refill.  The bar is §4g's, halfway from the random policy's exact return to the
    optimal one, 0.125: the untrained parameters play below it, the trained ones at or above it.  Without the
    feature the engine has no optimizer argument and the test fails at the constructor.

    LEARN_K: mean greedy play return against iterations, measured on one MI355X for seeds 1 / 2 / 3
    (tools/adam_learning.py; the RMSProp column from the same run, reported only):
      adam, 7e-4      0: -0.836 / -0.840 / -0.852,  64: -0.578 / -0.666 / -0.502,  128: -0.666 / -0.338 / -0.168,
                      256: 0.809 / -0.188 / -0.148,  512 .. 8192: 1.0 / 1.0 / 1.0
      rmsprop, 7e-4   512: -0.688 / -0.647 / -0.736,  1024: -0.711 / -0.643 / -0.662,  2048: -0.818 / -0.936 / -0.426,
                      4096: -0.881 / -0.725 / -0.443,  8192: -0.492 / -0.250 / -0.479
    The smallest power of two at which all three Adam seeds clear the bar is 512; LEARN_K is twice that (0.3 s of
    training).  Adam cleared the bar at 7e-4, so no scan over other rates was made.  (One-step Q, q_nstep = 0, in
    DESIGN §4j: also 512.)"""
    import main
    from src.engine import Engine
    seed, A = 1, 3
    eng = Engine(num_envs=256, n_step=5, action_size=A, algo='q', overlap=True, seed=seed, num_frames=C.FRAMES,
                 game='catch', optimizer='adam', q_nstep=1, **LEARN)
    eng.reset(main.initial_params(eng, A, 'q', seed))
    eng.target_params.copy_(eng.params)
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    play = dict(n_episode=1024, n_step=50, refill=True, test_ep=0.0)
    before = eng.play(**play)
    for _ in range(LEARN_K):
        eng.iterate()
    torch.cuda.synchronize()
    after = eng.play(**play)
    for out in (before, after):
        assert (out['lengths'] == C.ROWS - 1).all() and out['terminated'].all()
    r0, r1 = float(before['returns'].mean()), float(after['returns'].mean())
    print('catch, n-step q, adam, lr 7e-4: mean greedy return untrained', r0, 'after', LEARN_K, 'iterations', r1,
          'bar', C.LEARNING_BAR)
    assert C.LEARNING_BAR == 0.125 and eng.optimizer == 'adam' and abs(eng.cfg.learning_rate - 7e-4) < 1e-9
    assert eng.cfg.q_nstep == 1 and eng.algo == 'q' and eng.overlap
    assert r0 < C.LEARNING_BAR, (r0, C.LEARNING_BAR)
    assert r1 >= C.LEARNING_BAR, (r1, C.LEARNING_BAR)
    eng.close()
