"""C5 LSTM policy head (BASELINE config 5, SpaceInvaders-v0 LSTM): HIP kernels and the engine's
recurrent path against the CPU oracle (oracle/ref_cpu.py lstm_*, oracle/engine_ref.py lstm=True).
The reference has no recurrent code, so the oracle is a build-defined restatement of TF1
BasicLSTMCell, pinned by torch autograd (tests/test_oracle_autograd.py) -- parity unpinned
against a reference execution.  Tolerances: cell outputs 1e-5 relative (fp32 MFMA vs fp64),
BPTT gradients 1e-4 relative-L2, engine losses 1e-4 (north star 1e-3)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import ref_cpu as Rc  # noqa: E402
from oracle.engine_ref import EngineRef  # noqa: E402
import _plan as PL  # noqa: E402
from _net_parity import GUARD  # noqa: E402
from _engine_parity import (REF_KEYS, EpisodeCount, assert_draws_explained, assert_env_state,  # noqa: E402
                            assert_independent_grads, assert_saved_acts, report_independent)

NOT_LSTM = ('dqn_type', 'double_q', 'target_q_update_step')     # options of the other heads / of Q-learning

U = 256


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _lstm_params(seed, scale=0.06):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((512, 1024)) * scale).astype(np.float32)
    b = (rng.standard_normal(1024) * 0.1).astype(np.float32)
    return w, b


@pytest.mark.parametrize('B', [1, 16, 37, 256])
def test_lstm_step_matches_oracle(B):
    from src import kernels as K
    rng = np.random.default_rng(B)
    w, b = _lstm_params(B)
    x = np.maximum(rng.standard_normal((B, 256)), 0).astype(np.float32)
    h = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    c = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    terms = (rng.random(B) < 0.3).astype(np.uint8)
    dev = lambda a: torch.as_tensor(a).cuda()  # noqa: E731
    out = K.lstm_step(dev(w), dev(b), dev(x), dev(h), dev(c), dev(terms))
    torch.cuda.synchronize()
    keep = (1 - terms.astype(np.float64))[:, None]
    hr, cr, gr = Rc.lstm_cell(x.astype(np.float64), h * keep, c * keep, w.astype(np.float64), b.astype(np.float64))
    # fp32 MFMA accumulation over K = 512 of O(1) terms: ~1e-6 absolute on the preactivations
    np.testing.assert_allclose(out['h'].cpu().numpy(), hr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(out['c'].cpu().numpy(), cr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(out['gates'].cpu().numpy(), gr, rtol=1e-5, atol=5e-6)
    assert np.array_equal(out['hp'].cpu().numpy(), (h * keep).astype(np.float32))
    assert np.array_equal(out['cp'].cpu().numpy(), (c * keep).astype(np.float32))
    # no mask / no saved tensors
    out2 = K.lstm_step(dev(w), dev(b), dev(x), dev(h), dev(c), None, save=False)
    hr2, _, _ = Rc.lstm_cell(x.astype(np.float64), h.astype(np.float64), c.astype(np.float64), w.astype(np.float64),
                             b.astype(np.float64))
    np.testing.assert_allclose(out2['h'].cpu().numpy(), hr2, rtol=1e-5, atol=5e-6)


def _guarded(rows, cols):
    """[rows + 1, cols] filled with GUARD: the kernel owns rows 0..rows-1, the last row shows a write
    one row past the end."""
    return torch.full((rows + 1, cols), GUARD, dtype=torch.float32, device='cuda')


def _guard_intact(t):
    return bool((t[-1] == GUARD).all())


@pytest.mark.parametrize('B', [15, 17])
def test_lstm_step_env_tile_edges_guarded(B):
    """a3c_lstm_step one env short of k_lstm_fwd's 16-env tile and one over (a second, one-env
    tile), called through the C entry on caller buffers: every output has a row of sentinels behind
    row B - 1, which a store of the tile's unused rows would overwrite."""
    from src import _lib
    assert (B + 1) % PL.LSTM_TILE == 0 or (B - 1) % PL.LSTM_TILE == 0
    rng = np.random.default_rng(B)
    w, b = _lstm_params(B)
    x = np.maximum(rng.standard_normal((B, 256)), 0).astype(np.float32)
    h = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    c = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    terms = (rng.random(B) < 0.3).astype(np.uint8)
    dev = lambda a: torch.as_tensor(a).cuda()  # noqa: E731
    wd, bd, xd, hd, cd, td = dev(w), dev(b), dev(x), dev(h), dev(c), dev(terms)
    w_t = torch.empty((1024, 512), dtype=torch.float32, device='cuda')
    out = dict(hp=_guarded(B, U), cp=_guarded(B, U), gates=_guarded(B, 4 * U), h=_guarded(B, U), c=_guarded(B, U))
    ptr, L = _lib.ptr, _lib.lib()
    _lib.check(L.a3c_lstm_transpose(ptr(wd), ptr(w_t), _lib.stream_handle()), 'a3c_lstm_transpose')
    _lib.check(L.a3c_lstm_step(ptr(w_t), ptr(bd), ptr(xd), ptr(hd), ptr(cd), ptr(td), B, ptr(out['hp']), ptr(out['cp']),
                               ptr(out['gates']), ptr(out['h']), ptr(out['c']), _lib.stream_handle()), 'a3c_lstm_step')
    torch.cuda.synchronize()
    for k, v in out.items():
        assert _guard_intact(v), k
    keep = (1 - terms.astype(np.float64))[:, None]
    hr, cr, gr = Rc.lstm_cell(x.astype(np.float64), h * keep, c * keep, w.astype(np.float64), b.astype(np.float64))
    got = {k: v[:B].cpu().numpy() for k, v in out.items()}
    np.testing.assert_allclose(got['h'], hr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(got['c'], cr, rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(got['gates'], gr, rtol=1e-5, atol=5e-6)
    assert np.array_equal(got['hp'], (h * keep).astype(np.float32))
    assert np.array_equal(got['cp'], (c * keep).astype(np.float32))


def _bptt_case(n, E):
    """Inputs of a BPTT over [n, E] (the oracle's own fp64 forward, rounded to float32) and the
    oracle's backward on them: (device-ready arrays, (dX masked by x > 0, dW, dB))."""
    rng = np.random.default_rng(100 + E)
    w, b = _lstm_params(E)
    prm = {'lstm_w': w, 'lstm_b': b}
    x = np.maximum(rng.standard_normal((n, E, 256)) - 0.3, 0).astype(np.float32)
    terms = (rng.random((n, E)) < 0.2).astype(np.uint8)
    h0 = (rng.standard_normal((E, U)) * 0.3).astype(np.float32)
    c0 = (rng.standard_normal((E, U)) * 0.3).astype(np.float32)
    seq = Rc.lstm_forward_seq(prm, x.astype(np.float64), h0.astype(np.float64), c0.astype(np.float64), terms)
    seq32 = {k: seq[k].astype(np.float32) for k in ('HP', 'CP', 'G', 'C')}
    dH = rng.standard_normal((n, E, U)).astype(np.float32)
    s64 = {k: v.astype(np.float64) for k, v in seq32.items()}
    dX, dW, dB = Rc.lstm_backward_seq(prm, s64, x.astype(np.float64), dH.astype(np.float64), terms)
    return (w, x, seq32['HP'], seq32['CP'], seq32['G'], seq32['C'], terms, dH), (dX * (x > 0), dW, dB)


@pytest.mark.parametrize('n,E', [(5, 37), (1, 16), (5, 256)])
def test_lstm_bptt_matches_oracle(n, E):
    from src import kernels as K
    args, (dX, dW, dB) = _bptt_case(n, E)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dx, dw, db = K.lstm_bptt(*[dev(a) for a in args])
    torch.cuda.synchronize()
    assert rel_l2(dx.cpu().numpy(), dX) < 1e-5
    assert rel_l2(dw.cpu().numpy(), dW) < 1e-5
    assert rel_l2(db.cpu().numpy(), dB) < 1e-5


# measured rel-L2 of dx / dw / db, then the largest per-gate one of dw and db:
#   (2, 17)   2.1e-07 / 9.6e-08 / 1.1e-07, per gate 1.2e-07
#   (3, 87)   2.2e-07 / 1.3e-07 / 1.5e-07, per gate 1.9e-07
@pytest.mark.parametrize('n,E', [(2, 17), (3, 87)])
def test_lstm_bptt_short_sequences_guarded_per_gate(n, E):
    """a3c_lstm_bptt through the C entry on caller buffers with a row of sentinels behind dx, dw and
    db.  n = 2 is one fused step (d[x, hp]_1 GEMM + dx_1 + cell backward of step 0) plus dx_0, with
    E = 17 one env over the 16-env tile of k_lstm_bptt_step and a 3-way split of the dW GEMM over 3
    k-tiles; (3, 87) a ragged tile (87 = 5 * 16 + 7) and the 4-way split over 17 k-tiles.  Beside the
    whole-tensor bound, dW and db are held to it per gate (four blocks of 256 columns: i, j, f, o),
    so an error confined to one gate is not diluted fourfold."""
    from src import _lib
    ws_plan = PL.lstm_ws(n, E)
    assert E % PL.LSTM_TILE and (ws_plan.split_dw, PL.cdiv(n * E, PL.BK)) == {(2, 17): (3, 3), (3, 87): (4, 17)}[(n, E)]
    args, (dX, dW, dB) = _bptt_case(n, E)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    w, x, hp, cp, gates, c, terms, dh = [dev(a) for a in args]
    dx, dw, db = _guarded(n * E, 256), _guarded(512, 1024), _guarded(1, 1024)
    ws = torch.empty(PL.lstm_workspace_bytes(n, E), dtype=torch.uint8, device='cuda')
    ptr = _lib.ptr
    _lib.check(_lib.lib().a3c_lstm_bptt(ptr(w), n, E, ptr(x), ptr(hp), ptr(cp), ptr(gates), ptr(c), ptr(terms), ptr(dh),
                                        ptr(dx), ptr(dw), ptr(db), ptr(ws), _lib.stream_handle()), 'a3c_lstm_bptt')
    torch.cuda.synchronize()
    assert _guard_intact(dx) and _guard_intact(dw) and _guard_intact(db)
    dx, dw, db = dx[:-1].cpu().numpy().reshape(n, E, 256), dw[:-1].cpu().numpy(), db[0].cpu().numpy()
    errs = [rel_l2(dx, dX), rel_l2(dw, dW), rel_l2(db, dB)]
    gate = [rel_l2(dw[:, g * U:(g + 1) * U], dW[:, g * U:(g + 1) * U]) for g in range(4)]
    gate += [rel_l2(db[g * U:(g + 1) * U], dB[g * U:(g + 1) * U]) for g in range(4)]
    print(f'lstm bptt n={n} E={E}: dx {errs[0]:.1e} dw {errs[1]:.1e} db {errs[2]:.1e} per gate max {max(gate):.1e}')
    assert max(errs) < 1e-5, errs
    assert max(gate) < 1e-5, gate


# ------------------------------------------------------------------ engine (C5)
def build(A, E, n, lives, seed, frames=48, scale=4.0, params=None, **kw):
    """(params(names_shapes) -> {name: array}: the initial parameters, in place of the usual init.)"""
    from src.engine import Engine
    from src.initializers import init_params, flatten_host
    from src.kernels import param_names_shapes
    eng = Engine(num_envs=E, n_step=n, action_size=A, algo='a3c', start_lives=lives, num_frames=frames, seed=seed,
                 lstm=True, **kw)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    p = init_params(ns, seed=seed, stddev=0.02 * scale) if params is None else params(ns)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), p))
    ref = EngineRef(p, E, n, A, 'a3c', lives, frames, seed, lstm=True,
                    **{k: v for k, v in kw.items() if k in REF_KEYS and k not in NOT_LSTM})
    ref.reset()
    return eng, ref, ns


def unflat(eng, ns, flat):
    f = flat.cpu().numpy()
    return {name: f[off:off + sz].reshape(shp) for (name, shp), off, sz in zip(ns, eng.offsets, eng.sizes)}


def same_act_grads(slot, planes, P, A, n, E, tgt, terms, beta=0.01, literal_adv=False):
    """oracle backward (heads, BPTT, trunk) on the engine's own saved activations and LSTM sequence."""
    B = n * E
    l1 = slot['act_l1'].cpu().numpy().astype(np.float64).reshape(B, 20, 20, 16)
    l2 = slot['act_l2'].cpu().numpy().astype(np.float64)
    z = slot['z'].cpu().numpy()[:n].reshape(B, -1)[:, :A + 1].astype(np.float64)
    h3 = slot['act_l3'].cpu().numpy().astype(np.float64)
    seq = {'H': slot['lstm_h'], 'C': slot['lstm_c'], 'HP': slot['lstm_hp'], 'CP': slot['lstm_cp'],
           'G': slot['lstm_gates']}
    seq = {k: v.cpu().numpy().astype(np.float64) for k, v in seq.items()}
    fwd = dict(z=z, h3=h3, flat=l2, lstm=seq, x_seq=h3.reshape(n, E, -1),
               acts=[Rc.states_nhwc(planes).astype(np.float64) / 255.0, l1, l2.reshape(B, 9, 9, 32)])
    acts = slot['actions'].cpu().numpy().reshape(-1)
    losses, dz = Rc.a3c_loss_and_dz(z, acts, tgt.reshape(-1).astype(np.float64), beta, bool(literal_adv))
    g = Rc.lstm_a3c_backward(P, fwd, dz, terms)
    return losses, {k: np.asarray(v, np.float32).reshape(P[k].shape) for k, v in g.items()}


@pytest.mark.parametrize('A,E,n,lives', [(6, 8, 5, 3), (4, 20, 3, 5), (18, 8, 3, 3)])
def test_engine_lstm_matches_oracle(A, E, n, lives):
    """(A = 18: the LSTM head on h through the wide head_row at W = 256 and the wide categorical
    select_with, rows of stride zs = 20 through k_head_bwd and the head GEMM.)"""
    check_lstm_sync_vs_oracle(A, E, n, lives, learning_rate=2e-3)


def check_lstm_sync_vs_oracle(A, E, n, lives, iters=4, on_update=None, start=None, seed=None, **kw):
    """The synchronous LSTM engine against the oracle, every iteration; the hyperparameters in kw
    reach both.  on_update(it, eng, ref, lr): called after every checked update.
    start(eng, ref): called once before the first rollout."""
    eng, ref, ns = build(A, E, n, lives, seed=300 + E if seed is None else seed, **kw)
    counts = EpisodeCount()
    if start is not None:
        start(eng, ref)
        torch.cuda.synchronize()
    for it in range(iters):
        Pk = unflat(eng, ns, eng.params)
        eng.rollout_grad()
        torch.cuda.synchronize()
        acts = eng.actions.cpu().numpy()
        h0 = ref.hc[0].copy()
        # the rollout's carry-in state = the oracle's carry (computed on its own fp64 forward)
        np.testing.assert_allclose(eng.lstm_hp.cpu().numpy()[0], h0, rtol=1e-4, atol=2e-5)
        out = ref.iterate(forced_actions=acts)
        counts.add(out)
        assert_draws_explained(acts, out, 'a3c', A, it, z_eng=eng.z.cpu().numpy()[:n])
        assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards'])
        terms = eng.terminals.cpu().numpy()
        assert np.array_equal(terms, out['terminals'])
        # per-step policy/value outputs of the recurrent forward
        z = eng.z.cpu().numpy()[:n, :, :A + 1]
        np.testing.assert_allclose(z, out['z'][:, :, :A + 1], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(eng.lstm_h.cpu().numpy(), out['lstm']['H'], rtol=1e-4, atol=2e-5)
        # the saved trunk activations and LSTM sequence vs the independent fp64 batch forward
        assert_saved_acts(eng.slot(0), out, n, E, ('saved', it))
        tgt = eng.returns.cpu().numpy()
        np.testing.assert_allclose(tgt, out['target'], rtol=1e-4, atol=2e-5)
        planes = np.concatenate([np.transpose(ref.states(ref.tau + t), (0, 3, 1, 2)) for t in range(n)])
        losses, g_same = same_act_grads(eng.slot(0), planes, Pk, A, n, E, tgt, terms, ref.h['beta'],
                                        ref.h['literal_adv'])
        loss = eng.loss.cpu().numpy()
        for i, key in enumerate(('policy', 'value', 'entropy', 'total')):
            assert abs(loss[i] - losses[key]) <= 1e-4 * max(1.0, abs(losses[key])), (it, key, loss[i], losses[key])
            assert abs(loss[i] - out['losses'][key]) <= 1e-4 * max(1.0, abs(out['losses'][key])), (it, key)
        G = unflat(eng, ns, eng.grads)
        for name, _ in ns:
            assert rel_l2(G[name], g_same[name]) < 1e-4, (it, name, rel_l2(G[name], g_same[name]))
            assert rel_l2(G[name], out['grads'][name]) < 2e-2, (it, name)
        eng.apply()
        lr = ref.apply({k: Rc.clip_by_norm(v, ref.h['clip_norm']) for k, v in g_same.items()})
        torch.cuda.synchronize()
        P = unflat(eng, ns, eng.params)
        for name, _ in ns:
            d = np.abs(P[name] - ref.params[name]).max()
            assert d <= 1e-5 * max(1.0, np.abs(ref.params[name]).max()), (it, name, d)
        assert_env_state(eng, ref, it)
        if on_update is not None:
            on_update(it, eng, ref, lr)
    ref.episode_counts = counts.report(f'lstm sync A={A} E={E} n={n}')
    return eng, ref


def test_engine_lstm_overlap_zero_lr_equals_sync():
    """The pipelined engine carries the LSTM state across its two slots exactly as the synchronous
    one does: with lr 0 its rollouts reproduce sync's one call later."""
    s, _, _ = build(6, 16, 5, 3, seed=41, learning_rate=0.0)
    o, _, _ = build(6, 16, 5, 3, seed=41, learning_rate=0.0, overlap=True)
    o.iterate()
    for k in range(1, 5):
        s.iterate()
        o.iterate()
        torch.cuda.synchronize()
        prev = o.slot((k - 1) & 1)
        assert torch.equal(prev['actions'], s.actions), k
        assert torch.equal(prev['terminals'], s.terminals), k
        torch.testing.assert_close(prev['lstm_h'], s.lstm_h, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(o.loss, s.loss, rtol=1e-5, atol=1e-5)
        assert rel_l2(o.grads.cpu().numpy(), s.grads.cpu().numpy()) < 1e-5, k


def test_engine_lstm_bench_shape_runs():
    """BASELINE config 5 per GPU (SpaceInvaders, 256 envs, n=5, LSTM head): runs, finite, graph
    replay equals eager."""
    a, _, _ = build(6, 256, 5, 3, seed=5, frames=256, scale=1.0, overlap=True, use_graph=True)
    b, _, _ = build(6, 256, 5, 3, seed=5, frames=256, scale=1.0, overlap=True, use_graph=False)
    for _ in range(3):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    assert torch.isfinite(a.params).all() and torch.isfinite(a.loss).all()
    assert torch.equal(a.params, b.params)


@pytest.mark.parametrize('E', [40, 256])
def test_engine_lstm_fc_fold_forms_identical(E, monkeypatch):
    """C5's fc fold in either place -- by every cell workgroup (k_lstm_fwd) or once per fc tile by
    the tile's last K-slice workgroup (k_fc_part_fold, an in-launch hand-off through sc1 stores and
    an agent-scope ticket) -- sums the same partials in the same order: bit-identical rollouts and
    updates, overlapped with the backward (uneven load), E = 40 a ragged last tile of both kernels."""
    runs = {}
    for fold in ('0', '1'):
        monkeypatch.setenv('A3C_LSTM_FCFOLD', fold)
        runs[fold], _, _ = build(6, E, 5, 3, seed=77, frames=256, scale=2.0, learning_rate=2e-3, overlap=True,
                                 use_graph=True)
    a, b = runs['0'], runs['1']
    for k in range(6):
        a.iterate()
        b.iterate()
        torch.cuda.synchronize()
        sa, sb = a.slot(k & 1), b.slot(k & 1)
        for key in ('actions', 'z', 'lstm_h', 'lstm_c', 'lstm_gates', 'act_l3'):
            if key in sa:
                assert torch.equal(sa[key], sb[key]), (k, key)
        assert torch.equal(a.loss, b.loss), k
        assert torch.equal(a.params, b.params), k


def test_lstm_rejected_where_unsupported():
    from src import _lib
    from src.kernels import Net  # noqa: F401
    desc = _lib.net_desc(6, 'q', lstm=True)
    with pytest.raises(RuntimeError):
        _lib.param_layout(desc)


@pytest.mark.parametrize('E,frames', [(16, 48), (256, 512)])
def test_engine_lstm_overlap_matches_oracle(E, frames):
    """The pipelined C5 engine (bench.py --lstm: rollout k on the parameters after update k-2) against
    the oracle replayed in that order with the engine's own actions: per-step outputs, returns,
    losses, gradients on the engine's own saved activations and LSTM sequence, and parameters.  The
    fc arrives at the cell as K-slice partials folded by k_lstm_fwd (act_l3 written there).
    After iterate() k, slot k-1 (the buffers the backward just consumed) is held against the oracle's
    independent fp64 forward of rollout k-1: trunk activations, lstm_h / lstm_c / lstm_gates, losses
    and gradients (2e-2, the bound of the synchronous test)."""
    check_lstm_overlap_vs_oracle(6, E, 5, 3, rollouts=4, seed=60 + E, frames=frames, scale=2.0, learning_rate=2e-3)


def check_lstm_overlap_vs_oracle(A, E, n, lives, rollouts=4, seed=76, start=None, **kw):
    """The pipelined LSTM engine against the oracle (see test_engine_lstm_overlap_matches_oracle).
    start(eng, ref): called once before the first rollout, on the idle engine."""
    from _engine_parity import rollout_planes
    eng, ref, ns = build(A, E, n, lives, seed=seed, overlap=True, **kw)
    hist = []
    worst = {}
    counts = EpisodeCount()
    names = [name for name, _ in ns]
    if start is not None:
        start(eng, ref)
        torch.cuda.synchronize()
    for k in range(rollouts):
        eng.iterate()
        torch.cuda.synchronize()
        sl = eng.slot(k & 1)
        Pk = {kk: v.copy() for kk, v in ref.params.items()}
        out = ref.iterate(forced_actions=sl['actions'].cpu().numpy())
        planes = rollout_planes(ref, n)
        ref.tau += n
        counts.add(out)
        assert np.array_equal(sl['rewards'].cpu().numpy(), out['rewards']), k
        assert np.array_equal(sl['terminals'].cpu().numpy(), out['terminals']), k
        assert_env_state(eng, ref, k, tau=ref.tau)
        assert_draws_explained(sl['actions'].cpu().numpy(), out, 'a3c', A, k,
                               z_eng=sl['z'].cpu().numpy()[:n].reshape(n, E, -1))
        z = sl['z'].cpu().numpy()[:n].reshape(n, E, -1)[:, :, :A + 1]
        np.testing.assert_allclose(z, out['z'][:, :, :A + 1], rtol=1e-4, atol=2e-5)
        hist.append((Pk, planes, out))
        if k == 0:
            continue
        Pp, planes_p, out_p = hist[k - 1]
        slp = eng.slot((k - 1) & 1)
        tgt = slp['returns'].cpu().numpy()
        np.testing.assert_allclose(tgt, out_p['target'], rtol=1e-4, atol=2e-5)
        terms = slp['terminals'].cpu().numpy()
        np.testing.assert_allclose(slp['lstm_h'].cpu().numpy(), out_p['lstm']['H'], rtol=1e-4, atol=2e-5)
        assert_saved_acts(slp, out_p, n, E, ('saved', k))
        losses, g_same = same_act_grads(slp, planes_p, Pp, A, n, E, tgt, terms)
        loss = eng.loss.cpu().numpy()
        for i, key in enumerate(('policy', 'value', 'entropy', 'total')):
            assert abs(loss[i] - losses[key]) <= 1e-4 * max(1.0, abs(losses[key])), (k, key, loss[i], losses[key])
            # independent: the oracle's own fp64 lstm_a3c_forward of rollout k-1 and its targets
            ind = out_p['losses'][key]
            assert abs(loss[i] - ind) <= 1e-4 * max(1.0, abs(ind)), ('independent', k, key, loss[i], ind)
        G = unflat(eng, ns, eng.grads)
        for name, _ in ns:
            assert rel_l2(G[name], g_same[name]) < 1e-4, (k, name, rel_l2(G[name], g_same[name]))
        assert_independent_grads(G, out_p['grads'], names, k, worst)
        ref.apply({kk: Rc.clip_by_norm(v, ref.h['clip_norm']) for kk, v in g_same.items()}, advance_tau=False,
                  tau=out_p['tau'])
        P = unflat(eng, ns, eng.params)
        for name, _ in ns:
            d = np.abs(P[name] - ref.params[name]).max()
            assert d <= 1e-5 * max(1.0, np.abs(ref.params[name]).max()), (k, name, d)
    report_independent(f'lstm overlap E={E}', worst)
    ref.episode_counts = counts.report(f'lstm overlap A={A} E={E} n={n}', backprop=rollouts - 1)
    return eng, ref
