"""GAE(lambda) on the GPU: the stand-alone op a3c_gae_returns (k_gae) and the fused lambda-return of
the head backward (k_head_bwd<W, GAE>, both widths) through the engine, against the numpy fp64
reference gae_ref of tests/test_gae_cpu.py.

Bars (the project's existing ones): returns / advantages |x - ref| <= 1e-5 max(1, |ref|); losses
1e-4 max(1, |loss|); gradients 1e-4 relative-L2 against the oracle backward on the engine's own
saved activations."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import ref_cpu as Rc  # noqa: E402
from _engine_parity import assert_losses, build, rel_l2, rollout_planes, same_act_grads, unflat  # noqa: E402
from test_gae_cpu import gae_ref  # noqa: E402

GAMMA = 0.99


def assert_returns(got, ref, tag):
    """the existing bar for returns: 1e-5 of max(1, |ref|), element-wise"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - 1e-5 * np.maximum(1.0, np.abs(ref))
    assert (err <= 0).all(), (tag, float(np.abs(got - ref).max()), np.argwhere(err > 0)[:4].tolist())


# ------------------------------------------------------------------ the stand-alone op
def forced_terminals(n, E, rng):
    """Random terminals plus, by env (e % 4; every pattern on every env when E < 4): t = 0, an
    interior step, t = n-1, two steps in a row."""
    terms = (rng.random((n, E)) < 0.1).astype(np.uint8)
    mid = n // 2
    for e in range(E):
        pats = range(4) if E < 4 else (e % 4,)
        for p in pats:
            if p == 0:
                terms[0, e] = 1
            elif p == 1:
                terms[mid, e] = 1
            elif p == 2:
                terms[n - 1, e] = 1
            else:
                terms[mid, e] = 1
                terms[min(mid + 1, n - 1), e] = 1
    return terms


def op_data(n, E, seed, normal_rewards=False):
    rng = np.random.default_rng(seed)
    if normal_rewards:
        rewards = rng.standard_normal((n, E)).astype(np.float32)
    else:   # the engine's clipped rewards, life-loss penalty included
        rewards = rng.choice(np.array([-2, -1, 0, 0, 0, 1], np.float32), (n, E))
    return rewards, forced_terminals(n, E, rng), rng.standard_normal((n, E)).astype(np.float32), \
        rng.standard_normal(E).astype(np.float32)


def strided_values(values, stride, col):
    """values [n, E] as column `col` of a row-major [n, E, stride] device buffer filled with NaN"""
    buf = torch.full(values.shape + (stride,), float('nan'), dtype=torch.float32, device='cuda')
    buf[..., col] = torch.as_tensor(values).cuda()
    return buf[..., col]


@pytest.mark.parametrize('E', [1, 37, 300])
@pytest.mark.parametrize('n', [1, 2, 5, 64])
def test_gae_op_matches_reference(n, E):
    """E = 37: a partial block; E = 300: past the 256-thread block boundary."""
    from src.kernels import gae_returns
    rewards, terms, values, boot = op_data(n, E, 100 * n + E)
    if n >= 5:
        assert terms[0].any() and terms[n - 1].any() and terms[1:n - 1].any()
        assert (terms[:-1] & terms[1:]).any()
    cu = lambda a: torch.as_tensor(a).cuda()   # noqa: E731
    r_d, t_d, b_d = cu(rewards), cu(terms), cu(boot)
    for stride, col in ((1, 0), (8, 6), (12, 7)):
        v_d = strided_values(values, stride, col)
        if n > 1 and E > 1:
            assert v_d.stride() == (E * stride, stride)
        for lam in (0.0, 0.5, 0.95, 1.0):
            G, adv = gae_returns(r_d, t_d, v_d, b_d, GAMMA, lam)
            G_only = gae_returns(r_d, t_d, v_d, b_d, GAMMA, lam, with_adv=False)   # adv nullable
            torch.cuda.synchronize()
            G_ref, A_ref = gae_ref(rewards, terms, values, boot, GAMMA, lam)
            assert_returns(G.cpu().numpy(), G_ref, ('G', n, E, stride, lam))
            assert_returns(adv.cpu().numpy(), A_ref, ('adv', n, E, stride, lam))
            assert torch.equal(G, G_only)


@pytest.mark.parametrize('n,E', [(1, 37), (5, 300), (64, 37)])
def test_gae_op_lambda_one_is_a3c_returns(n, E):
    """lambda = 1 against a3c_returns: within 1 ulp of float, not bit for bit.  k_returns rounds
    r_i + gamma R_{i+1} to float; k_gae carries A_i = R_i - V_i in float64 and rounds A_i + V_i,
    whose float64 value differs from R_i in its last bits (V_i is subtracted and added back), so the
    two casts to float can land on neighbouring values."""
    from src.kernels import gae_returns, returns
    rewards, terms, values, boot = op_data(n, E, 7 * n + E, normal_rewards=True)
    cu = lambda a: torch.as_tensor(a).cuda()   # noqa: E731
    R = returns(cu(rewards), cu(terms), cu(boot), GAMMA)
    G, adv = gae_returns(cu(rewards), cu(terms), strided_values(values, 8, 6), cu(boot), GAMMA, 1.0)
    torch.cuda.synchronize()
    R, G, adv = R.cpu().numpy(), G.cpu().numpy(), adv.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(R), np.abs(G)))
    print('lambda=1 vs a3c_returns: max |G - R| / ulp =', float((np.abs(G - R) / ulp).max()),
          'differing', int((G != R).sum()), 'of', G.size)
    assert (np.abs(G - R) <= ulp).all()
    # and the advantage is the n-step one: adv + V = R at the returns bar
    assert_returns(adv.astype(np.float64) + values, R, ('adv + V', n, E))


def test_gae_op_rejects_invalid_arguments():
    from src import _lib
    n, E = 3, 5
    r = torch.zeros((n, E), device='cuda')
    t = torch.zeros((n, E), dtype=torch.uint8, device='cuda')
    b = torch.zeros(E, device='cuda')
    out = torch.zeros((n, E), device='cuda')
    p, s = _lib.ptr, _lib.stream_handle()

    def call(rewards=r, terms=t, values=r, stride=1, boot=b, n=n, lam=0.9, R=out):
        return _lib.lib().a3c_gae_returns(p(rewards), p(terms), p(values), stride, p(boot), n, E, GAMMA, lam, p(R),
                                          p(None), s)
    assert call() == 0
    for bad in (dict(lam=-0.01), dict(lam=1.01), dict(lam=float('nan')), dict(n=0), dict(n=-1), dict(stride=0),
                dict(rewards=None), dict(terms=None), dict(values=None), dict(boot=None), dict(R=None)):
        assert call(**bad) == _lib.ERR_INVALID, bad
    assert b'a3c_gae_returns' in _lib.lib().a3c_last_error()
    torch.cuda.synchronize()
    with pytest.raises(_lib.A3CError):
        from src.kernels import gae_returns
        gae_returns(r, t, r, b, GAMMA, 1.5)


# ------------------------------------------------------------------ engine, lambda = 1
@pytest.mark.parametrize('E,n,overlap', [(8, 3, False), (16, 5, True)])
def test_engine_lambda_one_is_the_default_engine(E, n, overlap):
    """gae_lambda = 1 selects the kernels without GAE: bit-identical to an engine that never
    heard of the option."""
    a, _, _ = build('a3c', 6, E, n, 5, seed=1037, overlap=overlap, gae_lambda=1.0)
    b, _, _ = build('a3c', 6, E, n, 5, seed=1037, overlap=overlap)
    assert a.cfg.gae_lambda == 1.0 and b.cfg.gae_lambda == 1.0
    for _ in range(3):
        a.iterate()
        b.iterate()
    torch.cuda.synchronize()
    for name in ('params', 'loss', 'returns', 'grads', 'ms'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    if overlap:
        assert torch.equal(a.slot(1)['returns'], b.slot(1)['returns'])


# ------------------------------------------------------------------ engine, lambda = 0.9
LAM = 0.9


def build_lstm(A, E, n, lives, seed, frames=48, scale=4.0, **kw):
    from src.engine import Engine
    from src.initializers import flatten_host, init_params
    from src.kernels import param_names_shapes
    eng = Engine(num_envs=E, n_step=n, action_size=A, algo='a3c', start_lives=lives, num_frames=frames, seed=seed,
                 lstm=True, **kw)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=seed, stddev=0.02 * scale)))
    return eng, None, ns


def raw_gradient(eng, ns):
    """The un-clipped gradient of the last backward, per tensor, from the gradient buffer and
    sumsq (the squared norms of the raw gradient): a buffer already clipped to norm 40 is scaled
    back by sqrt(sumsq) / 40; a single-GPU engine clips inside the apply and leaves the buffer raw."""
    G = unflat(eng, ns, eng.grads)
    ss = eng.sumsq.cpu().numpy().astype(np.float64)
    for i, (name, _) in enumerate(ns):
        have = float(np.sum(G[name].astype(np.float64) ** 2))
        if not np.isclose(have, ss[i], rtol=1e-5):
            assert ss[i] > 40.0 ** 2 and np.isclose(have, 40.0 ** 2, rtol=1e-5), (name, have, ss[i])
            G[name] = (G[name].astype(np.float64) * (np.sqrt(ss[i]) / 40.0)).astype(np.float32)
    return G


def check_rollout(slot, loss, A, n, E, tag):
    """returns and loss of one back-propagated rollout against gae_ref on the slot's own rewards,
    terminals and V rows (z[:n, :, A], bootstrap z[n, :, A]); returns (terminals, G_ref)."""
    rewards = slot['rewards'].cpu().numpy()
    terms = slot['terminals'].cpu().numpy()
    z = slot['z'].cpu().numpy()
    acts = slot['actions'].cpu().numpy().reshape(-1)
    assert z.shape[0] == n + 1 and np.isfinite(z[..., :A + 1]).all()
    G_ref, _ = gae_ref(rewards, terms, z[:n, :, A], z[n, :, A], GAMMA, LAM)
    assert_returns(slot['returns'].cpu().numpy(), G_ref, ('returns', tag))
    # GAE is not the n-step return here: the check cannot pass on the lambda = 1 path
    R1 = Rc.nstep_returns(rewards, terms, z[n, :, A], GAMMA)
    assert np.abs(G_ref - R1).max() > 1e-3, tag
    G32 = G_ref.astype(np.float32)
    losses, _ = Rc.a3c_loss_and_dz(z[:n].reshape(n * E, -1)[:, :A + 1].astype(np.float64), acts,
                                   G32.reshape(-1).astype(np.float64), 0.01)
    assert_losses(loss, losses, 'a3c', ('loss', tag))
    return terms, G32


CASES = {
    # name: (A, E, n, seed, overlap, lstm, engine options, gradient check on the first iteration)
    'nips-sync': (6, 8, 3, 1150, False, False, {}, True),
    'nips-overlap': (6, 16, 5, 1003, True, False, {}, False),
    'wide-A18': (18, 8, 3, 1037, False, False, {}, False),
    'lstm-sync': (6, 8, 4, 1037, False, True, dict(learning_rate=2e-3), False),
    'nature-sync': (6, 8, 3, 1150, False, False, dict(dqn_type='nature', scale=2.0, learning_rate=2e-3), True),
}


@pytest.mark.parametrize('case', list(CASES))
def test_engine_gae_matches_reference(case):
    """Engine(gae_lambda=0.9): after every iterate() the returns buffer is the lambda-return of the
    slot's own rollout and the loss is the A3C loss at that target.  lives = 5, 48 frames and the
    seeds are chosen (by stepping the CPU env, whose terminals depend on neither actions nor
    parameters) so that the three checked rollouts of every case hold a terminal before the last
    step and one at the last step; seed 1150 has both in its first rollout, the one whose gradient
    is compared (engine and oracle still share parameters there, so the oracle's replay of the
    engine's actions gives the engine's states)."""
    A, E, n, seed, overlap, lstm, opts, grads = CASES[case]
    opts = dict(opts)
    mk = build_lstm if lstm else build
    kw = dict(overlap=True) if overlap else {}
    if lstm:
        eng, ref, ns = mk(A, E, n, 5, seed, gae_lambda=LAM, **kw, **opts)
    else:
        eng, ref, ns = mk('a3c', A, E, n, 5, seed=seed, gae_lambda=LAM, **kw, **opts)
    assert abs(eng.cfg.gae_lambda - LAM) < 1e-7
    assert eng.zs == (20 if A == 18 else 8)
    early = late = 0
    for k in range(4 if overlap else 3):
        Pk = unflat(eng, ns, eng.params) if grads and k == 0 else None
        eng.iterate()
        torch.cuda.synchronize()
        if overlap and k == 0:
            continue                              # the pipeline is filling: no backward yet
        slot = eng.slot((k - 1) & 1) if overlap else eng.slot(0)
        terms, G32 = check_rollout(slot, eng.loss.cpu().numpy(), A, n, E, (case, k))
        early += int(terms[:n - 1].sum())
        late += int(terms[n - 1].sum())
        if Pk is not None:
            acts = eng.actions.cpu().numpy()
            out = ref.iterate(forced_actions=acts, grads=False)
            assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards'])
            assert np.array_equal(terms, out['terminals'])
            planes = rollout_planes(ref, n)
            _, g_same = same_act_grads(eng, planes, Pk, 'a3c', A, n, E, G32)
            G = raw_gradient(eng, ns)
            for name, _ in ns:
                r = rel_l2(G[name], g_same[name])
                assert r < 1e-4, (case, name, r)
    assert early >= 1 and late >= 1, (case, early, late)


def test_engine_gae_rejections():
    from src import _lib
    from src.engine import Engine
    for kw in (dict(algo='q', gae_lambda=0.9), dict(gae_lambda=0.9, literal_adv=1), dict(gae_lambda=-0.1),
               dict(gae_lambda=1.5)):
        with pytest.raises(_lib.A3CError, match='gae_lambda') as ei:
            Engine(num_envs=4, n_step=2, num_frames=8, **kw)
        assert ei.value.rc == _lib.ERR_INVALID
    Engine(num_envs=4, n_step=2, num_frames=8, gae_lambda=0.0).close()      # the ends of [0, 1] are valid
    Engine(num_envs=4, n_step=2, num_frames=8, algo='q', gae_lambda=1.0).close()
