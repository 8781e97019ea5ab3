"""Every hyperparameter off the reference's default, from the kernels to the engine.

The rest of the suite runs gamma = discount = 0.99, beta = 0.01, decay = 0.99, momentum = 0,
epsilon = 0.1, clip_norm = 40, max_step = 8e7 and random_start = 30; a kernel that kept one of them
as a literal, ignored momentum, indexed the per-tensor clip multiplier wrongly, or read cfg.gamma
where cfg.discount belongs would pass it.  Here each value moves:

  1. kernels: returns / TD targets / GAE at gamma in {0, 0.5, 0.9, 1}; loss + backward at beta in
     {0, 0.1}; clip + RMSProp through the C ABI on a hand-made tensor table (sizes around the
     4096-element partial chunk, more than 64 partials in one tensor, a zero-size tensor,
     A3C_MAX_TENSORS tensors) with the clip regimes mixed in one table, and the promise of
     csrc/optim.hip's header -- element math bit for bit the numpy oracle's;
  2. engine: the parity checks of tests/_engine_parity.py with the set OFF below, in which gamma
     and discount differ, and a clip_norm picked per case from the oracle's first gradient so that
     some tensors are clipped and some are not;
  3. the learning-rate schedule where it is visible (max_step = 40: an eighth of lr0 per
     rollout), at late and large steps, and the target sync at its boundary;
  4. main.py's flags reaching a3c_engine_config.

Bounds are those of the tests whose helpers run here; none is widened."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import ref_cpu as R  # noqa: E402
from oracle.engine_ref import EngineRef  # noqa: E402
from _engine_parity import check_hogwild1_vs_oracle, check_overlap_vs_oracle, check_sync_vs_oracle  # noqa: E402
from _net_parity import check_loss_backward, cu  # noqa: E402
from test_gae_cpu import gae_ref  # noqa: E402


@pytest.fixture(scope='module')
def K():
    from src import _lib
    _lib.require_device()
    from src import kernels
    return kernels


# =================================================================== 1. kernels
GAMMAS = (0.0, 0.5, 0.9, 1.0)


def rollout_data(n, E, seed):
    """Clipped rewards, a bootstrap value and terminals at rate 0.2 with one column all terminal and
    one with none (E = 1: one variant each).  Returns (rewards, boot, [terminals, ...])."""
    rng = np.random.default_rng(seed)
    rew = rng.choice(np.array([-1, 0, 0, 0, 1], np.float32), (n, E))
    boot = rng.standard_normal(E).astype(np.float32)
    term = (rng.random((n, E)) < 0.2).astype(np.uint8)
    if E == 1:
        return rew, boot, [np.ones((n, 1), np.uint8), np.zeros((n, 1), np.uint8), term]
    term[:, 0] = 1
    term[:, 1] = 0
    return rew, boot, [term]


@pytest.mark.parametrize('E', [1, 67, 300])
@pytest.mark.parametrize('n', [1, 5])
def test_returns_bit_exact_at_every_gamma(K, n, E):
    """a3c_returns against ref_cpu.nstep_returns, bit for bit as at gamma = 0.99
    (test_returns_and_td_target_bit_exact).  gamma = 0 leaves the rewards, gamma = 1 their plain
    sums: a literal 0.99 in the kernel differs from both at the first step."""
    rew, boot, terms = rollout_data(n, E, 40 + 10 * n + E)
    for term in terms:
        for gamma in GAMMAS:
            got = K.returns(cu(rew), cu(term), cu(boot), gamma).cpu().numpy()
            ref = R.nstep_returns(rew, term, boot, gamma).astype(np.float32)
            assert np.array_equal(got, ref), (gamma, int(term.sum()))
        if not term.all():      # the data can tell two gammas apart
            assert not np.array_equal(R.nstep_returns(rew, term, boot, 0.5), R.nstep_returns(rew, term, boot, 0.9))


@pytest.mark.parametrize('A', [4, 6, 18])
@pytest.mark.parametrize('E', [1, 67, 300])
@pytest.mark.parametrize('n', [1, 5])
def test_td_target_bit_exact_at_every_discount(K, n, E, A):
    """a3c_td_target against ref_cpu.td_target, bit for bit; q rows of the head stride zs."""
    rew, _, terms = rollout_data(n, E, 50 + 10 * n + E + A)
    rng = np.random.default_rng(n + E + A)
    zs = (A + 3) // 4 * 4
    qn = np.full((n * E, zs), 1e30, np.float32)         # (a column read past A would win the max)
    qn[:, :A] = rng.standard_normal((n * E, A)).astype(np.float32)
    for term in terms:
        for discount in GAMMAS:
            got = K.td_target(cu(rew.reshape(-1)), cu(term.reshape(-1)), cu(qn), A, discount).cpu().numpy()
            ref = R.td_target(rew.reshape(-1), term.reshape(-1), qn[:, :A], discount).astype(np.float32)
            assert np.array_equal(got, ref), (discount, int(term.sum()))


@pytest.mark.parametrize('E', [1, 67, 300])
@pytest.mark.parametrize('n', [1, 5])
def test_gae_at_every_gamma_and_lambda(K, n, E):
    """a3c_gae_returns against gae_ref (tests/test_gae_cpu.py) at test_gpu_gae.py's bar: 1e-5 of
    max(1, |ref|), element-wise, returns and advantages."""
    rew, boot, terms = rollout_data(n, E, 60 + 10 * n + E)
    values = np.random.default_rng(n * E).standard_normal((n, E)).astype(np.float32)
    for term in terms:
        for gamma in GAMMAS:
            for lam in (0.0, 0.5, 1.0):
                G, adv = K.gae_returns(cu(rew), cu(term), cu(values), cu(boot), gamma, lam)
                G_ref, A_ref = gae_ref(rew, term, values, boot, gamma, lam)
                for got, ref, what in ((G, G_ref, 'G'), (adv, A_ref, 'adv')):
                    got, ref = got.cpu().numpy().astype(np.float64), np.asarray(ref, np.float64)
                    err = np.abs(got - ref) - 1e-5 * np.maximum(1.0, np.abs(ref))
                    assert (err <= 0).all(), (what, gamma, lam, float(np.abs(got - ref).max()))


@pytest.mark.parametrize('beta', [0.0, 0.1])
@pytest.mark.parametrize('B,literal', [(7, False), (13, True), (7, True), (13, False)])
def test_loss_backward_off_default_beta(K, B, literal, beta):
    """Net.loss_backward at the batch sizes of test_loss_backward_matches_oracle, both literal_adv
    settings: beta = 0 removes the entropy term, beta = 0.1 is ten times the default's."""
    check_loss_backward(K, 'a3c', 4 if B == 13 else 6, B, literal, beta=beta)


@pytest.mark.parametrize('beta', [0.0, 0.1])
@pytest.mark.parametrize('A,B,literal', [(7, 3, False), (8, 1, True)])
def test_nature_loss_backward_off_default_beta(K, A, B, literal, beta):
    """NatureNet.loss_backward likewise (the LSTM head's kernels take no beta: its loss runs in the
    feed-forward head backward, covered above and by the engine case below)."""
    from test_gpu_action_width import check_nature_forward_loss_backward
    check_nature_forward_loss_backward(K, A, B, literal, beta=beta)


# ------------------------------------------------------------------- clip + RMSProp, C ABI
HYPER = (dict(decay=0.9, momentum=0.5, epsilon=1e-2, lr=3e-3), dict(decay=0.5, momentum=0.9, epsilon=1e-6, lr=1e-2))
CLIP = 2.5              # (its square is a float: the tensor of norm exactly CLIP is exact in fp32)
CHUNK = 4096            # SS_CHUNK of csrc/optim.h: elements per sum-of-squares partial
TAIL = 64               # sentinel floats after each buffer
SENTINEL = 12345.0

# (size, gradient norm / clip); None: all zero; 'exact': one element equal to clip, the rest 0.
# 65 * CHUNK + 1 elements are 66 partials: the second trip of k_apply's 64-lane fold loop.
TABLE = ((1, 3.0), (3, 0.3), (4, 2.2), (5, 'exact'), (0, None), (CHUNK - 1, 2.5), (CHUNK, 0.3), (CHUNK + 1, 4.0),
         (2 * CHUNK + 1, 0.45), (65 * CHUNK + 1, 2.0), (7, None), (6, 0.5))


def make_table(sizes, gaps):
    """4-aligned ascending offsets; gaps[i] extra floats (a multiple of 4) between tensor i and the
    next.  A zero-size tensor shares its offset with its successor.  The flat vector ends with the
    last tensor, padded to a multiple of 4: that is the length the C ABI derives from the table.
    Returns (offsets, padded total)."""
    assert gaps[-1] == 0
    offs, end = [], 0
    for s, g in zip(sizes, gaps):
        offs.append(end)
        end = (end + s + 3) // 4 * 4 + g
    return offs, end


def table_grads(rng, sizes, offs, total, regimes):
    """A flat fp32 gradient (zero in the gaps and the padding) whose per-tensor norms stand in the
    given ratios to CLIP."""
    g = np.zeros(total, np.float32)
    for s, o, r in zip(sizes, offs, regimes):
        if s == 0 or r is None:
            continue
        if r == 'exact':
            g[o + s // 2] = CLIP
            continue
        v = rng.standard_normal(s)
        g[o:o + s] = (v * (r * CLIP / np.linalg.norm(v))).astype(np.float32)
    return g


def assert_regimes_mixed(g, sizes, offs):
    """From the fp64 norms of the fp32 gradient: the table holds tensors at least 2x over CLIP, at
    most 0.5x under, an all-zero one and one at CLIP exactly in fp32."""
    norms = np.array([np.sqrt(np.sum(g[o:o + s].astype(np.float64) ** 2)) for s, o in zip(sizes, offs)])
    live = np.array(sizes) > 0
    assert (norms[live] >= 2 * CLIP).sum() >= 2 and ((norms[live] <= 0.5 * CLIP) & (norms[live] > 0)).sum() >= 2
    assert (norms[live] == 0).any() and (norms[live] == CLIP).any()
    assert float(np.sqrt(np.float32(CLIP * CLIP))) == CLIP


def dev_buf(host):
    """host [total] on the device, followed by TAIL sentinels the kernels must leave alone."""
    b = torch.full((host.size + TAIL,), SENTINEL, dtype=torch.float32, device='cuda')
    b[:host.size] = torch.as_tensor(host)
    return b


def assert_tail(*bufs):
    for b in bufs:
        assert (b[-TAIL:] == SENTINEL).all()


def i64(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*[int(v) for v in vals])


def opt_workspace(blocks=None):
    from src import _lib
    nb = _lib.c_i64()
    _lib.check(_lib.lib().a3c_optim_workspace_bytes(0, ctypes.byref(nb)), 'a3c_optim_workspace_bytes')
    return torch.zeros(int(nb.value) if blocks is None else 8 * blocks, dtype=torch.uint8, device='cuda')


def oracle_step(w, ms, mom, g, sizes, offs, clip, hp):
    """R.clip_by_norm per tensor, then R.rmsprop_apply -- over the whole flat vector: the gaps and
    the padding carry zero gradients, so there ms decays and w moves by the carried momentum only,
    which is what the element rule gives for them.  In place; returns the fp64 sums of squares."""
    gc = g.copy()
    ss = []
    for s, o in zip(sizes, offs):
        ss.append(np.sum(g[o:o + s].astype(np.float64) ** 2))
        if clip > 0 and s > 0:
            gc[o:o + s] = R.clip_by_norm(g[o:o + s], clip)
    R.rmsprop_apply(w, ms, mom, gc, hp['lr'], hp['decay'], hp['momentum'], hp['epsilon'])
    return np.array(ss)


def run_table(sizes, regimes, gaps, clip, hp, steps, seed):
    from src import _lib
    offs, total = make_table(sizes, gaps)
    assert total % 4 == 0 and all(o % 4 == 0 for o in offs)
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(total).astype(np.float32)
    ms = (0.5 + rng.random(total)).astype(np.float32)
    mom = (rng.standard_normal(total) * 1e-2).astype(np.float32)       # carried momentum from the start
    w_d, ms_d, mom_d = dev_buf(w), dev_buf(ms), dev_buf(mom)
    sumsq = torch.full((len(sizes) + 1,), SENTINEL, dtype=torch.float32, device='cuda')
    ws = opt_workspace()
    lib = _lib.lib()
    for step in range(steps):
        g = table_grads(rng, sizes, offs, total, regimes)
        if len(sizes) == len(TABLE):
            assert_regimes_mixed(g, sizes, offs)
        g_d = dev_buf(g)
        if step == 0:          # the clip-only entry on the same table (the Hogwild workers' clip)
            gc_d = g_d.clone()
            _lib.check(lib.a3c_clip_grads(_lib.ptr(gc_d), len(sizes), i64(offs), i64(sizes), clip, None,
                                          _lib.ptr(ws), _lib.stream_handle()), 'a3c_clip_grads')
            gc = gc_d.cpu().numpy()
            for s, o in zip(sizes, offs):
                want = R.clip_by_norm(g[o:o + s], clip) if clip > 0 and s else g[o:o + s]
                np.testing.assert_allclose(gc[o:o + s], want, rtol=1e-6, atol=1e-12)
            gap = np.ones(total, bool)
            for s, o in zip(sizes, offs):
                gap[o:o + s] = False
            assert not gc[:total][gap].any()
            assert_tail(gc_d)
        _lib.check(lib.a3c_clip_rmsprop_apply(_lib.ptr(w_d), _lib.ptr(ms_d), _lib.ptr(mom_d), _lib.ptr(g_d), len(sizes),
                                              i64(offs), i64(sizes), hp['lr'], hp['decay'], hp['momentum'],
                                              hp['epsilon'], clip, _lib.ptr(sumsq), _lib.ptr(ws),
                                              _lib.stream_handle()), 'a3c_clip_rmsprop_apply')
        ss = oracle_step(w, ms, mom, g, sizes, offs, clip, hp)
        np.testing.assert_allclose(w_d[:total].cpu().numpy(), w, rtol=1e-6, atol=1e-9, err_msg=f'w step {step}')
        np.testing.assert_allclose(ms_d[:total].cpu().numpy(), ms, rtol=1e-6, err_msg=f'ms step {step}')
        np.testing.assert_allclose(mom_d[:total].cpu().numpy(), mom, rtol=1e-5, atol=1e-12, err_msg=f'mom step {step}')
        got = sumsq.cpu().numpy()
        assert np.isclose(got[:len(sizes)], ss, rtol=1e-6, atol=0).all(), (step, got, ss)
        assert got[len(sizes)] == SENTINEL
        assert np.array_equal(g_d[:total].cpu().numpy(), g)             # the fused pass leaves the gradient
        assert_tail(w_d, ms_d, mom_d, g_d)


@pytest.mark.parametrize('clip', [CLIP, 0.0, -1.0])
@pytest.mark.parametrize('hp', HYPER, ids=['rho.9-mom.5', 'rho.5-mom.9'])
def test_clip_rmsprop_arbitrary_table(K, hp, clip):
    """a3c_clip_rmsprop_apply / a3c_clip_grads on a table that is no net's layout, five applies with
    fresh gradients so ms and the momentum carry, at test_clip_rmsprop_matches_oracle's bounds.
    clip <= 0: clipping is off."""
    sizes = [s for s, _ in TABLE]
    regimes = [r for _, r in TABLE]
    gaps = [0, 4, 0, 64, 0, 0, 8, 0, 4, 0, 4, 0]
    run_table(sizes, regimes, gaps, clip, hp, steps=5, seed=17)


def test_clip_rmsprop_max_tensors_of_one_element(K):
    """A3C_MAX_TENSORS one-element tensors: every slot of the clip-multiplier table in use, each with
    its own regime (a multiplier read from another slot changes its neighbour's step)."""
    from src import _lib
    n = _lib.MAX_TENSORS
    regimes = [(3.0, 0.1, None, 'exact', 2.0, 0.5, 7.0, 0.01)[i % 8] for i in range(n)]
    for hp in HYPER:
        run_table([1] * n, regimes, [0] * n, CLIP, hp, steps=3, seed=23)


def test_clip_rmsprop_rejects_bad_tables(K):
    """A3C_ERR_INVALID and nothing launched: every buffer as it was."""
    from src import _lib
    lib = _lib.lib()
    n_big = (1024 + 1) * CHUNK                       # SS_MAX_BLOCKS + 1 partial blocks
    host = np.arange(n_big, dtype=np.float32) % 7 - 3
    bufs = [dev_buf(host) for _ in range(4)]
    before = [b.clone() for b in bufs]
    ws = opt_workspace(blocks=2048)                  # (room for the partials of the last case all the same)
    many = _lib.MAX_TENSORS + 1
    cases = {'unaligned offset': (2, [0, 6], [4, 4]),
             'descending offsets': (2, [8, 0], [4, 4]),
             'overlapping tensors': (2, [0, 4], [8, 4]),
             'no tensor': (0, [0], [4]),
             'too many tensors': (many, [4 * i for i in range(many)], [1] * many),
             'too many partial blocks': (1, [0], [n_big])}
    for what, (n, offs, sizes) in cases.items():
        rc = lib.a3c_clip_rmsprop_apply(*[_lib.ptr(b) for b in bufs], n, i64(offs), i64(sizes), 1e-2, 0.9, 0.5, 1e-2,
                                        CLIP, None, _lib.ptr(ws), _lib.stream_handle())
        assert rc == _lib.ERR_INVALID, (what, rc)
        rc = lib.a3c_clip_grads(_lib.ptr(bufs[3]), n, i64(offs), i64(sizes), CLIP, None, _lib.ptr(ws),
                                _lib.stream_handle())
        assert rc == _lib.ERR_INVALID, (what, rc)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b, b0)


@pytest.mark.parametrize('hp', HYPER, ids=['rho.9-mom.5', 'rho.5-mom.9'])
def test_rmsprop_element_math_is_bit_exact(K, hp):
    """csrc/optim.hip: "Element math is written with contraction off so it matches the numpy oracle
    bit for bit on equal gradients" -- for the paths that do not clip: a3c_rmsprop_range with lr by
    value and through lr_dev, and a3c_clip_rmsprop_apply with clip <= 0.  Three steps on 4097
    elements (a scalar tail after the float4 body), fresh gradients of mixed magnitude."""
    from src import _lib
    lib = _lib.lib()
    n, total = CHUNK + 1, CHUNK + 4
    rng = np.random.default_rng(29)
    w = rng.standard_normal(total).astype(np.float32)
    ms = (0.5 + rng.random(total)).astype(np.float32)
    mom = (rng.standard_normal(total) * 1e-2).astype(np.float32)
    start = [v.copy() for v in (w, ms, mom)]
    paths = {k: [dev_buf(w), dev_buf(ms), dev_buf(mom)] for k in ('lr', 'lr_dev', 'apply')}
    lr_dev = cu(np.array([hp['lr'], 0.0], np.float32))
    ws = opt_workspace()
    st = _lib.stream_handle()
    for step in range(3):
        g = np.zeros(total, np.float32)
        g[:n] = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)).astype(np.float32)
        g_d = dev_buf(g)
        a, b, c = paths['lr'], paths['lr_dev'], paths['apply']
        _lib.check(lib.a3c_rmsprop_range(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(g_d), n, None,
                                         hp['lr'], hp['decay'], hp['momentum'], hp['epsilon'], st), 'a3c_rmsprop_range')
        _lib.check(lib.a3c_rmsprop_range(_lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(g_d), n,
                                         _lib.ptr(lr_dev), 123.0, hp['decay'], hp['momentum'], hp['epsilon'], st),
                   'a3c_rmsprop_range')
        _lib.check(lib.a3c_clip_rmsprop_apply(_lib.ptr(c[0]), _lib.ptr(c[1]), _lib.ptr(c[2]), _lib.ptr(g_d), 1,
                                              i64([0]), i64([n]), hp['lr'], hp['decay'], hp['momentum'],
                                              hp['epsilon'], 0.0, None, _lib.ptr(ws), st), 'a3c_clip_rmsprop_apply')
        R.rmsprop_apply(w, ms, mom, g, hp['lr'], hp['decay'], hp['momentum'], hp['epsilon'])
        for path, bufs in paths.items():
            # the range entry covers [0, n); the table entry its padding up to `total` as well
            m = total if path == 'apply' else n
            for name, dev, host in zip(('w', 'ms', 'mom'), bufs, (w, ms, mom)):
                got = dev[:m].cpu().numpy()
                diff = int((got != host[:m]).sum())
                assert np.array_equal(got, host[:m]), (path, name, step, diff, 'of', m)
            assert_tail(*bufs)
    for path in ('lr', 'lr_dev'):             # past its n elements the range entry wrote nothing
        for dev, host0 in zip(paths[path], start):
            assert np.array_equal(dev[n:total].cpu().numpy(), host0[n:])


# =================================================================== 2. engine parity off the defaults
# a learning rate that is a float: a3c_engine_config carries it as one, the oracle as a double
LR = float(np.float32(2e-3))
# gamma != discount: the a3c path and the q path cannot read each other's field.  max_step = 40
# makes the schedule visible (section 3): an eighth of lr0 per 5-step rollout.
OFF = dict(gamma=0.9, discount=0.8, beta=0.05, decay=0.9, momentum=0.5, epsilon=0.01, learning_rate=LR, max_step=40)


def pick_clip(algo, A, E, n, lives, seed, frames=48, scale=4.0, lstm=False, **kw):
    """A clip_norm between the smallest and the largest per-tensor norm of the oracle's own first
    gradient (their geometric mean), on the CPU: the first update clips some tensors and not
    others.  The case asserts that from the engine's numbers (Watch)."""
    from src.initializers import init_params
    from src.kernels import param_names_shapes
    ns = param_names_shapes(A, algo, lstm=lstm, dqn_type=kw.get('dqn_type', 'nips'))
    p = init_params(ns, seed=seed, stddev=0.02 * scale)
    ref = EngineRef(p, E, n, A, algo, lives, frames, seed, lstm=lstm, **kw)
    ref.reset()
    norms = np.sqrt(np.array([float(v) for v in ref.iterate()['sumsq'].values()], np.float64))
    assert norms.max() > 4 * norms.min() > 0
    return float(np.float32(np.sqrt(norms.min() * norms.max())))


class Watch:
    """on_update of the parity checks: after every update the schedule word sched[0] equals the
    float of the oracle's learning rate exactly, and the first update mixes clipped and unclipped
    tensors -- from the engine's own sums of squares (sumsq, compared to the fp64 sums by the
    check), or, where the engine clips its buffer in place and keeps no sums (hogwild, world > 1),
    from the clipped gradient: a clipped tensor's norm is clip_norm, an unclipped one's is less."""

    def __init__(self, clipped_buffer=False, clip_mix=True):
        self.clipped_buffer = clipped_buffer
        self.clip_mix = clip_mix
        self.updates = 0
        self.lrs = []

    def __call__(self, it, eng, ref, lr):
        from src.engine import _view
        sched = _view(eng.sched_ptr, (2,), torch.float32).cpu().numpy()
        assert sched[0] == np.float32(lr), (it, sched[0], lr)
        self.lrs.append(float(lr))
        self.updates += 1
        if self.updates > 1 or not self.clip_mix:
            return
        clip = float(ref.h['clip_norm'])
        if self.clipped_buffer:
            g = eng.grads.cpu().numpy().astype(np.float64)
            norms = np.array([np.linalg.norm(g[o:o + s]) for o, s in zip(eng.offsets, eng.sizes)])
            over = np.abs(norms - clip) <= 1e-5 * clip
            under = ~over & (norms < clip)
            assert (over | under).all(), norms
        else:
            norms = np.sqrt(eng.sumsq.cpu().numpy().astype(np.float64))
            over, under = norms > clip, norms < clip
        assert over.any() and under.any(), (clip, norms)
        print(f'clip_norm {clip:.4g}: {int(over.sum())} tensors clipped, {int(under.sum())} not')


def off_case(algo, A, E, n, lives, seed, **kw):
    """OFF (+ the case's options) with the clip_norm picked for this case."""
    opts = dict(OFF, **kw)
    pick = {k: v for k, v in opts.items() if k not in ('overlap', 'on_update')}
    opts['clip_norm'] = pick_clip(algo, A, E, n, lives, seed, **pick)
    opts.pop('scale', None)
    opts.pop('frames', None)
    return opts


def assert_schedule_falls(watch, rollouts, n):
    """max_step = 40: the rate falls by n / 40 of lr0 from one update to the next."""
    assert watch.updates == rollouts and len(set(watch.lrs)) == rollouts
    steps = np.diff(np.array(watch.lrs)) / LR
    np.testing.assert_allclose(steps, -n / 40.0, rtol=1e-12)


@pytest.mark.parametrize('literal_adv', [0, 1])
def test_sync_a3c_off_defaults(literal_adv):
    """literal_adv = 1: the engine passes c.literal_adv to the backward; no other engine test sets it."""
    w = Watch()
    opts = off_case('a3c', 6, 8, 5, 0, seed=131, literal_adv=literal_adv)
    check_sync_vs_oracle('a3c', 6, 8, 5, 0, iters=4, seed=131, on_update=w, **opts)
    assert_schedule_falls(w, 4, 5)


@pytest.mark.parametrize('double_q', [0, 1])
def test_sync_q_off_defaults(double_q):
    w = Watch()
    opts = off_case('q', 6, 4, 8, 3, seed=127, target_q_update_step=40, double_q=double_q)
    check_sync_vs_oracle('q', 6, 4, 8, 3, iters=3, seed=127, on_update=w, **opts)
    assert_schedule_falls(w, 3, 8)


@pytest.mark.parametrize('algo', ['a3c', 'q'])
def test_overlap_off_defaults(algo):
    """The pipelined engine: the update of rollout k - 1 runs after rollout k, with the learning
    rate of rollout k - 1's own steps."""
    w = Watch()
    A, E, n, lives, seed = (6, 8, 5, 0, 77) if algo == 'a3c' else (6, 4, 8, 3, 55)
    opts = off_case(algo, A, E, n, lives, seed, **({'target_q_update_step': 40} if algo == 'q' else {}))
    check_overlap_vs_oracle(A, E, n, lives, rollouts=4, seed=seed, algo=algo, on_update=w, **opts)
    assert_schedule_falls(w, 3, n)


@pytest.mark.timeout(600)
def test_nature_sync_off_defaults():
    w = Watch()
    opts = off_case('a3c', 6, 8, 3, 0, seed=508, scale=2.0, dqn_type='nature')
    check_sync_vs_oracle('a3c', 6, 8, 3, 0, iters=3, seed=508, scale=2.0, on_update=w, **opts)
    assert_schedule_falls(w, 3, 3)


def test_lstm_sync_off_defaults():
    from test_gpu_lstm import check_lstm_sync_vs_oracle
    w = Watch()
    opts = off_case('a3c', 6, 8, 5, 3, seed=308, lstm=True)
    opts.pop('lstm')
    check_lstm_sync_vs_oracle(6, 8, 5, 3, iters=3, on_update=w, **opts)
    assert_schedule_falls(w, 3, 5)


def test_hogwild1_off_defaults():
    """a3c_clip_grads with cfg.clip_norm, a3c_rmsprop_range with the PS's decay / momentum /
    epsilon and the learning rate through lr_dev."""
    w = Watch(clipped_buffer=True)
    opts = off_case('a3c', 6, 8, 5, 0, seed=83)
    check_hogwild1_vs_oracle(6, 8, 5, 0, iters=3, seed=83, on_update=w, **opts)
    assert_schedule_falls(w, 3, 5)


@pytest.mark.timeout(600)
def test_loopback_world2_off_defaults():
    """Two virtual ranks on one GPU: k_apply_seq (the partitioned-PS shard step) receives decay,
    momentum and epsilon by a path of its own; two RMSProp steps per update carry the momentum."""
    from test_gpu_loopback import check_loopback_vs_oracle
    w = Watch(clipped_buffer=True)
    opts = off_case('a3c', 6, 8, 5, 0, seed=31)
    check_loopback_vs_oracle(2, 8, iters=3, seed=31, frames=48, on_update=w, **opts)
    assert_schedule_falls(w, 3, 5)


def test_sync_a3c_random_start_and_action_repeat():
    """random_start = 7, action_repeat = 2 with lives: both reach the device env and the oracle's."""
    w = Watch()
    opts = off_case('a3c', 6, 8, 5, 3, seed=137, random_start=7, action_repeat=2)
    eng, ref = check_sync_vs_oracle('a3c', 6, 8, 5, 3, iters=3, seed=137, on_update=w, **opts)
    assert eng.cfg.random_start == 7 and eng.cfg.action_repeat == 2


def test_off_defaults_reached_the_oracle():
    """(CPU side of the helpers, checked where they are used.)  Every option of OFF given to
    _engine_parity.build is in the oracle's table under its own name."""
    from _engine_parity import REF_KEYS
    assert set(OFF) | {'clip_norm', 'literal_adv', 'random_start', 'action_repeat'} <= set(REF_KEYS)
    ref = EngineRef({}, 1, 1, 6, **{k: v for k, v in OFF.items() if k in REF_KEYS}, clip_norm=3.0)
    for k, v in dict(OFF, clip_norm=3.0).items():
        assert ref.h[k] == v, k


# =================================================================== 3. schedule and target sync
def set_steps(G, W):
    """start= of a parity check: the engine and the oracle resume at global step G, worker step W."""
    def start(eng, ref):
        eng.set_step(G, W)
        ref.global_step, ref.wstep0 = G, W
    return start


@pytest.mark.parametrize('G,W,max_step', [(3_000_000_000, 79_999_990, 80_000_000),
                                          (2 ** 24 + 1, 2 ** 24 + 1, 80_000_000),
                                          (2 ** 24 + 1, 2 ** 24 + 1, 2 ** 24 + 41),
                                          (0, 0, 80_000_000)])
def test_schedule_at_late_and_large_steps(G, W, max_step):
    """Engine.set_step(G, W): sched[0] is bit-equal to the float of the fp64 formula
    (engine_ref.EngineRef.next_lr) and counters[1] advances by n E per rollout.  G beyond int32
    with W at the end of training: the rate is tiny, positive, then clamped at 0, and from then on
    the parameters stand still.  2^24 + 1: step arithmetic in fp32 would lose the last bit (at
    max_step = 8e7 one step is a fifth of the rate's float spacing; the row with max_step =
    2^24 + 41 makes each step a 37th of the rate)."""
    E, n = 4, 5
    seen = []

    w = Watch(clip_mix=False)       # (the default clip_norm: no regimes to look at here)

    def on_update(it, eng, ref, lr):
        w(it, eng, ref, lr)
        assert int(eng.counters[1].item()) == G + (it + 1) * n * E
        seen.append((float(lr), eng.params.clone()))

    check_sync_vs_oracle('a3c', 6, E, n, 0, iters=4, seed=141, on_update=on_update, start=set_steps(G, W),
                         learning_rate=LR, max_step=max_step)
    lrs = [lr for lr, _ in seen]
    if W > 2 ** 25:
        assert lrs[0] > 0 and lrs[1] > 0 and lrs[2] == 0 and lrs[3] == 0, lrs
        assert lrs[0] == (max_step - (W + n - 1) + 1.) / max_step * LR
        assert torch.equal(seen[3][1], seen[2][1]) and torch.equal(seen[2][1], seen[1][1])
    else:
        assert all(lr > 0 for lr in lrs)
        if max_step < 80_000_000:
            assert len({np.float32(lr) for lr in lrs}) == 4, lrs


@pytest.mark.parametrize('P,G', [(7, 0), (32, 0), (32, 31), (33, 0), (33, 32), (33, 5)])
def test_target_sync_boundary(P, G):
    """target_q_update_step = P against rollouts of n E = 32 steps from global step G (agent.py:
    166-167: a sync when (T + 1) // P changes over the rollout).  P = 7: several multiples inside
    every rollout.  P = n E: exactly one, wherever the rollout starts; from G = 31 it ends on one.
    P = n E + 1: from G = 0 the first rollout ends exactly on the first multiple (T + 1 = 33), the
    second starts on it and crosses none -- no sync -- and the third crosses one mid-way; from
    G = 32 the first crosses none; from G = 5 every rollout crosses one mid-way.  sched[1] and the
    target parameters follow EngineRef.finish_update."""
    from src.engine import _view
    E, n = 4, 8
    flags = []

    def on_update(it, eng, ref, lr):
        g1 = ref.global_step
        g0 = g1 - n * E
        want = (g1 + 1) // P != (g0 + 1) // P
        sched = _view(eng.sched_ptr, (2,), torch.float32).cpu().numpy()
        assert sched[1] == (1.0 if want else 0.0), (it, g0, sched[1], want)
        assert torch.equal(eng.target_params, eng.params) == want, (it, g0, want)
        flags.append(want)

    check_sync_vs_oracle('q', 6, E, n, 3, iters=3, seed=149, on_update=on_update, start=set_steps(G, G),
                         learning_rate=LR, target_q_update_step=P)
    expect = {(33, 32): [False, True, True], (33, 0): [True, False, True]}.get((P, G), [True] * 3)
    assert flags == expect, flags


# =================================================================== 4. flags reach the engine
def test_main_flags_reach_engine_config(tmp_path):
    import main
    argv = ['--mode', 'engine', '--env_name', 'Pong-v0', '--num_envs', '4', '--num_frames', '48', '--iterations', '2',
            '--log_every', '2', '--logdir', str(tmp_path), '--update', 'sync', '--resume', 'false',
            '--decay', '0.9', '--momentum', '0.5', '--epsilon', '0.01', '--beta', '0.05', '--max_step', '40']
    eng = main.main(argv)
    torch.cuda.synchronize()
    c = eng.cfg
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    assert (c.decay, c.momentum, c.epsilon, c.beta) == (f32(0.9), f32(0.5), f32(0.01), f32(0.05))
    assert c.max_step == 40
    from config import get_config
    config = get_config(main.parse_flags(argv))
    assert c.gamma == c.discount == config.discount
    assert c.clip_norm == f32(config.clip_norm) and c.learning_rate == f32(config.learning_rate)
    assert int(eng.counters[1].item()) == 2 * 4 * 5 and torch.isfinite(eng.params).all()
