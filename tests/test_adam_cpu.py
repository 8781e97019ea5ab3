"""Shared Adam (Engine(optimizer='adam'), main.py --optimizer adam) without a GPU: the numpy
restatement tests/_adam_ref.py against torch.optim.Adam and against the closed form of its first step; the
flags; the C ABI (symbols, signatures, the setter's rejections before any device work); the partitioned PS
under gloo with a numpy stand-in of the engine's shard apply; the checkpoint's TF1 names and the fallback
between optimizers."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _adam_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'async-rl-tensorflow_amd')
SO = os.path.join(PKG, 'lib', 'liba3c_hip.so')
HEADER = os.path.join(ROOT, 'include', 'a3c_hip.h')


# ------------------------------------------------------------------ 1. the restatement against torch
def run_both(eps, gmag, n=1000, steps=10, lr=7e-4, seed=0):
    """The total step w_T - w_0 of the restatement in fp64 and of torch.optim.Adam in fp64 on the same
    gradients: |g| log-uniform in gmag, random signs."""
    rng = np.random.default_rng(seed)
    w0 = rng.standard_normal(n)
    gs = [np.exp(rng.uniform(np.log(gmag[0]), np.log(gmag[1]), n)) * rng.choice([-1.0, 1.0], n) for _ in range(steps)]
    w = w0.copy()
    opt = AR.Adam(eps=eps, dtype=np.float64)
    for g in gs:
        opt.step(w, g, lr)
    t = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    topt = torch.optim.Adam([t], lr=lr, betas=(0.9, 0.999), eps=eps)
    for g in gs:
        t.grad = torch.tensor(g, dtype=torch.float64)
        topt.step()
    return w - w0, t.detach().numpy() - w0


def test_restatement_is_adam_up_to_where_eps_sits():
    """With eps far below sqrt(v) the two are the same rule: relative L2 of the total step under 1e-8
    (measured 2.4e-10: the orders of the fp64 operations differ)."""
    mine, ref = run_both(eps=1e-12, gmag=(1e-3, 1.0))
    rel = np.linalg.norm(mine - ref) / np.linalg.norm(ref)
    print('rel L2 of the total step against torch.optim.Adam:', rel)
    assert rel < 1e-8


def test_eps_is_placed_as_tensorflow_places_it():
    """TF adds eps to sqrt(v) under the bias-corrected step size; torch adds it to sqrt(v / (1 - beta2^t)).
    With eps = 1e-3 next to |g| ~ 1e-3 the two differ by far more than rounding."""
    mine, ref = run_both(eps=1e-3, gmag=(0.9e-3, 1.1e-3))
    rel = np.linalg.norm(mine - ref) / np.linalg.norm(ref)
    print('rel L2 with eps = 1e-3:', rel)
    assert rel > 1e-3


# ------------------------------------------------------------------ 2. the first step
def test_first_step_is_lr_times_sign_and_scale_invariant():
    """Step 1 from m = v = 0.  m = g (1 - beta1), v = g^2 (1 - beta2) and alpha = lr sqrt(1 - beta2) / (1 - beta1)
    give w -= lr g / (|g| + eps / sqrt(1 - beta2)): eps is divided by sqrt(1 - beta2) = 0.0316, not multiplied
    by it.  So the step is lr sign(g) up to eps / (|g| sqrt(1 - beta2)) = 3.2e-7 / |g|, and scaling g by 1,000
    changes it by less than that: with |g| in [0.1, 1] under 3.2e-6, inside the 1e-5 asserted.  (RMSProp with
    epsilon 0.1 scales with g: DESIGN §4h.)  The closed form's own bar: (float)beta2 = 0.999 + 1.3e-8 makes
    1 - beta2 1.3e-5 smaller and its square root 6.4e-6, (float)beta1 adds 2.4e-7, four fp32 roundings 2.4e-7:
    1e-5."""
    rng = np.random.default_rng(1)
    lr = 7e-4
    g = (rng.uniform(0.1, 1.0, 512) * rng.choice([-1.0, 1.0], 512)).astype(np.float32)
    steps = []
    for scale in (1.0, 1000.0):
        w = np.zeros(512, np.float32)
        AR.Adam().step(w, g * np.float32(scale), lr)
        gd = g.astype(np.float64) * scale
        want = -lr * gd / (np.abs(gd) + AR.EPS / np.sqrt(1 - AR.BETA2))
        np.testing.assert_allclose(w, want, rtol=1e-5)
        steps.append(w.astype(np.float64))
    assert np.abs(steps[1] / steps[0] - 1.0).max() < 1e-5
    assert np.allclose(np.abs(steps[0]), lr, rtol=2e-5)


def test_alpha_and_products():
    opt = AR.Adam()
    w = np.zeros(4, np.float32)
    for t in range(1, 6):
        a = opt.step(w, np.ones(4, np.float32), 7e-4)
        assert a.dtype == np.float32 and a == AR.alpha(7e-4, opt.p1, opt.p2)
    p1 = p2 = 1.0
    for _ in range(5):
        p1 *= 0.9
        p2 *= 0.999
    assert (opt.p1, opt.p2) == (p1, p2)
    sys.path.insert(0, PKG)
    from src.optim import adam_alpha
    assert adam_alpha(7e-4, p1, p2) == float(a)            # the drop-in optimizer's host alpha is this one


# ------------------------------------------------------------------ 3. flags
def flags(*argv):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import main
    return main, main.parse_flags(list(argv))


def test_flags_default_is_rmsprop_and_adds_no_keyword():
    main, f = flags()
    assert (f.optimizer, f.adam_beta1, f.adam_beta2, f.adam_epsilon) == ('rmsprop', 0.9, 0.999, 1e-8)
    assert main.engine_options(f) == dict(lstm=False) and main.adam_options(f) == {}
    main, f = flags('--optimizer', 'rmsprop', '--adam_beta1', '0.5')        # Adam's constants without Adam: unused
    assert main.engine_options(f) == dict(lstm=False)


def test_flags_adam_reaches_the_engine():
    main, f = flags('--optimizer', 'adam', '--algo', 'q', '--q_nstep', 'true')
    assert main.engine_options(f) == dict(lstm=False, q_nstep=1, optimizer='adam', adam_beta1=0.9, adam_beta2=0.999,
                                          adam_epsilon=1e-8)
    main, f = flags('--optimizer', 'adam', '--adam_beta1', '0.8', '--adam_beta2', '0.99', '--adam_epsilon', '1e-6',
                    '--update', 'sync')
    assert main.engine_options(f) == dict(lstm=False, optimizer='adam', adam_beta1=0.8, adam_beta2=0.99,
                                          adam_epsilon=1e-6)
    with pytest.raises(SystemExit):
        flags('--optimizer', 'adagrad')


def test_flags_reject_hogwild_and_bad_constants():
    main, f = flags('--optimizer', 'adam', '--update', 'hogwild')
    with pytest.raises(ValueError, match='hogwild'):
        main.engine_options(f)
    main, f = flags('--update', 'hogwild')
    assert main.engine_options(f) == dict(lstm=False)
    for argv in (('--adam_beta1', '1.0'), ('--adam_beta1=-0.1',), ('--adam_beta2', '1.0'), ('--adam_beta2', 'nan'),
                 ('--adam_epsilon', '0'), ('--adam_epsilon=-1e-8',)):
        main, f = flags('--optimizer', 'adam', *argv)
        with pytest.raises(ValueError, match='adam_'):
            main.engine_options(f)
        f.mode = 'agent'
        with pytest.raises(ValueError, match='adam_'):
            main.adam_options(f)


def test_engine_rejects_before_device_work(monkeypatch):
    """Engine(optimizer=...) checks the name and the constants before it asks for a device."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import _lib, engine
    monkeypatch.setattr(_lib, 'require_device', lambda: (_ for _ in ()).throw(AssertionError('device asked for')))
    with pytest.raises(ValueError, match='unknown optimizer'):
        engine.Engine(optimizer='adagrad')
    with pytest.raises(ValueError, match='adam_beta1'):
        engine.Engine(optimizer='adam', adam_beta1=1.0)
    with pytest.raises(ValueError, match='adam_epsilon'):
        engine.Engine(optimizer='adam', adam_epsilon=0.0)


# ------------------------------------------------------------------ 4. ABI
NEW_SYMBOLS = ('a3c_clip_adam_apply', 'a3c_engine_set_optimizer', 'a3c_engine_adam_powers',
               'a3c_engine_set_adam_powers')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(SO):
        pytest.skip('liba3c_hip.so not built (run __graft_entry__.build())')
    return ctypes.CDLL(SO)


def test_new_symbols(lib):
    from src import _lib
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + '(' in header, name
    assert '#define A3C_OPT_RMSPROP 0' in header and '#define A3C_OPT_ADAM 1' in header
    assert (_lib.A3C_OPT_RMSPROP, _lib.A3C_OPT_ADAM) == (0, 1)
    assert _lib.SIGNATURES['a3c_clip_adam_apply'] == _lib.SIGNATURES['a3c_clip_rmsprop_apply']
    assert _lib.SIGNATURES['a3c_engine_set_optimizer'][1][1:] == [ctypes.c_int] + [ctypes.c_double] * 3
    assert ctypes.sizeof(_lib.EngineOpts) == 12 and ctypes.sizeof(_lib.EngineConfig) == 184       # neither grew


def test_setter_rejects_before_it_touches_the_device(lib):
    """kind, the betas and eps are checked before the engine is looked at: with a NULL engine the message names
    the argument, and only valid arguments reach the NULL check.  No device is needed."""
    from src import _lib
    f = lib.a3c_engine_set_optimizer
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.a3c_last_error.restype = ctypes.c_char_p
    nan = float('nan')
    for args, word in (((2, 0.9, 0.999, 1e-8), b'kind'), ((-1, 0.9, 0.999, 1e-8), b'kind'),
                       ((1, 1.0, 0.999, 1e-8), b'beta'), ((1, -0.1, 0.999, 1e-8), b'beta'),
                       ((1, 0.9, 1.0, 1e-8), b'beta'), ((1, 0.9, nan, 1e-8), b'beta'), ((0, 1.5, 0.999, 1e-8), b'beta'),
                       ((1, 0.9, 0.999, 0.0), b'eps'), ((1, 0.9, 0.999, -1.0), b'eps'), ((1, 0.9, 0.999, nan), b'eps'),
                       ((1, 0.9, 0.999, 1e-8), b'null'), ((0, 0.9, 0.999, 1e-8), b'null')):
        assert f(None, *args) == _lib.ERR_INVALID and word in lib.a3c_last_error(), (args, lib.a3c_last_error())
    g = lib.a3c_engine_adam_powers
    g.restype = ctypes.c_int
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert g(None, None, None, None) == _lib.ERR_INVALID
    s = lib.a3c_engine_set_adam_powers
    s.restype = ctypes.c_int
    s.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    assert s(None, 0.5, 0.5, None) == _lib.ERR_INVALID


# ------------------------------------------------------------------ 5. the partitioned PS under gloo
TOTAL, ITERS, LR = 64 * 9, 3, 7e-4          # nine 64-float blocks: ragged last range at world 2 and 4


def rank_grad(rank, it):
    """Rank `rank`'s (already clipped) gradient of iteration `it`: |g| over four decades."""
    rng = np.random.default_rng(1000 * it + rank)
    return (np.exp(rng.uniform(np.log(1e-4), 0.0, TOTAL)) * rng.choice([-1.0, 1.0], TOTAL)).astype(np.float32)


class CpuAdamShardEngine:
    """The engine's partitioned-PS interface (apply_shard / apply_commit) in numpy: step q of a shard
    takes alpha from the products advanced q + 1 times, and the commit advances them by the ranks applied."""

    def __init__(self):
        self.params = np.linspace(-1.0, 1.0, TOTAL).astype(np.float32)
        self.m, self.v = np.zeros(TOTAL, np.float32), np.zeros(TOTAL, np.float32)
        self.p1 = self.p2 = 1.0
        self.split_point, self.grads, self.nranks, self.history = 0, None, 0, []

    def apply_shard(self, recv, nranks, lo, n, w_out):
        opt = AR.Adam()
        opt.p1, opt.p2 = self.p1, self.p2
        opt.m[None], opt.v[None] = self.m[lo:lo + n], self.v[lo:lo + n]        # views: updated in place
        w = self.params[lo:lo + n].copy()
        opt.sequence(w, recv.numpy()[:nranks * n].reshape(nranks, n), LR)
        w_out[:n] = torch.as_tensor(w)
        self.nranks = nranks

    def apply_commit(self, gathered):
        self.params[:] = gathered.numpy()[:TOTAL]
        for _ in range(self.nranks):
            self.p1 *= AR.BETA1
            self.p2 *= AR.BETA2
        self.nranks = 0
        self.history.append((self.p1, self.p2))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ps_worker(rank, world, port, out):
    for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from src.distributed import PartitionedPS, init_from_env
    init_from_env(backend='gloo')
    eng = CpuAdamShardEngine()
    ps = PartitionedPS(TOTAL, device='cpu')
    for it in range(ITERS):
        eng.grads = torch.as_tensor(rank_grad(rank, it))
        ps.apply(eng)
    out[rank] = dict(params=eng.params.copy(), history=list(eng.history), lo=ps.lo, n=ps.n)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize('world', [2, 4])
def test_gloo_partitioned_ps_applies_sequential_adam_steps(world):
    """Every rank's gradient is an Adam step of its own, in rank order, each with the alpha of its own step
    count; the replicas agree bit for bit with one process doing that, and the products advance by `world`
    per iteration."""
    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_ps_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    w = np.linspace(-1.0, 1.0, TOTAL).astype(np.float32)
    opt = AR.Adam()
    hist = []
    for it in range(ITERS):
        opt.sequence(w, [rank_grad(r, it) for r in range(world)], LR)
        hist.append((opt.p1, opt.p2))
    n = res[0]['n']
    assert sum(n) == TOTAL and n[-1] < n[0]
    for r in range(world):
        assert np.array_equal(res[r]['params'], w), r
        assert res[r]['history'] == hist, r
    p1 = 1.0
    for _ in range(ITERS * world):
        p1 *= AR.BETA1
    assert hist[-1][0] == p1 and len(hist) == ITERS


# ------------------------------------------------------------------ 6. checkpoint
NS = [('l1_w', (8, 8, 4, 16)), ('l1_b', (16,)), ('l2_w', (4, 4, 16, 32)), ('l2_b', (32,)),
      ('l4_w', (2592, 256)), ('l4_b', (256,)), ('p_w', (256, 6)), ('p_b', (6,)), ('q_w', (256, 1)), ('q_b', (1,))]


class FakeEngine:
    """What src/checkpoint.py touches of src/engine.Engine, over CPU tensors."""

    def __init__(self, optimizer, seed=None):
        self.algo, self.external_env, self.overlap, self.optimizer = 'a3c', False, False, optimizer
        self.offsets, self.sizes, off = [], [], 0
        for _, shp in NS:
            self.offsets.append(off)
            self.sizes.append(int(np.prod(shp)))
            off = -(-(off + self.sizes[-1]) // 64) * 64
        self.params, self.target_params = torch.zeros(off), torch.zeros(off)
        self.ms, self.mom = torch.zeros(off), torch.zeros(off)
        self.counters = torch.zeros(3, dtype=torch.int64)
        self._powers = (1.0, 1.0)
        self.reset()
        if seed is not None:
            g = torch.Generator().manual_seed(seed)
            for t in (self.params, self.ms, self.mom):
                for o, s in zip(self.offsets, self.sizes):
                    t[o:o + s] = torch.rand(s, generator=g)
            self._powers = (0.9 ** 7, 0.999 ** 7) if optimizer == 'adam' else (1.0, 1.0)
            self.counters[1] = 4242

    def reset(self, host_params=None):
        if host_params is not None:
            self.params.copy_(torch.as_tensor(host_params))
        self.ms.fill_(0.0 if self.optimizer == 'adam' else 1.0)
        self.mom.zero_()
        self._powers = (1.0, 1.0)

    @property
    def adam_powers(self):
        return self._powers

    @adam_powers.setter
    def adam_powers(self, p):
        assert self.optimizer == 'adam'
        self._powers = (float(p[0]), float(p[1]))

    def set_step(self, g, w=None):
        self.counters[1] = g


def test_checkpoint_round_trip_under_tf1_names():
    from src import checkpoint as C
    a = FakeEngine('adam', seed=3)
    arrays = C.engine_arrays(a, NS, with_state=False)
    assert C.slot_names('x') == ('x/RMSProp', 'x/RMSProp_1') and C.slot_names('x', 'adam') == ('x/Adam_1', 'x/Adam')
    o, s = a.offsets[4], a.sizes[4]
    assert np.array_equal(arrays['l4_linear/Matrix/Adam'].reshape(-1), a.mom[o:o + s].numpy())       # m
    assert np.array_equal(arrays['l4_linear/Matrix/Adam_1'].reshape(-1), a.ms[o:o + s].numpy())      # v
    assert arrays['beta1_power'].dtype == np.float64 and float(arrays['beta1_power']) == 0.9 ** 7
    assert float(arrays['beta2_power']) == 0.999 ** 7 and not any('RMSProp' in k for k in arrays)
    b = FakeEngine('adam')
    assert C.engine_restore(b, NS, arrays) == 4242
    for name in ('params', 'ms', 'mom'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.adam_powers == a.adam_powers
    r = C.engine_arrays(FakeEngine('rmsprop', seed=4), NS, with_state=False)      # RMSProp files are as they were
    assert 'beta1_power' not in r and 'l1_conv/w/RMSProp' in r and not any('/Adam' in k for k in r)


@pytest.mark.parametrize('wrote,reads', [('rmsprop', 'adam'), ('adam', 'rmsprop')])
def test_checkpoint_of_the_other_optimizer_restores_parameters_and_step(wrote, reads, capsys):
    from src import checkpoint as C
    a = FakeEngine(wrote, seed=5)
    arrays = C.engine_arrays(a, NS, with_state=False)
    b = FakeEngine(reads)
    assert C.engine_restore(b, NS, arrays) == 4242
    assert torch.equal(a.params, b.params) and int(b.counters[1]) == 4242
    fresh = FakeEngine(reads)
    assert torch.equal(b.ms, fresh.ms) and torch.equal(b.mom, fresh.mom) and b.adam_powers == (1.0, 1.0)
    err = capsys.readouterr().err
    assert wrote in err and reads in err and 'slots fresh' in err
    C.engine_restore(FakeEngine(wrote), NS, arrays)                 # the same optimizer: no such line
    assert 'slots fresh' not in capsys.readouterr().err
