"""The painted pool: 48 frames that put every device form of Environment.screen (luminance, then
Pillow-bilinear 210x160 -> 84x84) on the reference's own golden screens and on saturated, flat
and hard-edged images.  Test infrastructure only (imported by tests/test_painted_cpu.py,
tests/test_gpu_painted.py and tests/test_gpu_kernels.py).

The engine's pool is filled by a Philox hash: white noise, whose screens span bytes 54..197 only.
Engine.frame_pool and BatchedEnvironment.frame_pool are writable views, so a test replaces the
hashed frames by these after the reset and tells the oracle (EngineRef._screen) the same:

  frames  0..23   make_goldens.frame_from_spec(kind, seed) of the 24 SPECS, in order; their screens
                  are the reference's recorded tests/golden/screen_golden.npz['screens'];
  frames 24..47   procedural stress frames (STRESS, in order), R = G = B except the three pure
                  colours, white = 255 (truncated luminance 254).

paint / paint84 / paint_catch are start(eng, ref) hooks of the parity checks (tests/_engine_parity.py).
The ring planes written before the hook ran (the four begin planes) stay noise on both sides."""
import functools
import types

import numpy as np

from make_goldens import SPECS, frame_from_spec
from oracle import ref_cpu as R

H, W = 210, 160
N_GOLDEN, N_FRAMES = 24, 48


def _grey(img):
    """[210, 160] values -> u8 [210, 160, 3] with R = G = B."""
    g = np.asarray(img).astype(np.uint8)
    assert g.shape == (H, W)
    return np.repeat(g[:, :, None], 3, axis=2)


def _stress():
    y, x = np.indices((H, W))
    out = []

    def add(name, img):
        out.append((name, img if img.ndim == 3 else _grey(img)))

    add('checker 1 px', ((y + x) % 2) * 255)
    add('checker 2 px', ((y // 2 + x // 2) % 2) * 255)
    for p in (2, 3, 5):
        add(f'column stripes period {p}', (x % p == 0) * 255)
    for p in (2, 3, 5):
        add(f'row stripes period {p}', (y % p == 0) * 255)
    add('vertical edge', (x >= W // 2) * 255)
    add('horizontal edge', (y >= H // 2) * 255)
    add('16 px blocks', ((y // 16 + x // 16) % 2) * 255)       # the MFMA tile pitch
    corners = np.zeros((H, W), np.int64)
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        corners[cy, cx] = 255
    add('white pixel in each corner', corners)
    for cy, cx in ((0, 0), (H - 1, W - 1)):
        one = np.full((H, W), 255, np.int64)
        one[cy, cx] = 0
        add(f'black pixel at ({cy}, {cx}) on white', one)
    add('last two rows and columns white', ((y >= H - 2) | (x >= W - 2)) * 255)
    add('ramp y + x', (y + x) % 256)
    add('ramp 3 y + 7 x', (3 * y + 7 * x) % 256)
    for v in (1, 236, 254):
        add(f'flat grey {v}', np.full((H, W), v))
    for c, name in enumerate('RGB'):
        pure = np.zeros((H, W, 3), np.uint8)
        pure[:, :, c] = 255
        add(f'pure {name}', pure)
    add('binary noise', np.random.default_rng(20).integers(0, 2, (H, W)) * 255)
    return out


STRESS = [name for name, _ in _stress()]
assert len(STRESS) == N_FRAMES - N_GOLDEN
GREYS = {v: N_GOLDEN + STRESS.index(f'flat grey {v}') for v in (1, 236, 254)}     # grey value -> frame index


@functools.lru_cache(maxsize=None)
def painted_frames():
    """u8 [48, 210, 160, 3], read-only."""
    fr = np.stack([frame_from_spec(kind, seed) for kind, seed in SPECS] + [img for _, img in _stress()])
    assert fr.shape == (N_FRAMES, H, W, 3) and fr.dtype == np.uint8
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def painted_screens():
    """u8 [48, 84, 84]: the oracle's Environment.screen of every painted frame, read-only."""
    s = np.stack([R.screen(f) for f in painted_frames()])
    s.setflags(write=False)
    return s


def id_plane(f):
    """A plane that names its frame: what a second oracle is told (tell) where a replay has to say
    which frame a ring slot holds.  (The screens themselves cannot: white and flat grey 254 both
    come out as 254.)"""
    return np.full((84, 84), int(f) % N_FRAMES, np.uint8)


def to_pool(eng, frames):
    import torch
    pool = eng.frame_pool
    assert tuple(pool.shape) == frames.shape, (tuple(pool.shape), frames.shape)
    torch.cuda.synchronize()
    pool.copy_(torch.as_tensor(np.ascontiguousarray(frames)).cuda())
    torch.cuda.synchronize()


def tell(ref, screen):
    ref._screen = screen
    ref._screens.clear()


def paint(eng, ref):
    """start hook: the 48 frames into the engine's RGB pool (num_frames = 48), their screens as the
    oracle's.  After the reset on both sides: a reset fills the pool by hash again."""
    to_pool(eng, painted_frames())
    tell(ref, lambda f: painted_screens()[int(f)])


def paint84(eng, ref):
    """start hook of frame84 = 1 engines: the pool holds 84x84 planes, painted with the screens."""
    to_pool(eng, painted_screens())
    tell(ref, lambda f: painted_screens()[int(f)])


def paint_catch(eng, ref):
    """start hook of Catch engines: the frame index is the game's state, f < 640; frame f of the pool
    becomes painted frame f % 48."""
    n = int(eng.frame_pool.shape[0])
    to_pool(eng, painted_frames()[np.arange(n) % N_FRAMES])
    tell(ref, lambda f: painted_screens()[int(f) % N_FRAMES])


def step_frames(ref, actions):
    """The oracle's env alone, one rollout: actions [n, E] -> the frame index of every step's
    observed screen [n, E] (EngineRef.iterate's env calls, no network pass)."""
    frames = []
    for a in np.asarray(actions):
        frame, _, term = ref.env.act(a.astype(np.int32), is_training=True)
        frames.append(frame.astype(np.int64))
        if term.any():
            ref.env.new_random_game(term.astype(bool))
    return np.stack(frames)


def uniform_coverage(make_env, E, n, iterations, seed, A, num_frames=N_FRAMES):
    """The coverage condition of a ring case, on the CPU: the env alone (make_env() after its
    new_random_game), stepped with actions drawn uniformly by `seed`; returns the set of painted
    frame indices its n * iterations steps observe."""
    ref = types.SimpleNamespace(env=make_env())
    rng = np.random.default_rng(seed)
    seen = set()
    for _ in range(iterations):
        seen |= set((step_frames(ref, rng.integers(0, A, (n, E))) % num_frames).reshape(-1).tolist())
    return seen


# ---------------------------------------------------------------------------------- ring cases
# The engine configurations of tests/test_gpu_painted.py's ring tests (its docstring has the table of
# kernels they reach), here so that tests/test_painted_cpu.py can hold every (E, n, iterations, seed)
# to the coverage condition without a GPU.  kw: engine options; env: A3C_* variables of the create.
RING_E, RING_N, RING_ITERS = 16, 5, 6


def _case(seed, algo='a3c', A=6, lives=0, hook='paint', lstm=False, game='synth', env=None, **kw):
    return dict(seed=seed, algo=algo, A=A, lives=lives, hook=hook, lstm=lstm, game=game, env=env or {}, kw=kw)


RING_CASES = {
    'a3c-overlap-l2bits0': _case(701, overlap=True, env={'A3C_L2BITS': '0'}),
    'a3c-overlap-l2bits1': _case(702, overlap=True, env={'A3C_L2BITS': '1'}),
    'q-overlap': _case(703, algo='q', overlap=True),
    'a3c-sync-fused': _case(704, lives=3, env={'A3C_FUSE_CONV': '1'}),
    'q-sync-fused': _case(705, algo='q', env={'A3C_FUSE_CONV': '1'}),
    'a3c-sync': _case(706, A=4, lives=5),
    'a3c-overlap-unfused': _case(707, overlap=True, env={'A3C_FUSE_CONV': '0'}),
    'lstm-overlap': _case(708, lstm=True, overlap=True),
    'lstm-sync': _case(709, lstm=True, lives=3),
    'nature-sync': _case(710, dqn_type='nature'),
    'nature-overlap': _case(711, dqn_type='nature', overlap=True),
    'unfused-screen': _case(712, env={'A3C_FUSED_SCREEN': '0'}),
    'frame84-overlap': _case(713, hook='paint84', overlap=True, frame84=1),
    'frame84-nature-sync': _case(714, hook='paint84', dqn_type='nature', frame84=1),
    'catch-overlap': _case(715, A=3, hook='paint_catch', game='catch', overlap=True),
    'host-env': _case(716, lives=3, external_env=True),
}
BATCHED_ENV_CASE = dict(seed=717, E=RING_E, steps=RING_N * RING_ITERS, A=6)
