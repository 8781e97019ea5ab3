"""The painted pool (tests/_painted.py) on the CPU: what the GPU tests of tests/test_gpu_painted.py
rely on, asserted without a GPU.

  * frames 0..23 give the reference's recorded golden screens;
  * the 48 screens together hold at least 250 of the 255 reachable byte values, 0 and 254 among them
    (white is 254: the truncated luminance of (255, 255, 255)), and every output pixel is 0 in one
    frame and 254 in another -- the hashed pool's screens stay within 54..197;
  * the numpy restatement of the int8 matrix-core resample (tests/test_screen_i8_algorithm.py) equals
    the oracle on all 48;
  * the coverage condition of every ring case: its env alone, stepped with uniformly drawn actions,
    shows all 48 frames within the case's steps.  (The GPU test asserts the same of the engine's own
    actions.)  A seed that misses is replaced, never the condition."""
import os

import numpy as np
import pytest

import _catch_ref as C
import _painted as P
from oracle import ref_cpu as R
from oracle.synthetic_env import SyntheticAtari, pool_frame
from test_screen_i8_algorithm import screen_resample_i8


def test_first_24_are_the_reference_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, 'screen_golden.npz'))
    assert [(str(k), int(s)) for k, s in zip(g['kinds'], g['seeds'])] == list(P.SPECS)
    assert np.array_equal(P.painted_screens()[:P.N_GOLDEN], g['screens'])


def test_frames_are_what_the_module_says():
    fr = P.painted_frames()
    assert fr.shape == (48, 210, 160, 3) and fr.dtype == np.uint8 and len(P.STRESS) == 24
    stress = fr[P.N_GOLDEN:]
    pure = [P.N_GOLDEN + P.STRESS.index(f'pure {c}') for c in 'RGB']
    grey = [i for i in range(P.N_GOLDEN, 48) if i not in pure]
    assert all((fr[i][..., 0] == fr[i][..., 1]).all() and (fr[i][..., 1] == fr[i][..., 2]).all() for i in grey)
    for v, i in P.GREYS.items():
        assert (fr[i] == v).all()
    corners = fr[P.N_GOLDEN + P.STRESS.index('white pixel in each corner')][..., 0]
    assert corners.sum() == 4 * 255 and corners[0, 0] == corners[0, 159] == corners[209, 0] == corners[209, 159] == 255
    last = fr[P.N_GOLDEN + P.STRESS.index('last two rows and columns white')][..., 0]
    assert (last[208:] == 255).all() and (last[:, 158:] == 255).all() and not last[:208, :158].any()
    assert len({f.tobytes() for f in stress}) == 24


def test_screens_span_the_byte_range():
    S = P.painted_screens()
    vals = np.unique(S)
    print('distinct byte values', len(vals), 'min', int(vals.min()), 'max', int(vals.max()))
    assert len(vals) >= 250 and vals.min() == 0 and vals.max() == 254
    assert (S.min(axis=0) == 0).all() and (S.max(axis=0) == 254).all()
    noise = np.unique(np.stack([R.screen(pool_frame(131, f)) for f in range(4)]))
    assert noise.min() > 40 and noise.max() < 215      # what the hashed pool reaches


def test_i8_restatement_equals_the_oracle_on_every_painted_frame():
    for f, (frame, want) in enumerate(zip(P.painted_frames(), P.painted_screens())):
        np.testing.assert_array_equal(screen_resample_i8(R.luminance_u8(frame)), want, err_msg=str(f))


def _env_of(case):
    catch = case['game'] == 'catch'

    def make():
        cls = C.CatchEnv if catch else SyntheticAtari
        env = cls(case['seed'], P.RING_E, C.FRAMES if catch else P.N_FRAMES, case['A'], case['lives'])
        env.new_random_game()
        return env
    return make


@pytest.mark.parametrize('name', sorted(P.RING_CASES))
def test_ring_case_covers_every_frame(name):
    case = P.RING_CASES[name]
    seen = P.uniform_coverage(_env_of(case), P.RING_E, P.RING_N, P.RING_ITERS, case['seed'], case['A'])
    assert seen == set(range(P.N_FRAMES)), (name, sorted(set(range(P.N_FRAMES)) - seen))


def test_batched_env_case_covers_every_frame():
    c = P.BATCHED_ENV_CASE
    make = _env_of(dict(game='synth', seed=c['seed'], A=c['A'], lives=0))
    seen = P.uniform_coverage(make, c['E'], 1, c['steps'], c['seed'], c['A'])
    assert seen == set(range(P.N_FRAMES)), sorted(set(range(P.N_FRAMES)) - seen)
