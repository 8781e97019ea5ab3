"""Would the gradient bars see a lost tail sample?  Asked of the oracle alone, no GPU.

At B = 257 and B = 515 the NIPS conv backward's last workgroup is short (one sample of two, two of
three: tests/_plan.py), and the failure such a plan invites is a last workgroup that skips its
tail or reads the sample before it.  tests/test_gpu_batch_edges.py runs those batches through
check_loss_backward, whose same-activation bar is 1e-4 relative-L2 per tensor.  Here the oracle's
fp64 gradient of the very batch that check draws (parameters seeded B + 11, inputs B + 7, A = 6) is
compared with two mutants of itself:
  drop: sample B-1 contributes nothing;
  swap: sample B-1's contribution is replaced by sample B-2's.
The gradient is a sum of per-sample terms, so the mutants are formed from single-sample backwards.
Every weight and bias tensor must miss the 1e-4 bar by at least 10x.  Measured (rel-L2 of the
mutant against the true gradient; the minimum over the two mutants decides):

  tensor        a3c B=257         a3c B=515         q B=257
                drop     swap     drop     swap     drop     swap
  l1_w          6.8e-2   9.0e-2   1.7e-2   1.8e-2   2.7e-2   2.9e-2
  l1_b          7.7e-2   1.1e-1   1.5e-2   1.6e-2   2.4e-2   2.6e-2
  l2_w          8.3e-2   1.1e-1   1.5e-2   1.6e-2   2.2e-2   2.6e-2
  l2_b          8.9e-2   1.2e-1   1.1e-2   1.1e-2   2.0e-2   2.4e-2
  l4_w / l3_w   8.2e-2   1.1e-1   9.4e-3   8.9e-3   2.2e-2   2.6e-2
  l4_b / l3_b   9.7e-2   1.4e-1   8.2e-3   7.6e-3   1.9e-2   2.3e-2
  p_w           8.2e-2   9.6e-2   2.4e-2   2.4e-2   -        -
  p_b           1.1e-1   1.3e-1   2.1e-2   2.1e-2   -        -
  q_w           1.0e-1   1.6e-1   6.2e-3   4.8e-3   1.8e-2   2.1e-2
  q_b           6.2e+0   9.9e+0   5.4e-3   3.7e-3   1.7e-2   1.9e-2

The smallest entry, 3.7e-3 (q_b, a3c B = 515, swap), misses the bar 37-fold: every tensor meets
the condition at the seeds the GPU cases use, so no per-sample GPU check is needed."""
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')     # (_net_parity imports it)

from oracle import ref_cpu as R  # noqa: E402
from _net_parity import make_params, rel_l2  # noqa: E402

BAR = 1e-4          # check_loss_backward's same-activation bound
A = 6


def batch(algo, B):
    """check_loss_backward's own draw (tests/_net_parity.py) and the oracle's fp64 pass over it."""
    from src.kernels import param_names_shapes      # (Net.names_shapes, without a device)
    p = make_params(types.SimpleNamespace(names_shapes=param_names_shapes(A, algo)), seed=B + 11, scale=4.0)
    rng = np.random.default_rng(B + 7)
    planes = rng.integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)
    actions = rng.integers(0, A, B).astype(np.int32)
    target = rng.standard_normal(B).astype(np.float32)
    f = R.forward(p, R.states_nhwc(planes), algo, dtype=np.float64)
    if algo == 'a3c':
        _, dz = R.a3c_loss_and_dz(f['z'], actions, target.astype(np.float64), 0.01, False)
    else:
        _, dz = R.q_loss_and_dz(f['z'], actions, target.astype(np.float64))
    return p, f, dz


def sample_grad(p, f, dz, algo, b):
    """Sample b's term of the batch gradient (its row of dz already carries q's 1 / B)."""
    one = dict(z=f['z'][b:b + 1], h3=f['h3'][b:b + 1], flat=f['flat'][b:b + 1],
               acts=[a[b:b + 1] for a in f['acts']])
    return R.backward(p, one, dz[b:b + 1], algo)


@pytest.mark.parametrize('algo,B', [('a3c', 257), ('a3c', 515), ('q', 257)])
def test_lost_tail_sample_misses_the_bar_tenfold(algo, B):
    p, f, dz = batch(algo, B)
    g = R.backward(p, f, dz, algo)
    last, prev = sample_grad(p, f, dz, algo, B - 1), sample_grad(p, f, dz, algo, B - 2)
    # the per-sample terms do sum to the batch gradient (the mutants below rest on it)
    head = R.backward(p, dict(z=f['z'][:B - 1], h3=f['h3'][:B - 1], flat=f['flat'][:B - 1],
                              acts=[a[:B - 1] for a in f['acts']]), dz[:B - 1], algo)
    assert sorted(g) == sorted(p)
    for k in g:
        assert rel_l2(head[k] + last[k], g[k]) < 1e-12, k
        drop = rel_l2(g[k] - last[k], g[k])
        swap = rel_l2(g[k] - last[k] + prev[k], g[k])
        print(f'{algo} B={B} {k:5s} drop {drop:.1e} swap {swap:.1e}')
        assert min(drop, swap) >= 10 * BAR, (k, drop, swap)
