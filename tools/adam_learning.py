"""What the engine learns on Catch with shared Adam and, beside it, with the reference's RMSProp at the same
learning rate: DESIGN §4j's table.  The overlapped engine, 256 envs, n = 5, the reference initialisers,
§4h's epsilon schedule (learn_start = 0, ep_end_t = 1000) and target period (12800); after 0, 64, 128, ..
iterations (powers of two) the mean return of 1024 greedy episodes (Engine.play, refill, test_ep = 0), which
leaves the training state untouched.

  python tools/adam_learning.py                                       n-step Q (q_nstep = 1), seeds 1 2 3, adam then rmsprop
  python tools/adam_learning.py --q_nstep 0                           one-step Q
  python tools/adam_learning.py --algo a3c --seeds 1                  the a3c row at the defaults
  python tools/adam_learning.py --optimizer adam --learning_rate 2e-3 --seeds 1

The settings are arguments so that the table states them; the default rate is the reference's 7e-4."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
ap.add_argument('--optimizer', nargs='+', default=['adam', 'rmsprop'])
ap.add_argument('--algo', choices=['q', 'a3c'], default='q')
ap.add_argument('--q_nstep', type=int, default=1, help='algo q: 1 n-step Q-learning (§4h), 0 one-step')
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--max_iters', type=int, default=8192)
ap.add_argument('--learning_rate', type=float, default=7e-4)
ap.add_argument('--ep_end_t', type=int, default=1000, help='env steps per env over which epsilon anneals')
ap.add_argument('--target_q_update_step', type=int, default=12800, help='global env steps between target syncs')
args = ap.parse_args()

import torch  # noqa: E402
import main  # noqa: E402
from src.engine import Engine  # noqa: E402

A, FRAMES = 3, 640


def run(seed, optimizer):
    kw = dict(learning_rate=args.learning_rate)
    if args.algo == 'q':
        kw.update(learn_start=0, ep_end_t=args.ep_end_t, target_q_update_step=args.target_q_update_step)
        if args.q_nstep:
            kw['q_nstep'] = 1
    if optimizer == 'adam':                       # (rmsprop: exactly the options an engine without the argument gets)
        kw['optimizer'] = 'adam'
    eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo=args.algo, overlap=True, seed=seed,
                 num_frames=FRAMES, game='catch', **kw)
    eng.reset(main.initial_params(eng, A, args.algo, seed))
    if args.algo == 'q':
        eng.target_params.copy_(eng.params)
        eng.reset()                               # keeps the parameters, re-takes the pipeline snapshots
    play = dict(n_episode=1024, n_step=50, refill=True)
    if args.algo == 'q':                          # (a3c: the policy's own draw, as §4g's learning test plays)
        play['test_ep'] = 0.0
    done, marks, table, train_s = 0, [0] + [2 ** k for k in range(6, 32) if 2 ** k <= args.max_iters], {}, 0.0
    for m in marks:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while done < m:
            eng.iterate()
            done += 1
        torch.cuda.synchronize()
        train_s += time.perf_counter() - t0
        table[m] = round(float(eng.play(**play)['returns'].mean()), 4)
    print(json.dumps(dict(seed=seed, optimizer=optimizer, algo=args.algo, q_nstep=args.q_nstep, envs=args.envs,
                          n_step=args.n_step, learning_rate=args.learning_rate, ep_end_t=args.ep_end_t,
                          target_q_update_step=args.target_q_update_step, mean_greedy_return=table,
                          train_seconds=round(train_s, 3))), flush=True)
    eng.close()


for optimizer in args.optimizer:
    for seed in args.seeds:
        run(seed, optimizer)
