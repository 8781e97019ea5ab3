"""What the engine learns on CatchMemory-v0 (Catch with rules (1, 4): DESIGN §4k's table) with the LSTM
head and, beside it, with the feed-forward head, which provably cannot leave R_ML = -0.7202.  The
overlapped a3c engine, 256 envs, the reference initialisers, default hyperparameters; after 0, 64, 128, ..
iterations (powers of two) the mean return of 4096 episodes played by sampling from the policy
(Engine.play, refill), which leaves the training state untouched.  One JSON line per seed, head, n_step
and budget.

  python tools/catch_memory_learning.py                              seeds 1 2 3, lstm and ff, n_step 5 and 9
  python tools/catch_memory_learning.py --heads lstm --n_step 9 --optimizer adam
  python tools/catch_memory_learning.py --rules 10 0                 Catch-v0 through the same setter
  python tools/catch_memory_learning.py --first_screen true --heads lstm     DESIGN §4l's table: the training
                                                                     rollouts see each episode's first screen

At n_step 9 rollouts and episodes align (every episode is 9 steps), so the LSTM's BPTT spans the episode."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
ap.add_argument('--heads', nargs='+', choices=['lstm', 'ff'], default=['lstm', 'ff'])
ap.add_argument('--n_step', type=int, nargs='+', default=[5, 9])
ap.add_argument('--optimizer', choices=['rmsprop', 'adam'], default='rmsprop')
ap.add_argument('--rules', type=int, nargs=2, default=[1, 4], metavar=('VISIBLE', 'FROZEN'))
ap.add_argument('--first_screen', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=False)
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--episodes', type=int, default=4096)
ap.add_argument('--max_iters', type=int, default=16384)
args = ap.parse_args()

import torch  # noqa: E402
import main  # noqa: E402
from src.engine import Engine  # noqa: E402

A, FRAMES = 3, 640


def run(seed, head, n_step):
    kw = dict(optimizer='adam') if args.optimizer == 'adam' else {}
    if args.first_screen:
        kw['first_screen'] = True
    eng = Engine(num_envs=args.envs, n_step=n_step, action_size=A, overlap=True, seed=seed, num_frames=FRAMES,
                 lstm=head == 'lstm', game='catch', catch_rules=tuple(args.rules), **kw)
    eng.reset(main.initial_params(eng, A, 'a3c', seed))
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    done, train_s = 0, 0.0
    for m in [0] + [2 ** k for k in range(6, 32) if 2 ** k <= args.max_iters]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while done < m:
            eng.iterate()
            done += 1
        torch.cuda.synchronize()
        train_s += time.perf_counter() - t0
        ret = eng.play(n_episode=args.episodes, n_step=50, refill=True)['returns']
        print(json.dumps(dict(seed=seed, head=head, n_step=n_step, optimizer=args.optimizer, rules=list(args.rules),
                              envs=args.envs, first_screen=args.first_screen, iterations=m, mean_return=round(float(ret.mean()), 4),
                              episodes=int(ret.size), train_seconds=round(train_s, 3))), flush=True)
    eng.close()


for head in args.heads:
    for n_step in args.n_step:
        for seed in args.seeds:
            run(seed, head, n_step)
