"""What the Q engine learns on Catch with lambda-return targets (q_lambda; with sarsa = 1 Sarsa(lambda)) and,
beside them, with the one-step and the n-step rules it lies between, at equal env-steps: DESIGN §4m's table.
The overlapped engine, 256 envs, the reference initialisers, learn_start = 0; after 0, 64, 128, .. iterations
(powers of two) the mean return of 1024 greedy episodes (Engine.play, refill, test_ep = 0), which leaves the
training state untouched.

  python tools/q_lambda_learning.py                                   seeds 1 2 3, Q and Sarsa, every column
  python tools/q_lambda_learning.py --seeds 1 --sarsa 1 --rules 0.8   one run

A rule is a lambda in [0, 1], 'one-step' (q_lambda unset: the parent path) or 'n-step' (q_nstep = 1).  The
settings are arguments so that the table states them; their defaults are the ones §4h's tests use."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
ap.add_argument('--sarsa', type=int, nargs='+', default=[0, 1])
ap.add_argument('--rules', nargs='+', default=['one-step', '0', '0.5', '0.8', '0.95', '1', 'n-step'])
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--max_iters', type=int, default=8192)
ap.add_argument('--learning_rate', type=float, default=2e-2)
ap.add_argument('--epsilon', type=float, default=0.1, help='RMSProp epsilon')
ap.add_argument('--ep_end_t', type=int, default=1000, help='env steps per env over which epsilon anneals')
ap.add_argument('--target_q_update_step', type=int, default=12800, help='global env steps between target syncs')
args = ap.parse_args()

import torch  # noqa: E402
import main  # noqa: E402
from src.engine import Engine  # noqa: E402

A, FRAMES = 3, 640


def run(seed, sarsa, rule):
    kw = dict(sarsa=1) if sarsa else {}
    if rule == 'n-step':
        kw['q_nstep'] = 1
    elif rule != 'one-step':
        kw['q_lambda'] = float(rule)
    eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo='q', overlap=True, seed=seed,
                 num_frames=FRAMES, game='catch', learn_start=0, ep_end_t=args.ep_end_t,
                 target_q_update_step=args.target_q_update_step, learning_rate=args.learning_rate,
                 epsilon=args.epsilon, **kw)
    eng.reset(main.initial_params(eng, A, 'q', seed))
    eng.target_params.copy_(eng.params)
    eng.reset()                                   # keeps the parameters, re-takes the pipeline snapshots
    done, marks, table, train_s = 0, [0] + [2 ** k for k in range(9, 32) if 2 ** k <= args.max_iters], {}, 0.0
    for m in marks:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while done < m:
            eng.iterate()
            done += 1
        torch.cuda.synchronize()
        train_s += time.perf_counter() - t0
        out = eng.play(n_episode=1024, n_step=50, refill=True, test_ep=0.0)
        table[m] = round(float(out['returns'].mean()), 4)
    print(json.dumps(dict(seed=seed, sarsa=sarsa, rule=rule, envs=args.envs, n_step=args.n_step,
                          learning_rate=args.learning_rate, epsilon=args.epsilon, ep_end_t=args.ep_end_t,
                          target_q_update_step=args.target_q_update_step, mean_greedy_return=table,
                          train_seconds=round(train_s, 3))), flush=True)
    eng.close()


for sarsa in args.sarsa:
    for rule in args.rules:
        for seed in args.seeds:
            run(seed, sarsa, rule)
