"""Throughput of Engine.play at DESIGN §4e's shape: 256 envs, NIPS A3C, Pong, 16384-frame pool,
n_episode=1024, n_step=2000, poll_every=64; a warm-up call, then three timed calls (host clock
around the synchronous call), in live env-steps/s.  One figure per process:

  python tools/play_throughput.py                      waves mode
  python tools/play_throughput.py --refill             refill mode
  python tools/play_throughput.py --pkg <dir>          the package of another checkout (A/B against a
                                                       parent commit: its src/ and its lib/)
--calls 1 --no-warmup: one call only (under a profiler)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--refill', action='store_true')
ap.add_argument('--pkg', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              'async-rl-tensorflow_amd'))
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_episode', type=int, default=1024)
ap.add_argument('--n_step', type=int, default=2000)
ap.add_argument('--poll_every', type=int, default=64)
ap.add_argument('--calls', type=int, default=3)
ap.add_argument('--no-warmup', action='store_true')
ap.add_argument('--label', default=None)
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
from src.engine import Engine  # noqa: E402
from src.initializers import flatten_host, init_params  # noqa: E402
from src.kernels import param_names_shapes  # noqa: E402

A = 6
eng = Engine(num_envs=args.envs, n_step=5, action_size=A, algo='a3c', start_lives=0, num_frames=16384, seed=1)
ns = param_names_shapes(A, 'a3c')
eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=1, stddev=0.08)))
kw = dict(n_episode=args.n_episode, n_step=args.n_step, poll_every=args.poll_every)
if args.refill:
    kw['refill'] = True
if not args.no_warmup:
    eng.play(**kw)
rates, recs = [], []
for _ in range(args.calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.play(**kw)
    dt = time.perf_counter() - t0
    live = int(out['lengths'].sum())
    rates.append(live / dt)
    recs.append(dict(seconds=dt, live_env_steps=live, steps=out.get('steps')))
print(json.dumps(dict(label=args.label or ('refill' if args.refill else 'waves'), pkg=args.pkg, envs=args.envs,
                      n_episode=args.n_episode, n_step=args.n_step, poll_every=args.poll_every,
                      live_env_steps_per_s=rates, calls=recs)), flush=True)
