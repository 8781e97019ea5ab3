"""Throughput of the Q engine's Engine.iterate() with lambda-return targets (--side lambda: q_lambda = 0.8)
against the one-step engine (--side one-step: q_lambda unset, the path the engine had before), which runs the same
forwards and the same launches but for the target kernel (Sarsa: the one-step engine draws a_n inside its target
kernel, the lambda engine by a launch of its own), at DESIGN §4m's shape: Pong (6 actions, no lives), 256 envs,
the 16384-frame pool, the reference initialisers.  Warm-up iterations, then timed windows (host clock around
iterations that end in a device synchronise), in env-steps/s and ms per iteration.  One figure per process:

  python tools/q_lambda_throughput.py --overlap 1 --form q --side lambda
  python tools/q_lambda_throughput.py --sweep      every figure of §4m: overlap / sync x the forms q, double_q, sarsa,
                                                   three fresh processes per side, the two sides alternated
                                                   (one-step lambda one-step lambda ..)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--sweep', action='store_true')
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--overlap', type=int, default=1)
ap.add_argument('--form', choices=['q', 'double_q', 'sarsa'], default='q')
ap.add_argument('--side', choices=['lambda', 'one-step'], default='lambda')
ap.add_argument('--q_lambda', type=float, default=0.8)
ap.add_argument('--warmup', type=int, default=50)
ap.add_argument('--iters', type=int, default=None, help='iterations per window (default: 6400 / n_step)')
ap.add_argument('--windows', type=int, default=3)
ap.add_argument('--repeats', type=int, default=3, help='--sweep: fresh processes per figure')
args = ap.parse_args()

if args.sweep:
    for overlap in (1, 0):
        for form in ('q', 'double_q', 'sarsa'):
            for _ in range(args.repeats):
                for side in ('one-step', 'lambda'):
                    cmd = [sys.executable, os.path.abspath(__file__), '--envs', str(args.envs), '--n_step',
                           str(args.n_step), '--overlap', str(overlap), '--form', form, '--side', side,
                           '--q_lambda', str(args.q_lambda), '--warmup', str(args.warmup), '--windows', str(args.windows)]
                    if args.iters is not None:
                        cmd += ['--iters', str(args.iters)]
                    subprocess.run(cmd, check=True, timeout=300)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

import torch  # noqa: E402
from src.engine import Engine  # noqa: E402
from src.initializers import flatten_host, init_params  # noqa: E402
from src.kernels import param_names_shapes  # noqa: E402

A = 6
iters = args.iters or max(1, 6400 // args.n_step)
kw = {} if args.form == 'q' else {args.form: 1}
if args.side == 'lambda':                      # (unset: exactly the options an engine without it gets)
    kw['q_lambda'] = args.q_lambda
eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo='q', start_lives=0, num_frames=16384, seed=1,
             overlap=bool(args.overlap), **kw)
ns = param_names_shapes(A, 'q')
eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=1)))
for _ in range(args.warmup):
    eng.iterate()
torch.cuda.synchronize()
rates, ms = [], []
for _ in range(args.windows):
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.iterate()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rates.append(iters * args.n_step * args.envs / dt)
    ms.append(1e3 * dt / iters)
assert torch.isfinite(eng.params).all()
print(json.dumps(dict(side=args.side, form=args.form, q_lambda=eng.q_lambda, n_step=args.n_step, overlap=args.overlap,
                      envs=args.envs, iters=iters, env_steps_per_s=[round(r) for r in rates],
                      ms_per_iteration=[round(m, 4) for m in ms])), flush=True)
