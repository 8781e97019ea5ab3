"""Throughput of the Q engine's Engine.iterate() with Sarsa targets (--side sarsa) against double Q
(--side double_q), which runs the same forwards -- the slot's own parameters on s_n, then the target network --
and as many launches, at DESIGN §4i's shape: Pong (6 actions, no lives), 256 envs, the 16384-frame pool,
the reference initialisers.  Warm-up iterations, then timed windows (host clock around iterations that end in a
device synchronise), in env-steps/s and ms per iteration.  One figure per process:

  python tools/sarsa_throughput.py --n_step 5 --overlap 1 --side sarsa
  python tools/sarsa_throughput.py --n_step 5 --overlap 1 --side double_q --q_nstep 1
  python tools/sarsa_throughput.py --sweep      every figure of §4i: n in {5, 32} x overlap / sync x q_nstep
                                                0 / 1, three fresh processes per side, the two sides
                                                alternated (double_q sarsa double_q sarsa ..)
--side q is plain Q-learning (neither)."""
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
ap.add_argument('--q_nstep', type=int, default=0)
ap.add_argument('--side', choices=['sarsa', 'double_q', 'q'], default='sarsa')
ap.add_argument('--warmup', type=int, default=50)
ap.add_argument('--iters', type=int, default=None, help='iterations per window (default: 6400 / n_step)')
ap.add_argument('--windows', type=int, default=3)
ap.add_argument('--repeats', type=int, default=3, help='--sweep: fresh processes per figure')
args = ap.parse_args()

if args.sweep:
    for n in (5, 32):
        for overlap in (1, 0):
            for q_nstep in (0, 1):
                for _ in range(args.repeats):
                    for side in ('double_q', 'sarsa'):
                        cmd = [sys.executable, os.path.abspath(__file__), '--envs', str(args.envs), '--n_step', str(n),
                               '--overlap', str(overlap), '--q_nstep', str(q_nstep), '--side', side,
                               '--warmup', str(args.warmup), '--windows', str(args.windows)]
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
kw = dict(q_nstep=1) if args.q_nstep else {}      # (unset: exactly the options an engine without it gets)
if args.side != 'q':
    kw[args.side] = 1
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
print(json.dumps(dict(side=args.side, q_nstep=args.q_nstep, n_step=args.n_step, overlap=args.overlap,
                      envs=args.envs, iters=iters, env_steps_per_s=[round(r) for r in rates],
                      ms_per_iteration=[round(m, 4) for m in ms])), flush=True)
