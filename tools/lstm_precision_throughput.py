"""Throughput of the LSTM engine's Engine.iterate() in its two lstm compute modes, fp32 against bf16, at
the bench's --lstm shape: 6 actions, 3 lives, 256 envs, n = 5, the 16384-frame pool, the reference initialisers.  The
method is tools/nat_precision_throughput.py's: one engine per pipeline (overlap, then sync), the modes alternating in
one process, A B A B .., switched by Engine.set_lstm_precision with warm-up iterations after every switch; a timed
window is blocks of 200 env steps per env (host clock around iterations that end in a device synchronise) until 2 s
have passed.  Then the kernel-alone times (a3c_engine_time_kernel, HIP events) of the three LSTM passes in both
modes.  One JSON line per window and per kernel table:

  python tools/lstm_precision_throughput.py
  python tools/lstm_precision_throughput.py --overlap 1 --rounds 2"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--overlap', type=int, default=None, help='1 / 0: that pipeline alone (default: both)')
ap.add_argument('--rounds', type=int, default=3, help='A B pairs per pipeline')
ap.add_argument('--warmup', type=int, default=30, help='iterations after every switch')
ap.add_argument('--seconds', type=float, default=2.0)
ap.add_argument('--kernel_iters', type=int, default=50)
args = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

import torch  # noqa: E402
from src import _lib  # noqa: E402
from src.engine import Engine  # noqa: E402
from src.initializers import flatten_host, init_params  # noqa: E402
from src.kernels import param_names_shapes  # noqa: E402

A = 6
BLOCK = max(1, 200 // args.n_step)             # iterations per 200 steps


def window(eng):
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(BLOCK):
            eng.iterate()
        torch.cuda.synchronize()
        n += BLOCK
        dt = time.perf_counter() - t0
        if dt >= args.seconds:
            return n * args.n_step * args.envs / dt, 1e3 * dt / n


for overlap in ((1, 0) if args.overlap is None else (args.overlap,)):
    eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo='a3c', start_lives=3, num_frames=16384,
                 seed=1, overlap=bool(overlap), lstm=True)
    ns = param_names_shapes(A, 'a3c', lstm=True)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=1)))
    for _ in range(args.rounds):
        for mode in ('fp32', 'bf16'):
            eng.set_lstm_precision(mode)
            for _ in range(args.warmup):
                eng.iterate()
            torch.cuda.synchronize()
            rate, ms = window(eng)
            print(json.dumps(dict(lstm_precision=mode, overlap=overlap, envs=args.envs, n_step=args.n_step,
                                  env_steps_per_s=round(rate), ms_per_iteration=round(ms, 4))), flush=True)
    assert torch.isfinite(eng.params).all()
    if not overlap or args.overlap is not None:    # kernels alone, on the last engine (an iteration has run in each mode)
        for mode in ('fp32', 'bf16'):
            eng.set_lstm_precision(mode)
            eng.iterate()
            eng.iterate()
            torch.cuda.synchronize()
            us = {k: round(1e3 * eng.time_kernel(v, args.kernel_iters), 2) for k, v in _lib.KER_LSTM.items()}
            print(json.dumps({'lstm_precision': mode, 'kernel_alone_us': us}), flush=True)
    eng.close()
