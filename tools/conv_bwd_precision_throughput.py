"""Throughput of Engine.iterate() in the two compute modes of the nips conv backward, fp32 against bf16,
at the bench's shape: 6 actions, 3 lives, 256 envs, n = 5, the 16384-frame pool, the reference initialisers.  The
method is tools/lstm_precision_throughput.py's: one engine per pipeline (overlap, sync, then the LSTM head
overlapped), the modes alternating in one process, A B A B .., switched by Engine.set_conv_bwd_precision with warm-up
iterations after every switch; a timed window is blocks of 200 env steps per env (host clock around iterations that
end in a device synchronise) until 2 s have passed, and carries the kernel's live span inside the engine's iterations
(a3c_engine_span_stats).  After every engine's windows the kernel-alone time (a3c_engine_time_kernel, HIP events) in
both modes, alternated as well.  One JSON line per window and per kernel-alone pair, appended to
profiles/conv_bwd_precision_throughput.jsonl:

  python tools/conv_bwd_precision_throughput.py
  python tools/conv_bwd_precision_throughput.py --pipelines overlap --rounds 2"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--pipelines', default='overlap,sync,lstm', help='comma list of overlap, sync, lstm (overlapped LSTM head)')
ap.add_argument('--rounds', type=int, default=3, help='A B pairs per pipeline')
ap.add_argument('--warmup', type=int, default=30, help='iterations after every switch')
ap.add_argument('--seconds', type=float, default=2.0)
ap.add_argument('--kernel_iters', type=int, default=50)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_bwd_precision_throughput.jsonl'))
args = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

import torch  # noqa: E402
from src import _lib  # noqa: E402
from src.engine import Engine  # noqa: E402
from src.initializers import flatten_host, init_params  # noqa: E402
from src.kernels import param_names_shapes  # noqa: E402

A = 6
BLOCK = max(1, 200 // args.n_step)             # iterations per 200 steps
out = open(args.out, 'a')


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + '\n')
    out.flush()


def window(eng):
    eng.span_stats(0, reset=True)
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(BLOCK):
            eng.iterate()
        torch.cuda.synchronize()
        n += BLOCK
        dt = time.perf_counter() - t0
        if dt >= args.seconds:
            return n * args.n_step * args.envs / dt, 1e3 * dt / n, eng.span_stats(0)[0]


for pipe in args.pipelines.split(','):
    lstm, overlap = pipe == 'lstm', pipe != 'sync'
    eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo='a3c', start_lives=3, num_frames=16384,
                 seed=1, overlap=overlap, lstm=lstm)
    ns = param_names_shapes(A, 'a3c', lstm=lstm)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=1)))
    for _ in range(args.rounds):
        for mode in ('fp32', 'bf16'):
            eng.set_conv_bwd_precision(mode)
            for _ in range(args.warmup):
                eng.iterate()
            torch.cuda.synchronize()
            rate, ms, span = window(eng)
            emit(conv_bwd_precision=mode, pipeline=pipe, envs=args.envs, n_step=args.n_step, env_steps_per_s=round(rate),
                 ms_per_iteration=round(ms, 4), conv_bwd_live_span_us=round(span, 2))
    assert torch.isfinite(eng.params).all()
    for _ in range(args.rounds):                # the kernel alone, in the variant this pipeline launches
        us = {}
        for mode in ('fp32', 'bf16'):
            eng.set_conv_bwd_precision(mode)
            us[mode] = round(1e3 * eng.time_kernel(_lib.KER_CONV_BWD, args.kernel_iters), 2)
        emit(pipeline=pipe, conv_bwd_alone_us=us)
    eng.close()
