"""Throughput of Engine.iterate() in the two compute modes of the nips fc backward, fp32 against bf16, at
the bench's shape: 6 actions, 3 lives, 256 envs, n = 5, the 16384-frame pool, the reference initialisers.  The method
is tools/conv_bwd_precision_throughput.py's: one engine per pipeline (overlap, sync, then the LSTM head overlapped),
the modes alternating in one process, A B A B .., switched by Engine.set_fc_bwd_precision with warm-up iterations after
every switch; a timed window is blocks of 200 env steps per env (host clock around iterations that end in a device
synchronise) until 2 s have passed, and carries the conv backward's live span inside the engine's iterations.
--conv_bwd_precision sets the other backward switch of every engine (run the tool with fp32 and with bf16).  Then the
kernels alone at B = n * envs: k_fc_dw_bf and k_fc_dx_bf through a3c_fc_bwd_bf16 (one pass per call: the other's
outputs NULL) against the fp32 GEMMs the engine launches, through a3c_gemm_f32 (dW: wg_split 4, xcd 1; dX: the
MASKBITS epilogue), HIP events over --kernel_iters launches after a warm-up, the forms alternated.  One JSON line per
window and per kernel-alone round, appended to profiles/fc_bwd_precision_throughput.jsonl:

  python tools/fc_bwd_precision_throughput.py
  python tools/fc_bwd_precision_throughput.py --conv_bwd_precision bf16 --pipelines sync --rounds 2"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_step', type=int, default=5)
ap.add_argument('--pipelines', default='overlap,sync,lstm', help='comma list of overlap, sync, lstm (overlapped LSTM head); empty: none')
ap.add_argument('--conv_bwd_precision', default='fp32')
ap.add_argument('--rounds', type=int, default=3, help='A B pairs per pipeline')
ap.add_argument('--warmup', type=int, default=30, help='iterations after every switch')
ap.add_argument('--seconds', type=float, default=2.0)
ap.add_argument('--kernel_iters', type=int, default=50)
ap.add_argument('--kernel_rounds', type=int, default=5, help='0: no kernel-alone part')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fc_bwd_precision_throughput.jsonl'))
args = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, 'async-rl-tensorflow_amd'))

import torch  # noqa: E402
from src import _lib, kernels  # noqa: E402
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


for pipe in [p for p in args.pipelines.split(',') if p]:
    lstm, overlap = pipe == 'lstm', pipe != 'sync'
    eng = Engine(num_envs=args.envs, n_step=args.n_step, action_size=A, algo='a3c', start_lives=3, num_frames=16384,
                 seed=1, overlap=overlap, lstm=lstm, conv_bwd_precision=args.conv_bwd_precision)
    ns = param_names_shapes(A, 'a3c', lstm=lstm)
    eng.reset(flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=1)))
    for _ in range(args.rounds):
        for mode in ('fp32', 'bf16'):
            eng.set_fc_bwd_precision(mode)
            for _ in range(args.warmup):
                eng.iterate()
            torch.cuda.synchronize()
            rate, ms, span = window(eng)
            emit(fc_bwd_precision=mode, conv_bwd_precision=args.conv_bwd_precision, pipeline=pipe, envs=args.envs,
                 n_step=args.n_step, env_steps_per_s=round(rate), ms_per_iteration=round(ms, 4),
                 conv_bwd_live_span_us=round(span, 2))
    assert torch.isfinite(eng.params).all()
    eng.close()

if args.kernel_rounds:
    _lib.require_device()
    B = args.n_step * args.envs
    g = torch.Generator(device='cuda').manual_seed(1)
    l2 = torch.randn((B, 2592), device='cuda', generator=g).clamp_(min=0)
    dl3 = torch.randn((B, 256), device='cuda', generator=g)
    W = 0.08 * torch.randn((2592, 256), device='cuda', generator=g)
    pw = torch.bitwise_left_shift(torch.ones(32, dtype=torch.int64, device='cuda'), torch.arange(32, device='cuda'))
    bits = ((l2 > 0).view(B, 81, 32).to(torch.int64) * pw).sum(-1).to(torch.int32).contiguous()
    res = (torch.empty((2592, 256), device='cuda'), torch.empty(256, device='cuda'), torch.empty((B, 2592), device='cuda'))
    dW, colsum, dl2 = res
    d_dw = kernels.gemm_desc(l2, dl3, dW, 2592, 256, B, False, True, 2592, 256, 256, colsum=colsum, wg_split=4, xcd=1)
    d_dx = kernels.gemm_desc(dl3, W, dl2, B, 2592, 256, True, False, 256, 256, 2592, epi=_lib.GEMM_MASKBITS,
                             maskbits=bits, ldm=81)
    forms = dict(fp32_dw=lambda: kernels.gemm(d_dw), bf16_dw=lambda: kernels.fc_bwd_bf16(l2, dl3, W, out=(dW, colsum, None)),
                 fp32_dx=lambda: kernels.gemm(d_dx),
                 bf16_dx=lambda: kernels.fc_bwd_bf16(l2, dl3, W, maskbits=bits, out=(None, None, dl2)))

    def timed(f):
        for _ in range(10):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return round(1e3 * e0.elapsed_time(e1) / args.kernel_iters, 2)

    for _ in range(args.kernel_rounds):
        emit(B=B, kernel_iters=args.kernel_iters, alone_us={k: timed(f) for k, f in forms.items()})
