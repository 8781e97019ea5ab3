"""Slot utilisation (live slots / run slots) of Engine.play's two scheduling modes, on the CPU, from
the restatements' schedules (tests/_play_ref.py, tests/_play_refill_ref.py).  In the synthetic env
the terminals do not depend on the actions, so forward=False with zero actions gives the engine's
schedule; the screens are stubbed out (only the schedule is wanted).  Waves mode is charged the
steps the host runs: each wave up to the first poll at or behind its last live step.

  python tools/play_utilisation.py [--envs 256 --n_episode 1024 --n_step 2000 --poll_every 64 --calls 4]

`--calls`: consecutive play calls on one context, as tools/play_throughput.py makes them (a warm-up
and three timed ones); the emulators go on between calls, so each call has its own schedule."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from _play_ref import make_ref, play_ref  # noqa: E402
from _play_refill_ref import play_refill_ref, step_bound  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--n_episode', type=int, default=1024)
ap.add_argument('--n_step', type=int, default=2000)
ap.add_argument('--poll_every', type=int, default=64)
ap.add_argument('--calls', type=int, default=4)
ap.add_argument('--seed', type=int, default=1)
a = ap.parse_args()
E, N, S, P = a.envs, a.n_episode, a.n_step, a.poll_every


def polled(steps, cap):
    """Run steps the host issues when the last live step is `steps`: up to the next poll."""
    return min(cap, -(-steps // P) * P)


def fresh():
    ref = make_ref({}, E, 6, 'a3c', 0, frames=16384, seed=a.seed)
    ref.screen_of = lambda f: 0
    return ref


waves = -(-N // E)
wref, rref = fresh(), fresh()
for call in range(a.calls):
    w = play_ref(wref, N, S, forced_actions=np.zeros((waves, S, E), np.int32), forward=False)
    r = play_refill_ref(rref, N, S, forced_actions=np.zeros((step_bound(N, S, E), E), np.int32), forward=False)
    w_live = int(w['lengths'].sum())
    w_run = sum(polled(int(w['lengths'][i * E:(i + 1) * E].max()), S) for i in range(waves))
    r_live, r_run = int(r['lengths'].sum()), polled(r['steps'], step_bound(N, S, E))
    uw, ur = w_live / (w_run * E), r_live / (r_run * E)
    print(json.dumps(dict(call=call, waves=dict(live=w_live, run_steps=w_run, utilisation=round(uw, 4)),
                          refill=dict(live=r_live, run_steps=r_run, utilisation=round(ur, 4)),
                          expected_speedup=round(ur / uw, 4))), flush=True)
