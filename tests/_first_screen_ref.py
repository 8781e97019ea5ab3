"""first_screen, restated on the CPU oracle.  Test infrastructure only (imported by
tests/test_first_screen_cpu.py and tests/test_gpu_first_screen.py).

The rule, as include/a3c_hip.h states it: when env e's act at rollout step t is terminal, ring slot
(tau + t + 1) % R of env e holds the screen of the new game's first state -- the frame the reset has
just put into the env state -- and the landing's screen is not written.  Nothing else changes.

FirstScreen is a mixin in front of any oracle.engine_ref.EngineRef subclass.  It does not copy
iterate(): for the length of one iterate() it wraps the oracle env's act (to count the rollout step)
and its new_random_game(mask) (to write the slot after the reset, over the landing screen iterate()
has just put there), then calls the class's own iterate().  out['frames'] reports the index of the
frame whose screen entered the ring, as the engine's per-step frame record does."""
import numpy as np

import _catch_memory_ref as M


class FirstScreen:
    def iterate(self, forced_actions=None, grads=True):
        env, step, shown = self.env, [-1], []
        act, new = env.act, env.new_random_game

        def counted_act(*a, **kw):
            step[0] += 1
            return act(*a, **kw)

        def shown_new_random_game(m=None):
            new(m)
            mask = np.ones(self.E, bool) if m is None else np.asarray(m, bool).copy()
            slot = (self.tau + step[0] + 1) % self.R
            for e in np.flatnonzero(mask):
                self.ring[e, slot] = self.screen_of(env.frame[e])
            shown.append((step[0], mask, env.frame.copy()))

        env.act, env.new_random_game = counted_act, shown_new_random_game
        try:
            out = super().iterate(forced_actions, grads)
        finally:
            del env.act, env.new_random_game          # (instance attributes: the class's methods are back)
        for t, mask, frame in shown:
            out['frames'][t][mask] = frame[mask]
        out['first_screens'] = [(t, mask) for t, mask, _ in shown]
        return out


def first_screen(base):
    """`base` (an EngineRef class) under the first_screen rule."""
    return type('FirstScreen' + base.__name__, (FirstScreen, base), {})


def with_rules(visible, frozen):
    """(Env, reference-loop EngineRef, first_screen EngineRef) under Catch rules (visible, frozen)."""
    env, ref = M.with_rules(visible, frozen)
    return env, ref, first_screen(ref)


FirstScreenMemoryEngineRef = first_screen(M.CatchMemoryEngineRef)       # CatchMemory-v0, rules (1, 4)
