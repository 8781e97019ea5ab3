"""Batched A3C / Q-learning actor-learner engine (one per GPU) over the C-ABI.

``Engine.iterate()`` is one pass of the rollout + gradient path for E envs: n env steps
(forward, action draw, env step, Atari preprocessing into the frame ring), bootstrap /
target-net forward, returns, loss + backward, per-tensor clip, then the optional multi-GPU
gradient exchange (``exchange`` callback, e.g. an RCCL all-reduce) and the RMSProp apply.
It replaces the per-worker loop of agent.py:52-67 (+ observe/batch_update :153-207) and the
parameter-server apply of main.py:60-66.

``overlap=True`` pipelines the engine: rollout k runs on an engine-owned stream with the
parameters after update k-2 while the backward, exchange and apply of rollout k-1 run on the
caller's stream (A3C's stale-parameter asynchrony at a fixed staleness of one update).  Rollout
k's buffers are ``slot(k & 1)``.  With ``algo='q'`` rollout k-1's TD targets are formed by its
backward, with the target network as it stands then (agent.py:169-190 at the same staleness).

Kernels are launched eagerly by default; ``use_graph=True`` captures each engine call into
hipGraphs and replays them (bit-identical, measured slower on MI355X: DESIGN.md §6).
``frame84=1`` (an engine option) feeds pre-sized 84x84 frames instead of raw RGB (measurement
mode M2).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .optim import check_adam

GAMES = {  # ALE minimal action sets / starting lives
    'Pong-v0': (6, 0),
    'Breakout-v0': (4, 5),
    'SpaceInvaders-v0': (6, 3),
    'Catch-v0': (3, 0),
    'CatchMemory-v0': (3, 0),
}
OPTIMIZERS = {'rmsprop': _lib.A3C_OPT_RMSPROP, 'adam': _lib.A3C_OPT_ADAM}
GAME_IDS = {'synth': _lib.A3C_GAME_SYNTH, 'catch': _lib.A3C_GAME_CATCH}
CATCH_FRAMES = 640


class _DevArray:
    """Zero-copy view of engine-owned device memory for torch.as_tensor."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {'data': (int(ptr), False), 'shape': tuple(int(s) for s in shape),
                                         'typestr': typestr, 'version': 2, 'strides': None}


def _view(ptr, shape, dtype):
    typestr = {torch.float32: '<f4', torch.int32: '<i4', torch.uint8: '|u1', torch.int64: '<i8',
               torch.uint32: '<u4'}[dtype]
    return torch.as_tensor(_DevArray(ptr, shape, typestr), device='cuda')


class Engine:
    def __init__(self, num_envs=256, n_step=5, action_size=6, algo='a3c', start_lives=0, num_frames=None,
                 seed=123, env_id_base=0, world_size=1, use_graph=False, overlap=False, lstm=False,
                 external_env=False, dqn_type='nips', game='synth', catch_rules=None, first_screen=None, q_lambda=None,
                 **overrides):
        """game: 'synth' (the synthetic Atari stand-in) or 'catch' (Catch-v0, DESIGN §4g: action_size 3,
        start_lives 0, device envs, raw RGB pool; random_start is ignored).  num_frames=None: 1024
        frames (Catch needs its 640: a smaller explicit value is rejected by the library).
        sarsa=0|1 (algo q): Sarsa targets, with q_nstep=1 n-step Sarsa; an option of
        a3c_engine_opts, not a field of the config.
        optimizer='rmsprop' | 'adam' (not given: RMSProp, and no call is made): Adam with TF1
        ApplyAdam semantics, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8 and the learning rate of
        the same schedule; ``mom`` is then m, ``ms`` is v and ``adam_powers`` the fp64 products beta1^t,
        beta2^t.  decay, momentum and epsilon are RMSProp's and ignored by Adam.
        catch_rules=None | (visible_rows, frozen_rows) (game 'catch'; None: Catch-v0's (10, 0),
        and no call is made): a3c_engine_set_catch_rules right after the create -- the ball is drawn in
        rows < visible_rows only, the paddle is frozen in the first frozen_rows steps; kept as
        ``catch_rules``.  environment.catch_rules_of(env_name) is the pair of a game's name.
        first_screen=None | False | True (game 'catch'; None: off, and no call is made):
        a3c_engine_set_first_screen right after the create -- at a terminal the training rollout writes
        the new game's first screen into the history where the reference loop (agent.py:59-67) writes
        the landing's, as Agent.play does (agent.py:366-367); kept as ``first_screen``.  Play ignores it.
        q_lambda=None | float in [0, 1] (algo q without q_nstep; None: the one-step rule, and no
        call is made): a3c_engine_set_q_lambda right after the create -- lambda-return targets over the
        rollout, Q(lambda), with double_q its double-Q form, with sarsa=1 Sarsa(lambda); 0 is the one-step
        target and 1 the n-step return; kept as ``q_lambda``.  Not in the saved state: a resumed run gives it
        again."""
        self.q_lambda = self._check_q_lambda(q_lambda, algo, overrides.get('q_nstep', 0))
        if first_screen is not None and game != 'catch':
            raise ValueError('first_screen is an option of game catch, not of %r' % (game,))
        self.first_screen = bool(first_screen)
        if catch_rules is not None:
            if game != 'catch':
                raise ValueError('catch_rules are the rules of game catch, not of %r' % (game,))
            v, f = (int(x) for x in catch_rules)
            if not (1 <= v <= 10 and 0 <= f <= 8):
                raise ValueError('catch_rules %r: visible_rows in 1..10, frozen_rows in 0..8' % (tuple(catch_rules),))
            catch_rules = (v, f)
        self.catch_rules = catch_rules
        optimizer = overrides.pop('optimizer', None)
        adam = check_adam(overrides.pop('adam_beta1', 0.9), overrides.pop('adam_beta2', 0.999),
                          overrides.pop('adam_epsilon', 1e-8))
        if optimizer is not None and optimizer not in OPTIMIZERS:
            raise ValueError('unknown optimizer %r (the engine knows %s)' % (optimizer, sorted(OPTIMIZERS)))
        self.optimizer = optimizer or 'rmsprop'
        _lib.require_device()
        if game not in GAME_IDS:
            raise ValueError('unknown game %r (the engine knows %s)' % (game, sorted(GAME_IDS)))
        self.game = game
        if num_frames is None:
            num_frames = max(1024, CATCH_FRAMES)
        if lstm and algo != 'a3c':
            raise ValueError('the LSTM head is an a3c head')
        self.dqn_type = str(dqn_type).lower()
        if self.dqn_type == 'nature' and (algo != 'a3c' or lstm or external_env):
            raise ValueError('the nature trunk (network.py:30-42) runs A3C heads, feed-forward, on device envs')
        cfg = _lib.EngineConfig()
        lib().a3c_engine_config_default(ctypes.byref(cfg))
        cfg.net = _lib.net_desc(action_size, algo, lstm, self.dqn_type)
        self.lstm = bool(lstm)
        cfg.num_envs = int(num_envs)
        cfg.n_step = int(n_step)
        cfg.start_lives = int(start_lives)
        cfg.num_frames = int(num_frames)
        cfg.seed = int(seed)
        cfg.env_id_base = int(env_id_base)
        cfg.world_size = int(world_size)
        cfg.use_graph = 1 if use_graph else 0
        cfg.overlap = 1 if overlap else 0
        cfg.external_env = 1 if external_env else 0
        self.overlap = bool(overlap)
        self.external_env = bool(external_env)
        # options of a3c_engine_opts (the config struct cannot grow): out before the config's fields
        opts = None
        if 'sarsa' in overrides:
            opts = _lib.EngineOpts()
            lib().a3c_engine_opts_default(ctypes.byref(opts))
            opts.game = GAME_IDS[game]
            opts.sarsa = int(overrides.pop('sarsa'))
        self.sarsa = bool(opts.sarsa) if opts is not None else False
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise ValueError(f'unknown engine option {k}')
            setattr(cfg, k, v)
        self.cfg = cfg
        self.algo = algo
        self.A = int(action_size)
        self.E, self.n = int(num_envs), int(n_step)
        h = ctypes.c_void_p()
        if opts is not None:
            check(lib().a3c_engine_create_opts(ctypes.byref(cfg), ctypes.byref(opts), ctypes.byref(h)),
                  'a3c_engine_create_opts')
        elif game == 'synth':
            check(lib().a3c_engine_create(ctypes.byref(cfg), ctypes.byref(h)), 'a3c_engine_create')
        else:
            check(lib().a3c_engine_create_ex(ctypes.byref(cfg), GAME_IDS[game], ctypes.byref(h)), 'a3c_engine_create_ex')
        self._h = h
        if optimizer is not None:
            check(lib().a3c_engine_set_optimizer(h, OPTIMIZERS[optimizer], *adam), 'a3c_engine_set_optimizer')
        if catch_rules is not None:
            check(lib().a3c_engine_set_catch_rules(h, *catch_rules), 'a3c_engine_set_catch_rules')
        if first_screen is not None:
            check(lib().a3c_engine_set_first_screen(h, int(bool(first_screen))), 'a3c_engine_set_first_screen')
        if self.q_lambda is not None:
            check(lib().a3c_engine_set_q_lambda(h, 1, self.q_lambda), 'a3c_engine_set_q_lambda')
        b = _lib.EngineBuffers()
        check(lib().a3c_engine_get_buffers(h, ctypes.byref(b)), 'a3c_engine_get_buffers')
        self._b = b
        self.zs = int(b.zs)
        self.offsets = [int(b.offsets[i]) for i in range(b.n_tensors)]
        self.sizes = [int(b.sizes[i]) for i in range(b.n_tensors)]
        P, E, n = int(b.n_params), self.E, self.n
        self.params = _view(b.params, (P,), torch.float32)
        self.target_params = _view(b.target_params, (P,), torch.float32)
        self.ms = _view(b.ms, (P,), torch.float32)
        self.mom = _view(b.mom, (P,), torch.float32)
        self.grads = _view(b.grads, (P,), torch.float32)
        self.frame_ring = _view(b.frame_ring, (E, b.ring_slots, 84, 84), torch.uint8)
        self.ring_slots = int(b.ring_slots)
        # [0] tau, [1] global step T (agent.py:165), [2] the workers' base step (agent.py:34,55)
        self.counters = _view(b.tau, (3,), torch.int64)
        self.loss = _view(b.loss, (4,), torch.float32)
        self.sched_ptr = int(b.sched)             # device [0] = lr of the last gradient
        self.sumsq = _view(b.sumsq, (b.n_tensors,), torch.float32)
        self._slots = [self._slot_views(k) for k in range(2 if self.overlap else 1)]
        for k, v in self._slots[0].items():
            setattr(self, k, v)
        self.frame84 = bool(cfg.frame84)
        self.frame_pool = _view(b.frame_pool, (int(cfg.num_frames),) + ((84, 84) if self.frame84 else (210, 160, 3)),
                                torch.uint8)
        # env state is double-buffered by step parity: the current state lives at tau & 1
        self._env = {'frame': _view(b.env_frame, (2, E), torch.int32),
                     'lives': _view(b.env_lives, (2, E), torch.int32),
                     'episode': _view(b.env_episode, (2, E), torch.int32),
                     'ep_step': _view(b.env_step, (2, E), torch.int32),
                     'ep_len': _view(b.env_len, (2, E), torch.int32)}

    def set_first_screen(self, on):
        """a3c_engine_set_first_screen between iterations: no reset, the next terminal follows it."""
        check(lib().a3c_engine_set_first_screen(self._h, int(bool(on))), 'a3c_engine_set_first_screen')
        self.first_screen = bool(on)

    @staticmethod
    def _check_q_lambda(value, algo, q_nstep):
        if value is None:
            return None
        value = float(value)
        if not 0.0 <= value <= 1.0:
            raise ValueError('q_lambda must be in [0, 1] (got %r)' % (value,))
        if algo != 'q':
            raise ValueError('q_lambda is a Q-learning option (algo %r; a3c has gae_lambda)' % (algo,))
        if q_nstep:
            raise ValueError('q_lambda with q_nstep: the n-step engine is lambda = 1 with the target forward of s_n alone')
        return value

    def set_q_lambda(self, value):
        """a3c_engine_set_q_lambda between iterations (None: back to the one-step rule): no reset, the next
        gradient follows it."""
        value = self._check_q_lambda(value, self.algo, self.cfg.q_nstep)
        check(lib().a3c_engine_set_q_lambda(self._h, int(value is not None), 0.0 if value is None else value),
              'a3c_engine_set_q_lambda')
        self.q_lambda = value

    def _slot_views(self, k):
        b = _lib.EngineBuffers()
        check(lib().a3c_engine_slot_buffers(self._h, k, ctypes.byref(b)), 'a3c_engine_slot_buffers')
        E, n = self.E, self.n
        lstm = {}
        if self.lstm:
            U = int(b.lstm_units)
            lstm = dict(lstm_h=_view(b.lstm_h, (n, E, U), torch.float32),
                        lstm_c=_view(b.lstm_c, (n, E, U), torch.float32),
                        lstm_hp=_view(b.lstm_hp, (n, E, U), torch.float32),
                        lstm_cp=_view(b.lstm_cp, (n, E, U), torch.float32),
                        lstm_gates=_view(b.lstm_gates, (n, E, 4 * U), torch.float32))
        if self.dqn_type == 'nature':     # conv outputs NHWC [20,20,32] / [9,9,64] / [7,7,64], fc out 512
            acts = dict(act_l1=_view(b.act_l1, (n * E, 12800), torch.float32),
                        act_l2=_view(b.act_l2, (n * E, 5184), torch.float32),
                        act_l3=_view(b.act_l3, (n * E, 3136), torch.float32),
                        act_l4=_view(b.act_l4, (n * E, 512), torch.float32))
        else:
            acts = dict(act_l1=_view(b.act_l1, (n * E, 6400), torch.float32),
                        act_l2=_view(b.act_l2, (n * E, 2592), torch.float32),
                        act_l3=_view(b.act_l3, (n * E, 256), torch.float32))
        sarsa = {}
        if self.sarsa:      # the action drawn for the bootstrap state s_n by the slot's last gradient
            p = ctypes.c_void_p()
            check(lib().a3c_engine_slot_boot_actions(self._h, k, ctypes.byref(p)), 'a3c_engine_slot_boot_actions')
            sarsa = dict(boot_actions=_view(p.value, (E,), torch.int32))
        return dict(**lstm, **acts, **sarsa, actions=_view(b.actions, (n, E), torch.int32),
                    rewards=_view(b.rewards, (n, E), torch.float32),
                    terminals=_view(b.terminals, (n, E), torch.uint8),
                    z=_view(b.z, (n + 1, E, self.zs), torch.float32),
                    returns=_view(b.returns, (n, E), torch.float32))

    def slot(self, k):
        """Rollout buffers of slot k (overlap: rollout i lives in slot i & 1)."""
        return self._slots[k]

    def env_field(self, name):
        """Current synthetic-env state field [E] (frame, lives, episode, ep_step, ep_len)."""
        tau = int(self.counters[0].item())
        return self._env[name][tau & 1]

    @property
    def env_frame(self):
        return self.env_field('frame')

    def close(self):
        if getattr(self, '_h', None):
            lib().a3c_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------------------------
    def reset(self, host_params=None):
        """host_params: flat float32 numpy array of the engine layout (None keeps params)."""
        arg = None
        if host_params is not None:
            hp = np.ascontiguousarray(np.asarray(host_params, dtype=np.float32))
            if hp.size != self.params.numel():
                raise ValueError('host_params has the wrong length')
            self._hp = hp
            arg = hp.ctypes.data_as(ctypes.c_void_p)
        check(lib().a3c_engine_reset(self._h, arg, _lib.stream_handle()), 'a3c_engine_reset')
        self._ext_began = False
        self._step0_w = 0

    def rollout_grad(self):
        check(lib().a3c_engine_rollout_grad(self._h, _lib.stream_handle()), 'a3c_engine_rollout_grad')

    def apply(self):
        check(lib().a3c_engine_apply(self._h, _lib.stream_handle()), 'a3c_engine_apply')

    @property
    def grad_ready(self):
        return bool(lib().a3c_engine_grad_ready(self._h))

    @property
    def split_point(self):
        """Split exchange (several GPUs): the float offset where the fc / head gradients start --
        clipped before the conv backward, so their exchange can run under it; 0: no split."""
        if not hasattr(lib(), 'a3c_engine_exchange_split'):
            return 0          # (an older build selected by A3C_LIB: the one-phase exchange, named on load)
        cut = _lib.c_i64()
        check(lib().a3c_engine_exchange_split(self._h, ctypes.byref(cut)), 'a3c_engine_exchange_split')
        return int(cut.value)

    def wait_grad_head(self):
        """The current stream waits until the last rollout_grad's grads[split_point:] are clipped."""
        check(lib().a3c_engine_wait_grad_head(self._h, _lib.stream_handle()), 'a3c_engine_wait_grad_head')

    def apply_shard(self, grads_by_rank, nranks, lo, n, w_out):
        """Partitioned PS step 1: nranks sequential RMSProp steps of [lo, lo+n) -> w_out."""
        check(lib().a3c_engine_apply_shard(self._h, _lib.ptr(grads_by_rank), int(nranks), int(lo), int(n),
                                           _lib.ptr(w_out), _lib.stream_handle()), 'a3c_engine_apply_shard')

    def apply_commit(self, params_src=None):
        """Partitioned PS step 2: params <- params_src, snapshot / target sync, counters."""
        check(lib().a3c_engine_apply_commit(self._h, _lib.ptr(params_src), _lib.stream_handle()),
              'a3c_engine_apply_commit')

    def iterate(self, exchange=None):
        """One iteration: rollout + gradient, [exchange(grads)], apply.  Single-GPU device-env
        engines without an exchange take the fused path (a3c_engine_iterate: the apply enqueued with
        the backward, bit-identical to rollout_grad() + apply()).  An exchange with
        ``owns_apply`` (src.distributed.PartitionedPS) performs the apply itself."""
        if exchange is None and self.cfg.world_size == 1 and not self.external_env:
            check(lib().a3c_engine_iterate(self._h, _lib.stream_handle()), 'a3c_engine_iterate')
            return
        self.rollout_grad()
        if not self.grad_ready:          # overlap pipeline filling: no gradient yet
            return
        if getattr(exchange, 'owns_apply', False):
            exchange.apply(self)
            return
        if exchange is not None:
            exchange(self.grads)
        self.apply()

    # ---------------------------------------------------------------- evaluation (agent.py:351-391)
    def play(self, n_episode=100, n_step=10000, test_ep=None, greedy=False, poll_every=64, trace=False, refill=False):
        """Agent.play (agent.py:351-391) batched: n_episode evaluation episodes of at most n_step
        env steps each, E at a time (episode w*E + e: env e in wave w), with the live parameters and
        no learning -- the training state is untouched.  The env steps with is_training=False (a
        lost life is no terminal and costs no -1, agent.py:373) and the returns are sums of raw
        rewards (agent.py:377).  test_ep: the fixed epsilon (q: None -> each env's final epsilon,
        main.py:68; a3c: used with greedy=True only); test_ep=0 is greedy.  Synchronous.
        Returns {'returns' f32, 'lengths' i32, 'terminated' bool [n_episode], 'best_reward',
        'best_idx' (agent.py:381-383)}; trace=True adds the device tensors 'actions'
        [waves, n_step, E] i32 and 'z' [waves, n_step, E, zs] f32, written by the steps' own
        kernels (entries of frozen envs and of steps not run stay as allocated: -1 / NaN).
        refill=True: no waves -- an env whose episode ends (terminal, or its own n_step steps) takes
        the next unassigned episode in the same step, in env-id order; the traces are then
        [waves*n_step, E(, zs)] indexed by run step.  Either way the result carries the schedule,
        'episode_env' i32 and 'episode_tau0' i64 [n_episode] (the env that played the episode and
        the tau of its first step), and 'steps', the run steps in which any env was live."""
        refill = int(refill)                     # (the library rejects anything but 0 / 1)
        cfg = _lib.PlayConfig()
        lib().a3c_play_config_default(ctypes.byref(cfg))
        cfg.n_episode, cfg.n_step, cfg.greedy = int(n_episode), int(n_step), 1 if greedy else 0
        cfg.test_ep = -1.0 if test_ep is None else float(test_ep)
        cfg.poll_every = int(poll_every)
        if test_ep is not None and float(test_ep) < 0:
            raise ValueError('test_ep must be >= 0 (None: the per-env final epsilon)')
        n_ep = max(cfg.n_episode, 1)
        ret = np.zeros(n_ep, np.float32)
        length = np.zeros(n_ep, np.int32)
        term = np.zeros(n_ep, np.uint8)
        acts = zt = None
        if trace and cfg.n_episode >= 1 and cfg.n_step >= 1:      # (else the call rejects the arguments)
            waves = -(-cfg.n_episode // self.E)
            shape = (waves * cfg.n_step, self.E) if refill else (waves, cfg.n_step, self.E)
            acts = torch.full(shape, -1, dtype=torch.int32, device='cuda')
            zt = torch.full(shape + (self.zs,), float('nan'), dtype=torch.float32, device='cuda')
        args = (ret.ctypes.data_as(ctypes.c_void_p), length.ctypes.data_as(ctypes.c_void_p),
                term.ctypes.data_as(ctypes.c_void_p), _lib.ptr(acts), _lib.ptr(zt), _lib.stream_handle())
        if refill:
            check(lib().a3c_engine_play_ex(self._h, ctypes.byref(cfg), refill, *args), 'a3c_engine_play_ex')
        else:
            check(lib().a3c_engine_play(self._h, ctypes.byref(cfg), *args), 'a3c_engine_play')
        ep_env = np.zeros(n_ep, np.int32)
        ep_tau0 = np.zeros(n_ep, np.int64)
        steps = _lib.c_i64(0)
        check(lib().a3c_engine_play_schedule(self._h, ep_env.ctypes.data_as(ctypes.c_void_p),
                                             ep_tau0.ctypes.data_as(ctypes.c_void_p), cfg.n_episode,
                                             ctypes.byref(steps)), 'a3c_engine_play_schedule')
        best_reward, best_idx = 0.0, 0                                   # agent.py:361
        for idx in range(cfg.n_episode):
            if ret[idx] > best_reward:                                   # agent.py:381-383
                best_reward, best_idx = float(ret[idx]), idx
        out = dict(returns=ret, lengths=length, terminated=term.astype(bool), best_reward=best_reward,
                   best_idx=best_idx, episode_env=ep_env, episode_tau0=ep_tau0, steps=int(steps.value))
        if trace:
            out.update(actions=acts, z=zt)
        return out

    def play_buffers(self):
        """Views of the play context (tests): ring [E, R_play, 84, 84], tau [1], env fields [2, E]
        (both parity copies equal), the last wave's returns / lengths / terminated [E], frozen [2, E],
        and lstm_h / lstm_c [2, E, U] with the LSTM head; of refill runs episode_idx [E] and sched [4]
        (the next unassigned index twice, episodes not finished, steps with a live env)."""
        b = _lib.PlayBuffers()
        check(lib().a3c_engine_play_buffers(self._h, ctypes.byref(b)), 'a3c_engine_play_buffers')
        E = self.E
        out = dict(ring=_view(b.frame_ring, (E, b.ring_slots, 84, 84), torch.uint8), ring_slots=int(b.ring_slots),
                   tau=_view(b.tau, (1,), torch.int64), frame=_view(b.env_frame, (2, E), torch.int32),
                   lives=_view(b.env_lives, (2, E), torch.int32), episode=_view(b.env_episode, (2, E), torch.int32),
                   ep_step=_view(b.env_step, (2, E), torch.int32), ep_len=_view(b.env_len, (2, E), torch.int32),
                   returns=_view(b.returns, (E,), torch.float32), lengths=_view(b.lengths, (E,), torch.int32),
                   terminated=_view(b.terminated, (E,), torch.uint8), frozen=_view(b.frozen, (2, E), torch.uint8),
                   episode_idx=_view(b.episode_idx, (E,), torch.int32), sched=_view(b.sched, (4,), torch.int32))
        if self.lstm:
            out.update(lstm_h=_view(b.lstm_h, (2, E, _lib.A3C_LSTM_UNITS), torch.float32),
                       lstm_c=_view(b.lstm_c, (2, E, _lib.A3C_LSTM_UNITS), torch.float32))
        return out

    # ---------------------------------------------------------------- summaries (agent.py:69-139)
    STATS = ('reward_sum', 'ep_reward_sum', 'ep_reward_max', 'ep_reward_min', 'games', 'loss_sum', 'q_sum',
             'updates', 'env_steps', 'policy_loss_sum', 'value_loss_sum', 'entropy_sum')

    def stats_accumulate(self):
        """Add the rollout whose gradient the last iterate() computed to the device aggregates."""
        check(lib().a3c_engine_stats_accumulate(self._h, _lib.stream_handle()), 'a3c_engine_stats_accumulate')

    def read_stats(self, reset=True):
        """train_with_summary's aggregates since the last read (agent.py:104-131) over this GPU's
        envs: avg reward per env-step, avg loss / q per update, episode max / min / avg reward,
        number of games."""
        out = (ctypes.c_double * 16)()
        check(lib().a3c_engine_stats_read(self._h, out, 1 if reset else 0, _lib.stream_handle()),
              'a3c_engine_stats_read')
        raw = dict(zip(self.STATS, list(out)[:len(self.STATS)]))
        games, upd, steps = raw['games'], raw['updates'], raw['env_steps']
        res = {'avg_reward': raw['reward_sum'] / steps if steps else 0.0,
               'avg_loss': raw['loss_sum'] / upd if upd else 0.0,
               'avg_q': raw['q_sum'] / upd if upd else 0.0,
               # agent.py:110-115: 0 when no episode finished in the interval
               'avg_ep_reward': raw['ep_reward_sum'] / games if games else 0.0,
               'max_ep_reward': raw['ep_reward_max'] if games else 0.0,
               'min_ep_reward': raw['ep_reward_min'] if games else 0.0,
               'num_game': int(games), 'updates': int(upd), 'env_steps': int(steps)}
        if self.algo == 'a3c' and upd:
            res.update(avg_policy_loss=raw['policy_loss_sum'] / upd, avg_value_loss=raw['value_loss_sum'] / upd,
                       avg_entropy=raw['entropy_sum'] / upd)
        return res

    # ---------------------------------------------------------------- checkpoint / resume
    @property
    def worker_step(self):
        """agent.py:55's loop counter (the lr / epsilon schedules' step) at the next rollout.
        Host-stepped engines before their first rollout: the device counters are written by
        ext_begin, so the step is the one set_step restored (0 on a fresh run)."""
        if self.external_env and not getattr(self, '_ext_began', False):
            return int(getattr(self, '_step0_w', 0))
        c = self.counters.cpu()
        return int(c[2]) + int(c[0]) - 3

    def set_step(self, global_step, worker_step=None):
        """Resume from parameters + step (the reference's Saver, agent.py:29): the global step and
        the workers' loop counter restart there (agent.py:34,46)."""
        w = global_step if worker_step is None else worker_step
        self._step0_w = int(w)
        check(lib().a3c_engine_set_step(self._h, int(global_step), int(w), _lib.stream_handle()),
              'a3c_engine_set_step')

    def save_state(self):
        """The whole engine state as a host u8 array (parameters, RMSProp slots, counters, envs,
        frame ring, LSTM carry, the overlap pipeline's rollout in flight)."""
        nb = _lib.c_i64()
        check(lib().a3c_engine_state_bytes(self._h, ctypes.byref(nb)), 'a3c_engine_state_bytes')
        buf = np.empty(int(nb.value), np.uint8)
        check(lib().a3c_engine_state_save(self._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                          _lib.stream_handle()), 'a3c_engine_state_save')
        return buf

    def load_state(self, buf):
        """Restore save_state()'s array into this (reset) engine of the same configuration; the
        next iteration continues the saved run bit for bit."""
        buf = np.ascontiguousarray(np.asarray(buf, np.uint8))
        check(lib().a3c_engine_state_load(self._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                          _lib.stream_handle()), 'a3c_engine_state_load')

    @property
    def adam_powers(self):
        """(beta1^t, beta2^t) of the t Adam steps applied so far: the engine's fp64 device state, read
        behind the work on the current stream; (1.0, 1.0) for RMSProp."""
        p1, p2 = _lib.c_double(), _lib.c_double()
        check(lib().a3c_engine_adam_powers(self._h, ctypes.byref(p1), ctypes.byref(p2), _lib.stream_handle()),
              'a3c_engine_adam_powers')
        return float(p1.value), float(p2.value)

    @adam_powers.setter
    def adam_powers(self, powers):
        """Resume: the products a checkpoint stored (Adam engines, no gradient pending)."""
        check(lib().a3c_engine_set_adam_powers(self._h, float(powers[0]), float(powers[1]), _lib.stream_handle()),
              'a3c_engine_set_adam_powers')

    def advance(self):
        check(lib().a3c_engine_advance(self._h, _lib.stream_handle()), 'a3c_engine_advance')

    def iterate_hogwild(self, ps):
        """Rollout + gradient, unlocked push of the (per-worker clipped) gradient into the
        sharded Hogwild parameter server, pull of the shared parameters (src/hogwild.py).

        Overlap engine (the default of bench.py / main.py --update hogwild): rollout k runs on the
        engine's rollout stream while the caller's stream back-propagates rollout k-1, pushes its
        clipped gradient into every shard and pulls the shards into the parameter snapshot of
        rollout k+1 -- the push and pull overlap the next rollout, at staleness 1 like the overlap
        mode (the reference's workers keep acting while the PS applies, main.py:60-65).  Rollout
        k+1 is enqueued behind that pull (the engine orders its rollout stream after the caller's)."""
        if self.optimizer == 'adam':
            raise ValueError('Hogwild applies RMSProp in its lock-free shards, which keep no shared step count for '
                             "Adam's bias correction (DESIGN §4j): use iterate()")
        self.rollout_grad()
        if not self.grad_ready:
            return                      # overlap pipeline filling: no gradient yet
        if self.cfg.world_size == 1:
            # one worker: the engine fuses its clip into apply, which hogwild bypasses
            if not hasattr(self, '_clip_ws'):
                b = _lib.c_i64()
                check(lib().a3c_optim_workspace_bytes(self.params.numel(), ctypes.byref(b)), 'ws')
                self._clip_ws = torch.empty(int(b.value), dtype=torch.uint8, device='cuda')
            check(lib().a3c_clip_grads(_lib.ptr(self.grads), len(self.offsets), _lib.i64_array(self.offsets),
                                       _lib.i64_array(self.sizes), float(self.cfg.clip_norm), None,
                                       _lib.ptr(self._clip_ws), _lib.stream_handle()), 'a3c_clip_grads')
        ps.push(self.grads, lr_dev=self.sched_ptr)
        # counters, the overlap snapshot, and for q the target copy of the pulled (global) weights
        # when the global step crossed a multiple of target_q_update_step (agent.py:166-167, 342-344)
        if ps.world == 1:
            self.apply_commit(ps.params_view())     # the one shard is the whole vector: pull = commit
        else:
            ps.pull(self.params)
            self.apply_commit(None)

    # ---------------------------------------------------------------- host-stepped envs
    def ext_begin(self, rgb):
        """external_env: first frames [E,210,160,3] u8 (pinned host or device) -> every history slot."""
        self._ext_check(rgb, torch.uint8, (self.E, 210, 160, 3), 'rgb')
        check(lib().a3c_engine_ext_begin(self._h, _lib.ptr(rgb), _lib.stream_handle()), 'a3c_engine_ext_begin')

    def ext_act(self, actions_out):
        """external_env: forward + draw of the next rollout step; actions -> actions_out [E] int32
        (pinned host: valid after the stream synchronises)."""
        self._ext_check(actions_out, torch.int32, (self.E,), 'actions_out')
        check(lib().a3c_engine_ext_act(self._h, _lib.ptr(actions_out), _lib.stream_handle()), 'a3c_engine_ext_act')

    def ext_upload(self, rgb, env_lo, env_hi):
        """external_env: the post-act frames of envs [env_lo, env_hi) only (rgb stays the full
        [E,210,160,3] buffer); finish the step with ext_observe(None, rewards, terminals)."""
        self._ext_check(rgb, torch.uint8, (self.E, 210, 160, 3), 'rgb')
        check(lib().a3c_engine_ext_upload(self._h, _lib.ptr(rgb), int(env_lo), int(env_hi), _lib.stream_handle()),
              'a3c_engine_ext_upload')

    def ext_observe(self, rgb, rewards, terminals):
        """external_env: the step's post-act frames (None: sent by ext_upload), rewards and
        terminals of every env."""
        if rgb is not None:
            self._ext_check(rgb, torch.uint8, (self.E, 210, 160, 3), 'rgb')
        self._ext_check(rewards, torch.float32, (self.E,), 'rewards')
        self._ext_check(terminals, torch.uint8, (self.E,), 'terminals')
        check(lib().a3c_engine_ext_observe(self._h, _lib.ptr(rgb), _lib.ptr(rewards), _lib.ptr(terminals),
                                           _lib.stream_handle()), 'a3c_engine_ext_observe')

    def _ext_check(self, t, dtype, shape, name):
        if not self.external_env:
            raise ValueError('engine was not created with external_env=True')
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {shape}')
        if not t.is_cuda and not t.is_pinned():
            raise ValueError(f'{name}: host buffers must be pinned (async copies)')

    def begin_host(self, pool):
        """New random games of every host env; their first screens fill the history (ext_begin)."""
        self.ext_begin(pool.begin())
        self._ext_began = True
        self._ext_actions = torch.zeros(self.E, dtype=torch.int32).pin_memory()

    def rollout_host(self, pool):
        """The n env steps of one iteration with host-stepped envs (src/host_env.HostEnvPool): per
        rollout step the GPU draws the actions, the host steps every env, the post-act frames go
        back to the GPU for Environment.screen + History.add.  Finish with rollout_grad()."""
        if not getattr(self, '_ext_began', False):
            self.begin_host(pool)
        stream = torch.cuda.current_stream()
        # pools that step env ranges (SyntheticHostEnvPool) are stepped in `upload_chunks` ranges:
        # the H2D copy of one range runs while the host steps the next
        chunks = max(1, min(int(getattr(pool, 'upload_chunks', 1)), self.E)) if hasattr(pool, 'step_range') else 1
        bounds = [self.E * c // chunks for c in range(chunks + 1)]
        for _ in range(self.n):
            self.ext_act(self._ext_actions)
            stream.synchronize()            # actions on the host; the previous H2D copies are done
            acts = self._ext_actions.numpy()
            if chunks == 1:
                pool.step(acts)
                self.ext_observe(pool.rgb, pool.rewards, pool.terminals)
                continue
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                pool.step_range(acts, lo, hi)
                self.ext_upload(pool.rgb, lo, hi)
            self.ext_observe(None, pool.rewards, pool.terminals)

    def iterate_host(self, pool, exchange=None):
        """One iteration with host-stepped envs: rollout_host, then loss, backward, exchange, apply."""
        self.rollout_host(pool)
        self.rollout_grad()
        if getattr(exchange, 'owns_apply', False):
            exchange.apply(self)
            return
        if exchange is not None:
            exchange(self.grads)
        self.apply()

    def span_stats(self, which, reset=False):
        """Live launch spans recorded by the kernels themselves (which 0: k_conv_bwd, 1:
        k_head_screen_conv12): reset=True clears; else (avg_us, max_us, launches)."""
        avg, mx, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        check(lib().a3c_engine_span_stats(self._h, int(which), 1 if reset else 0, ctypes.byref(avg),
                                          ctypes.byref(mx), ctypes.byref(cnt)), 'a3c_engine_span_stats')
        return float(avg.value), float(mx.value), int(cnt.value)

    def span_steps(self):
        """k_head_screen_conv12's live spans split by rollout step: ([avg_us] * n, [launches] * n)."""
        avg = (ctypes.c_double * self.n)()
        cnt = (ctypes.c_int64 * self.n)()
        check(lib().a3c_engine_span_steps(self._h, avg, cnt), 'a3c_engine_span_steps')
        return [round(float(a), 2) for a in avg], [int(c) for c in cnt]

    def time_kernel(self, kernel, iters=20):
        """Average device ms of one engine kernel (HIP events on the current stream)."""
        out = ctypes.c_float()
        check(lib().a3c_engine_time_kernel(self._h, int(kernel), int(iters), _lib.stream_handle(),
                                           ctypes.byref(out)), 'a3c_engine_time_kernel')
        return float(out.value)

    @property
    def env_steps_per_iteration(self):
        return self.E * self.n
