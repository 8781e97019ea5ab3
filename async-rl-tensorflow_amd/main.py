"""main.py:1-98 on MI355X.  Same flags; ``--job_name``/``--ps_hosts``/``--worker_hosts`` are
accepted but the TF ps/worker cluster is replaced by one process per GPU under torchrun
(torch.distributed, backend nccl = RCCL), see src/distributed.py.

  --mode agent   the reference's per-step Q-learning Agent loop (agent.py:52-139), one env per
                 process, drop-in API (src/agent.py);
  --mode engine  the batched MI355X actor-learner (num_envs envs per GPU, n-step rollout +
                 gradient + exchange + RMSProp per iteration, src/engine.py).

  python main.py --mode engine --env_name Pong-v0 --iterations 1000
  python main.py --mode engine --env_name Catch-v0 --iterations 1000   the learnable device game
  python main.py --mode engine --algo q --q_nstep true --n_step 5 --env_name Catch-v0   n-step Q-learning
  python main.py --mode engine --algo q --sarsa true --n_step 5 --env_name Catch-v0     Sarsa (--q_nstep true: n-step)
  python main.py --mode engine --algo q --q_lambda 0.8 --n_step 5 --env_name Catch-v0    lambda-return targets: Q(lambda), with
                 --sarsa true Sarsa(lambda), with --double_q true its double-Q form
  python main.py --mode engine --algo q --optimizer adam --env_name Catch-v0             shared Adam instead of RMSProp
  python main.py --mode engine --lstm true --env_name CatchMemory-v0   Catch that only a head with memory learns
  python main.py --mode engine --lstm true --env_name CatchMemory-v0 --first_screen true   ... with each episode's first
                 screen shown to the training rollouts, without which it is not learned
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py --mode engine
  python main.py --mode engine --is_train false --n_episode 100     evaluate the newest checkpoint
  python main.py --mode engine --is_train false --play_refill true  ... refilling finished envs (no waves)
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np    # noqa: E402
import torch          # noqa: E402


def str2bool(v):
  return str(v).lower() in ('1', 'true', 'yes', 'y', 't')


def parse_flags(argv=None):
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  # Model
  p.add_argument('--model', default='m1')
  p.add_argument('--dueling', type=str2bool, default=False)
  p.add_argument('--double_q', type=str2bool, default=False)
  # Environment
  p.add_argument('--env_name', default='Breakout-v0')
  p.add_argument('--action_repeat', type=int, default=1)
  # Optimizer
  p.add_argument('--decay', type=float, default=0.99)
  p.add_argument('--epsilon', type=float, default=0.1)
  p.add_argument('--momentum', type=float, default=0.0)
  p.add_argument('--beta', type=float, default=0.01)
  p.add_argument('--optimizer', choices=['rmsprop', 'adam'], default='rmsprop',
                 help='the shared optimizer of --mode engine and --mode agent: rmsprop (the reference: TF ApplyRMSProp '
                      'with --decay, --momentum, --epsilon) or adam (TF1 ApplyAdam with --adam_beta1, --adam_beta2, '
                      '--adam_epsilon on the same learning-rate schedule; --decay, --momentum and --epsilon are '
                      "RMSProp's and ignored by it; not with --update hogwild; DESIGN §4j)")
  p.add_argument('--adam_beta1', type=float, default=0.9, help='--optimizer adam: beta1, in [0, 1)')
  p.add_argument('--adam_beta2', type=float, default=0.999, help='--optimizer adam: beta2, in [0, 1)')
  p.add_argument('--adam_epsilon', type=float, default=1e-8,
                 help='--optimizer adam: epsilon, > 0, added to sqrt(v) as TF does')
  # Distributed (accepted for compatibility; torchrun provides RANK/WORLD_SIZE)
  p.add_argument('--ps_hosts', default='0.0.0.0:2222')
  p.add_argument('--worker_hosts', default='0.0.0.0:2223,0.0.0.0:2224')
  p.add_argument('--job_name', default='')
  p.add_argument('--task_index', type=int, default=0)
  # Misc
  p.add_argument('--gpu_fraction', default='1/1')
  p.add_argument('--display', type=str2bool, default=False)
  p.add_argument('--is_train', type=str2bool, default=True)
  p.add_argument('--random_seed', type=int, default=123)
  # MI355X engine
  p.add_argument('--mode', choices=['agent', 'engine'], default='engine')
  p.add_argument('--algo', choices=['a3c', 'q'], default='a3c')
  p.add_argument('--n_step', type=int, default=5)
  p.add_argument('--gae_lambda', type=float, default=1.0,
                 help='engine mode, a3c: GAE(lambda) advantages and lambda-returns; 1 = the n-step return (DESIGN §4f)')
  p.add_argument('--q_nstep', type=str2bool, default=False,
                 help='engine mode, q: asynchronous n-step Q-learning (Algorithm S2) -- the target of every step of '
                      'the rollout is its n-step return, bootstrapped from the target network on s_n (DESIGN §4h)')
  p.add_argument('--sarsa', type=str2bool, default=False,
                 help='engine mode, q: asynchronous Sarsa -- the target takes the target network at the action the '
                      'behaviour policy takes in the next state, not at the maximum; with --q_nstep true n-step Sarsa '
                      '(DESIGN §4i)')
  p.add_argument('--q_lambda', type=float, default=None,
                 help='engine mode, q: lambda-return targets over the rollout (Q(lambda); with --sarsa Sarsa(lambda), '
                      'with --double_q its double-Q form) -- 0 is the one-step target, 1 the n-step return of '
                      '--q_nstep true; unset: the one-step / n-step rules as they are (DESIGN §4m)')
  p.add_argument('--num_envs', type=int, default=256)
  p.add_argument('--num_frames', type=int, default=16384)
  p.add_argument('--iterations', type=int, default=1000)
  p.add_argument('--envs_on', choices=['device', 'host', 'gym'], default='device',
                 help='engine mode: envs stepped on the GPU (synthetic), on host threads (C++ synthetic '
                      'emulator, frames over PCIe), or gym/ALE envs on the host (AtariEnv, needs gym)')
  p.add_argument('--host_threads', type=int, default=16)
  p.add_argument('--max_step', type=int, default=None)
  p.add_argument('--log_every', type=int, default=None,
                 help='engine mode: iterations between summaries (default: test_step env-steps per env, '
                      'agent.py:104)')
  p.add_argument('--save_model_secs', type=int, default=600, help='checkpoint period (main.py:80)')
  p.add_argument('--max_to_keep', type=int, default=30, help='checkpoints kept (agent.py:29)')
  p.add_argument('--checkpoint_dir', default=None, help='default: <logdir>/<model_dir> (main.py:75)')
  p.add_argument('--resume', type=str2bool, default=True,
                 help='restore the newest checkpoint of checkpoint_dir, as managed_session does (main.py:90)')
  p.add_argument('--update', choices=['overlap', 'sync', 'hogwild'], default='overlap',
                 help='engine mode: stale-1 overlapped A3C, synchronous exchange, or Hogwild sharded PS')
  p.add_argument('--exchange', choices=['sequential', 'sum'], default='sequential',
                 help='multi-GPU sync/overlap exchange: sequential = partitioned PS applying every '
                      "worker's clipped gradient as its own RMSProp step in rank order (the reference "
                      'PS semantics); sum = one all-reduce, one RMSProp step of the summed gradients')
  p.add_argument('--lstm', type=str2bool, default=False,
                 help='engine mode, a3c: the 256-cell LSTM policy head (BASELINE config 5, DESIGN §4b)')
  p.add_argument('--first_screen', type=str2bool, default=False,
                 help='engine mode, Catch-v0 / CatchMemory-v0 on the device: at a terminal the training rollout adds '
                      "the new game's first screen to the history (as play does, agent.py:366-367) where the "
                      "reference loop (agent.py:59-67) adds the landing's; play ignores it (DESIGN §4l)")
  p.add_argument('--dqn_type', choices=['nips', 'nature'], default='nips',
                 help="conv trunk of network.py:30-50 (Network(DQN_type=...)): nips (fused kernels) or nature "
                      "(implicit-GEMM kernels, nature.hip; --algo a3c)")
  # evaluation: --mode engine --is_train false (Agent.play, agent.py:351-391)
  p.add_argument('--n_episode', type=int, default=100, help='play: episodes (agent.py:351)')
  p.add_argument('--play_steps', type=int, default=10000, help="play: cap on an episode's env steps (agent.py:351 n_step)")
  p.add_argument('--test_ep', type=float, default=None,
                 help='play: the fixed epsilon (agent.py:351); default: q -- each env\'s final epsilon (main.py:68), '
                      'a3c -- the categorical draw, or greedy with --greedy')
  p.add_argument('--greedy', action='store_true', help='play, a3c: argmax (epsilon-greedy with --test_ep) on the logits')
  p.add_argument('--play_refill', type=str2bool, default=False,
                 help='play: an env whose episode ends takes the next episode at once (no waves; DESIGN §4e)')
  p.add_argument('--logdir', default='./logs')
  return p.parse_args(argv)


def engine_options(flags):
  """The reference options of --mode engine: each one either reaches the Engine or is rejected,
  so no option is silently dropped (agent.py:176-184 double-Q, :234-249 dueling, network.py:30-42
  nature trunk).  Returns the Engine keyword arguments the flags select."""
  if flags.dueling:
    raise ValueError('--dueling (agent.py:234-249) is not fused into the engine: use --mode agent')
  from src.environment import game_kind
  if game_kind(flags.env_name) == 'catch' and flags.envs_on != 'device':
    raise ValueError('--env_name %s is a device game: --envs_on %s is not supported (the host-thread '
                     'emulator and gym know the Atari games only)' % (flags.env_name, flags.envs_on))
  if flags.dqn_type == 'nature' and (flags.algo != 'a3c' or flags.lstm):
    raise ValueError('--dqn_type nature: the A3C Network trunk (network.py:30-42) runs with --algo a3c and the '
                     'feed-forward head (the Q-net of agent.py:226-252 is nips only)')
  if flags.double_q and flags.algo != 'q':
    raise ValueError('--double_q is a Q-learning option (agent.py:176-184): use it with --algo q')
  if flags.lstm and flags.algo != 'a3c':
    raise ValueError('--lstm is an A3C policy head: use it with --algo a3c')
  if not 0.0 <= flags.gae_lambda <= 1.0:
    raise ValueError('--gae_lambda must be in [0, 1] (got %r)' % flags.gae_lambda)
  if flags.gae_lambda != 1.0 and flags.algo != 'a3c':
    raise ValueError('--gae_lambda is an A3C option (algo q has one-step TD targets): use it with --algo a3c')
  if flags.q_nstep and flags.algo != 'q':
    raise ValueError('--q_nstep is a Q-learning option (n-step targets, DESIGN §4h): use it with --algo q')
  if flags.sarsa and flags.algo != 'q':
    raise ValueError('--sarsa is a Q-learning option (its target is a Q value, DESIGN §4i): use it with --algo q')
  if flags.sarsa and flags.double_q:
    raise ValueError('--sarsa with --double_q: double Q picks the argmax, Sarsa the taken action (DESIGN §4i)')
  q_lambda = getattr(flags, 'q_lambda', None)
  if q_lambda is not None:
    if not 0.0 <= q_lambda <= 1.0:
      raise ValueError('--q_lambda must be in [0, 1] (got %r)' % q_lambda)
    if flags.algo != 'q':
      raise ValueError('--q_lambda is a Q-learning option (lambda-return Q targets, DESIGN §4m; algo a3c has '
                       '--gae_lambda): use it with --algo q')
    if flags.q_nstep:
      raise ValueError('--q_lambda with --q_nstep: the n-step engine is lambda = 1 with the target forward of s_n '
                       'alone (DESIGN §4m); give one of them')
  first_screen = bool(getattr(flags, 'first_screen', False))
  if first_screen and game_kind(flags.env_name) != 'catch':
    raise ValueError('--first_screen is an option of the device game Catch (--env_name Catch-v0 or CatchMemory-v0, '
                     "DESIGN §4l): %s's frames are hashed, and host or gym envs are not covered" % flags.env_name)
  if first_screen and flags.envs_on != 'device':
    raise ValueError('--first_screen needs --envs_on device (got %s)' % flags.envs_on)
  adam = adam_options(flags)
  if adam and flags.update == 'hogwild':
    raise ValueError('--optimizer adam with --update hogwild: the lock-free shards keep no shared step count for '
                     "Adam's bias correction (DESIGN §4j): use --update overlap or sync")
  kw = dict(lstm=bool(flags.lstm), **adam)
  if flags.gae_lambda != 1.0:
    kw['gae_lambda'] = float(flags.gae_lambda)
  if flags.double_q:
    kw['double_q'] = True
  if flags.q_nstep:
    kw['q_nstep'] = 1
  if flags.sarsa:
    kw['sarsa'] = 1
  if q_lambda is not None:
    kw['q_lambda'] = float(q_lambda)
  if flags.dqn_type == 'nature':
    kw['dqn_type'] = 'nature'
  if first_screen:
    kw['first_screen'] = True
  return kw


def adam_options(flags):
  """--optimizer adam as keyword arguments (Engine's; AdamOptimizer's without the adam_ prefix), {} for
  rmsprop.  Pure; ValueError for a beta outside [0, 1) or an epsilon <= 0."""
  if getattr(flags, 'optimizer', 'rmsprop') != 'adam':
    return {}
  from src.optim import check_adam
  b1, b2, eps = check_adam(flags.adam_beta1, flags.adam_beta2, flags.adam_epsilon)
  return dict(optimizer='adam', adam_beta1=b1, adam_beta2=b2, adam_epsilon=eps)


def play_options(flags, world=None):
  """--mode engine --is_train false (Agent.play, agent.py:351-391, as a3c_engine_play): the
  Engine.play keyword arguments the flags select, or None when training.  Pure -- runs before any
  device work -- and rejects what play cannot honour, so --is_train is not silently dropped."""
  if flags.is_train:
    return None
  if flags.envs_on != 'device':
    raise ValueError('--is_train false plays the device envs: --envs_on %s is not supported' % flags.envs_on)
  if flags.update == 'hogwild':
    raise ValueError('--is_train false does not update: --update hogwild has no meaning there')
  world = int(os.environ.get('WORLD_SIZE', '1')) if world is None else int(world)
  if world > 1:
    raise ValueError('--is_train false evaluates with one process (WORLD_SIZE = %d)' % world)
  if flags.n_episode < 1 or flags.play_steps < 1:
    raise ValueError('--n_episode and --play_steps must be >= 1')
  if flags.test_ep is not None and flags.test_ep < 0:
    raise ValueError('--test_ep must be >= 0')
  if flags.greedy and flags.algo != 'a3c':
    raise ValueError('--greedy selects the a3c draw; q engines are epsilon-greedy (--test_ep 0 for greedy)')
  kw = dict(n_episode=int(flags.n_episode), n_step=int(flags.play_steps), test_ep=flags.test_ep,
            greedy=bool(flags.greedy))
  if flags.play_refill:
    kw['refill'] = True
  return kw


def run_play(config, flags, play_kw):
  """Evaluate the newest checkpoint (or, with a warning, the initial parameters) on a synchronous
  engine: one JSON line on stdout and in <logdir>/play.jsonl; nothing is trained or saved."""
  from src import checkpoint as C
  from src.base import BaseModel
  from src.engine import Engine
  from src.environment import catch_rules_of, game_kind, game_spec
  from src.kernels import param_names_shapes
  torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
  A, lives = game_spec(config.env_name)
  eng = Engine(num_envs=flags.num_envs, n_step=flags.n_step, action_size=A, algo=flags.algo, start_lives=lives,
               num_frames=flags.num_frames, seed=flags.random_seed, overlap=False, **engine_options(flags),
               game=game_kind(config.env_name), catch_rules=catch_rules_of(config.env_name),
               random_start=config.random_start, action_repeat=config.action_repeat)
  ns = param_names_shapes(A, flags.algo, lstm=eng.lstm, dqn_type=eng.dqn_type)
  ckdir = flags.checkpoint_dir or os.path.join(flags.logdir, BaseModel(config, verbose=False).model_dir)
  saver = C.Saver(ckdir, max_to_keep=flags.max_to_keep)
  restored = C.restore_engine(saver, eng, ns) if flags.resume else None
  if restored is None:
    print('main.py: no checkpoint in %s: playing the initial parameters' % ckdir, file=sys.stderr, flush=True)
    eng.reset(initial_params(eng, A, flags.algo, flags.random_seed))
  torch.cuda.synchronize()
  t0 = time.time()
  out = eng.play(**play_kw)
  dt = time.time() - t0
  ret, length = out['returns'], out['lengths']
  rec = dict(mode='play', checkpoint=saver.latest() if restored is not None else None,
             global_step=int(eng.counters[1].item()), n_episode=int(ret.size), n_step=play_kw['n_step'],
             test_ep=play_kw['test_ep'], greedy=play_kw['greedy'], best_reward=out['best_reward'],
             best_idx=out['best_idx'], mean_reward=float(ret.mean()), min_reward=float(ret.min()),
             max_reward=float(ret.max()), mean_length=float(length.mean()), terminated=int(out['terminated'].sum()),
             env_steps=int(length.sum()), seconds=dt)
  if play_kw.get('refill'):
    rec.update(refill=True, steps=out['steps'])
  print(json.dumps(rec), flush=True)
  os.makedirs(flags.logdir, exist_ok=True)
  with open(os.path.join(flags.logdir, 'play.jsonl'), 'a') as f:
    f.write(json.dumps(rec) + '\n')
  return eng


def initial_params(eng, action_size, algo, seed):
  """Flat host parameters initialised as the reference does: conv weights
  truncated_normal(0, 0.02) (agent.py:214), linear weights normal(0.02) (ops.py:36-37),
  zero biases (ops.py:24,38-39)."""
  from src.initializers import flatten_host, init_params
  from src.kernels import param_names_shapes
  ns = param_names_shapes(action_size, algo, lstm=eng.lstm, dqn_type=eng.dqn_type)
  return flatten_host(ns, eng.offsets, eng.params.numel(), init_params(ns, seed=seed))


def make_host_pool(config, flags, E, A, lives, rank):
  """Host-stepped envs for the external-env engine: the C++ synthetic emulator
  (`host`), or E gym envs wrapped with the reference's Environment rules (`gym`,
  environment.py:14-96)."""
  from src.host_env import AtariEnv, HostEnvPool, SyntheticHostEnvPool
  if flags.envs_on == 'host':
    return SyntheticHostEnvPool(E, A, lives, num_frames=min(flags.num_frames, 2048), seed=flags.random_seed,
                                env_id_base=rank * E, random_start=config.random_start,
                                action_repeat=config.action_repeat, threads=flags.host_threads)
  try:
    import gym
  except ImportError as e:
    raise RuntimeError('--envs_on gym needs the gym package (with the Atari ROMs)') from e
  # one emulator seed and one no-op-start stream per env (the reference: one env and one `random`
  # per worker process, environment.py:37), so the pool's threads cannot reorder the draws
  envs = []
  for e in range(E):
    sid = flags.random_seed + rank * E + e
    envs.append(AtariEnv(gym.make(config.env_name), action_repeat=config.action_repeat,
                         random_start=config.random_start, rng=random.Random(sid), seed=sid))
  return HostEnvPool(envs, threads=flags.host_threads)


def _agree(flag, world):
  """Rank 0's decision on every rank (checkpoint times must match across the ranks)."""
  if world == 1:
    return bool(flag)
  import torch.distributed as dist
  t = torch.tensor([1 if flag else 0], dtype=torch.int32,
                   device='cuda' if dist.get_backend() == 'nccl' else 'cpu')
  dist.broadcast(t, src=0)
  return bool(t.item())


def run_engine(config, flags):
  from src import checkpoint as C
  from src import distributed as D
  from src.base import BaseModel
  from src.engine import Engine
  from src.environment import catch_rules_of, game_kind, game_spec
  from src.kernels import param_names_shapes
  rank, world, local = D.init_from_env()
  torch.cuda.set_device(local)
  A, lives = game_spec(config.env_name)
  E = flags.num_envs
  net_kw = engine_options(flags)
  opts = dict(gamma=config.discount, discount=config.discount, beta=config.beta, learning_rate=config.learning_rate,
              max_step=config.max_step, decay=config.decay, momentum=config.momentum, epsilon=config.epsilon,
              clip_norm=config.clip_norm, literal_adv=int(config.literal_adv), ep_start=config.ep_start,
              ep_end=config.ep_end, ep_end_t=config.ep_end_t, learn_start=config.learn_start,
              target_q_update_step=config.target_q_update_step, random_start=config.random_start,
              action_repeat=config.action_repeat)
  host = flags.envs_on != 'device'
  if host and flags.update == 'hogwild':
    raise ValueError('--envs_on host/gym drives a synchronous engine; use --update sync or overlap')
  # hogwild overlaps the push / pull of rollout k-1 with rollout k (src/engine.py iterate_hogwild)
  overlap = flags.update in ('overlap', 'hogwild') and not host
  if flags.update == 'overlap' and not overlap and rank == 0:
    print('main.py: --update overlap needs device envs; running the synchronous engine',
          file=sys.stderr, flush=True)
  pool = make_host_pool(config, flags, E, A, lives, rank) if host else None
  eng = Engine(num_envs=E, n_step=flags.n_step, action_size=A, algo=flags.algo, start_lives=lives,
               num_frames=1 if host else flags.num_frames, seed=flags.random_seed, env_id_base=rank * E,
               world_size=world, overlap=overlap, external_env=host, game=game_kind(config.env_name),
               catch_rules=catch_rules_of(config.env_name), **net_kw, **opts)
  ns = param_names_shapes(A, flags.algo, lstm=eng.lstm, dqn_type=eng.dqn_type)
  # checkpoints: <logdir>/<model_dir> as the Supervisor's logdir (main.py:75), Saver max_to_keep
  # (agent.py:29); restored at start as managed_session does (main.py:90)
  ckdir = flags.checkpoint_dir or os.path.join(flags.logdir, BaseModel(config, verbose=False).model_dir)
  saver = C.Saver(ckdir, max_to_keep=flags.max_to_keep)
  restored = C.restore_engine(saver, eng, ns, rank, world) if flags.resume else None
  if restored is None:
    eng.reset(initial_params(eng, A, flags.algo, flags.random_seed))
    D.broadcast_params(eng.params, src=0)
    if flags.algo == 'q':
      eng.target_params.copy_(eng.params)
    if overlap:
      eng.reset()    # keeps the broadcast parameters, re-takes the pipeline snapshots
  elif rank == 0:
    print(json.dumps({'restored': saver.latest(), 'global_step': restored}), flush=True)
  xch = None
  if world > 1:
    xch = D.PartitionedPS(eng.params.numel()) if flags.exchange == 'sequential' else D.GradExchange()
  ps = None
  if flags.update == 'hogwild':
    from src.hogwild import HogwildPS
    ps = HogwildPS(eng.params, decay=config.decay, momentum=config.momentum, epsilon=config.epsilon,
                   ms=eng.ms, mom=eng.mom)     # (restored slots, or the TF1 init after reset)
  # the reference's worker loop `for self.step in xrange(self.step, self.max_step)` (agent.py:46,55):
  # each worker -- here each env, all in lock-step -- takes env-steps up to max_step on its own
  # counter; one rollout is n of them, and the overlap pipeline applies one call later
  n = flags.n_step
  remaining = max(0, int(config.max_step) - eng.worker_step)
  iterations = min(flags.iterations, -(-remaining // n) + (1 if overlap else 0))
  test_step = int(getattr(config, 'test_step', getattr(config, '_test_step', 5000)))
  log_every = flags.log_every or max(1, test_step // n)
  torch.cuda.synchronize()
  t0 = time.time()
  last_save = t0
  log = None
  if rank == 0:
    os.makedirs(flags.logdir, exist_ok=True)
    log = open(os.path.join(flags.logdir, 'engine.jsonl'), 'a')
  for it in range(iterations):
    if ps is not None:
      eng.iterate_hogwild(ps)
    elif pool is not None:
      eng.iterate_host(pool, exchange=xch)
    else:
      eng.iterate(exchange=xch)
    if rank == 0:
      eng.stats_accumulate()       # train_with_summary's aggregates (agent.py:91-131), on device
    if (it + 1) % log_every == 0:
      if rank == 0:
        loss = eng.loss.tolist()
        st = eng.read_stats(reset=True)
        torch.cuda.synchronize()
        dt = time.time() - t0
        wstep = eng.worker_step
        rec = dict(iteration=it + 1, global_step=int(eng.counters[1].item()), worker_step=wstep,
                   env_steps_per_sec=(it + 1) * E * n * world / dt, **st,
                   learning_rate=max(0.0, (config.max_step - wstep + 1.) / config.max_step * config.learning_rate),
                   loss_policy=loss[0], loss_value=loss[1], entropy=loss[2], loss_total=loss[3],
                   mean_return=float(eng.returns.mean().item()))
        print(json.dumps(rec), flush=True)
        log.write(json.dumps(rec) + '\n')
      if _agree(rank == 0 and time.time() - last_save >= flags.save_model_secs, world):
        _sync_slots(eng, xch, ps)
        C.save_engine(saver, eng, ns, rank, world, barrier=_barrier(world))
        last_save = time.time()
  torch.cuda.synchronize()
  if iterations > 0:
    _sync_slots(eng, xch, ps)
    C.save_engine(saver, eng, ns, rank, world, barrier=_barrier(world))    # the final state
  if ps is not None:
    ps.close()
  if pool is not None:
    pool.close()
  if log:
    log.close()
  return eng


def _sync_slots(eng, xch, ps):
  """The RMSProp slots a sharded update keeps per owner (partitioned PS ranges, Hogwild shards)
  into the engine's full ms / mom before a checkpoint."""
  for x in (xch, ps):
    if hasattr(x, 'sync_slots'):
      x.sync_slots(eng)


def _barrier(world):
  if world == 1:
    return None
  import torch.distributed as dist
  return dist.barrier


def run_agent(config, flags):
  from src import distributed as D
  from src.agent import Agent, Supervisor
  from src.environment import GymEnvironment
  from src.optim import AdamOptimizer, RMSPropOptimizer
  adam = adam_options(flags)
  rank, world, local = D.init_from_env()
  torch.cuda.set_device(local)
  random.seed(flags.random_seed + rank)
  env = GymEnvironment(config)
  optimizer = RMSPropOptimizer(None, decay=0.99, momentum=0, epsilon=0.1)     # main.py:64-65
  if adam:
    optimizer = AdamOptimizer(None, beta1=adam['adam_beta1'], beta2=adam['adam_beta2'], epsilon=adam['adam_epsilon'])
  agent = Agent(config, env, optimizer)
  agent.ep_end = random.sample([0.1, 0.01, 0.5], 1)[0]                        # main.py:68
  if world > 1:
    D.broadcast_params(agent.params, src=0)
  print(agent.model_dir)
  is_chief = rank == 0
  sv = Supervisor(is_chief=is_chief, logdir=os.path.join(flags.logdir, agent.model_dir), agent=agent)
  agent.update_target_q_network()
  if flags.is_train:
    (agent.train_with_summary if is_chief else agent.train)(sv, is_chief)
  else:
    agent.play(sv, is_chief)
  return agent


def main(argv=None):
  flags = parse_flags(argv)
  if flags.mode == 'agent' and flags.gae_lambda != 1.0:
    raise ValueError('--gae_lambda is an engine option: --mode agent is the per-step Q-learning loop')
  if flags.mode == 'agent' and flags.q_nstep:
    raise ValueError('--q_nstep is an engine option: --mode agent is the per-step Q-learning loop (one-step targets)')
  if flags.mode == 'agent' and flags.sarsa:
    raise ValueError('--sarsa is an engine option: --mode agent is the per-step Q-learning loop (max targets)')
  if flags.mode == 'agent' and flags.q_lambda is not None:
    raise ValueError('--q_lambda is an engine option: --mode agent is the per-step Q-learning loop (one-step targets)')
  if flags.mode == 'agent' and flags.first_screen:
    raise ValueError('--first_screen is an engine option: --mode agent is the reference loop (agent.py:59-67) as it stands')
  random.seed(flags.random_seed)
  np.random.seed(flags.random_seed)
  from config import get_config
  config = get_config(flags)
  config.cnn_format = 'NHWC'                       # main.py:45
  if flags.max_step is not None:
    config.max_step = flags.max_step
  config.algo, config.n_step, config.num_envs = flags.algo, flags.n_step, flags.num_envs
  if flags.mode == 'engine':
    engine_options(flags)             # reject unsupported reference options before any device work
    play_kw = play_options(flags)
    if play_kw is not None:
      return run_play(config, flags, play_kw)
    return run_engine(config, flags)
  return run_agent(config, flags)


if __name__ == '__main__':
  main()
