"""Game overs inside training rollouts, in every engine mode, against the CPU replay oracle.

The synthetic env ends an episode after 200-2000 steps, so the short parity runs see a game over
(env_reset: the episode counter, the new length and start frame, the lives refill, the no-op loop
of new_random_game) only by luck of their seed.  Here every case ends its episodes on schedule
(_engine_parity.schedule / end_episodes: ep_len shortened in the engine and the oracle alike, one
game over on every (rollout, t) cell of every back-propagated rollout) and runs one of the existing
checks unchanged -- same comparisons, same bars -- then asserts, from the counts the check
collected, the coverage tests/test_episode_ends_cpu.py proved for the case from the env alone.
So no case passes without its game overs, and what they must not break is compared: the bootstrap
cut at a terminal (returns, TD targets, late targets, GAE), the LSTM state zeroed after one, the
double-buffered env state after a reset, the frame ring, the summaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from _engine_parity import (EpisodeCount, assert_env_state, build, check_hogwild1_vs_oracle,  # noqa: E402
                            check_overlap_vs_oracle, check_sync_vs_oracle, scheduled)
from test_episode_ends_cpu import CASES, backprop, covered  # noqa: E402

A = 6


def assert_coverage(name, counts):
    """The counts a check collected meet the condition the CPU twin proved for the case."""
    case = CASES[name]
    assert counts['backprop'] == backprop(case) and counts['rollouts'] == case['rollouts'], (name, counts)
    assert covered(case, counts['cells']) is None, (name, covered(case, counts['cells']), counts['cells'].tolist())
    assert counts['cells'].sum() >= 3, (name, counts)


def run_case(name, monkeypatch=None):
    case = CASES[name]
    E, n, lives, seed, rollouts = case['E'], case['n'], case['lives'], case['seed'], case['rollouts']
    kw = dict(case.get('opts', {}))
    if 'scale' in case:
        kw['scale'] = case['scale']
    if case.get('schedule', True):
        kw['start'] = scheduled(backprop(case))
    if case.get('unfused'):
        # read by a3c_engine_create; a frame84 engine needs the fused screen, so its rejection shows
        # that the engines built below run the unfused head and the separate screen launch
        from src import _lib
        from src.engine import Engine
        monkeypatch.setenv('A3C_FUSED_SCREEN', '0')
        with pytest.raises(_lib.A3CError, match='fused screen'):
            Engine(num_envs=4, n_step=2, num_frames=8, frame84=1)
    check = case['check']
    if check == 'sync':
        _, ref = check_sync_vs_oracle(case['algo'], A, E, n, lives, iters=rollouts, seed=seed, **kw)
    elif check in ('overlap', 'hogwild-overlap'):
        _, ref = check_overlap_vs_oracle(A, E, n, lives, rollouts=rollouts, seed=seed, algo=case['algo'],
                                         learning_rate=3e-3, hogwild=check == 'hogwild-overlap', **kw)
    elif check == 'hogwild1':
        _, ref = check_hogwild1_vs_oracle(A, E, n, lives, iters=rollouts, seed=seed, learning_rate=3e-3, **kw)
    elif check == 'lstm-sync':
        from test_gpu_lstm import check_lstm_sync_vs_oracle
        _, ref = check_lstm_sync_vs_oracle(A, E, n, lives, iters=rollouts, seed=seed, learning_rate=2e-3, **kw)
    elif check == 'lstm-overlap':
        from test_gpu_lstm import check_lstm_overlap_vs_oracle
        _, ref = check_lstm_overlap_vs_oracle(A, E, n, lives, rollouts=rollouts, seed=seed, learning_rate=2e-3, **kw)
    else:
        raise ValueError(check)
    assert_coverage(name, ref.episode_counts)
    return ref


PARITY = [name for name, c in CASES.items()
          if c['check'] in ('sync', 'overlap', 'hogwild-overlap', 'hogwild1', 'lstm-sync', 'lstm-overlap')]


@pytest.mark.parametrize('name', PARITY)
def test_game_overs_match_oracle(name, monkeypatch):
    """One game over on every step of every back-propagated rollout (lives1-*: the natural ones of
    one-life envs, where a lost life is the game over), through the mode's own parity check."""
    run_case(name, monkeypatch)


@pytest.mark.parametrize('name', ['host-a3c', 'host-q'])
def test_game_overs_from_host_envs_match_oracle(name):
    """Host-stepped envs: the terminals (and the frames of the new games) arrive through
    ext_observe.  The host envs and the oracle's are shortened alike."""
    from src.host_env import HostEnvPool
    from test_gpu_host_env import HostSynthEnv
    case = CASES[name]
    E, n, lives, P = case['E'], case['n'], case['lives'], case['frames']
    made = []

    def pool(seed):
        made.append(HostEnvPool([HostSynthEnv(seed, e, P, A, lives) for e in range(E)], threads=2))
        return made[0]
    start = scheduled(backprop(case), host_envs=lambda: [h.env for h in made[0].envs])
    _, ref = check_sync_vs_oracle(case['algo'], A, E, n, lives, iters=case['rollouts'], seed=case['seed'], frames=P,
                                  host_pool=pool, start=start, learning_rate=2e-3, **case.get('opts', {}))
    assert_coverage(name, ref.episode_counts)


@pytest.mark.parametrize('name', ['gae-sync', 'gae-lstm-sync'])
def test_lambda_return_stops_at_game_overs(name):
    """GAE(0.9): returns and loss of every rollout against gae_ref (tests/test_gpu_gae.py
    check_rollout, its bars) with a game over at every t; the oracle replays the env in lock-step
    (rewards, terminals and env state bit-exact) and counts."""
    from test_gpu_gae import LAM, check_rollout
    case = CASES[name]
    E, n, lives, seed = case['E'], case['n'], case['lives'], case['seed']
    assert case['opts']['gae_lambda'] == LAM
    if case['check'] == 'gae-lstm':
        from test_gpu_lstm import build as build_lstm
        eng, ref, _ = build_lstm(A, E, n, lives, seed=seed, learning_rate=2e-3, gae_lambda=LAM)
    else:
        eng, ref, _ = build('a3c', A, E, n, lives, seed=seed, gae_lambda=LAM)
    assert abs(eng.cfg.gae_lambda - LAM) < 1e-7
    scheduled(backprop(case))(eng, ref)
    counts = EpisodeCount()
    for k in range(case['rollouts']):
        eng.iterate()
        torch.cuda.synchronize()
        terms, _ = check_rollout(eng.slot(0), eng.loss.cpu().numpy(), A, n, E, (name, k))
        out = ref.iterate(forced_actions=eng.actions.cpu().numpy(), grads=False)    # the env replay
        ref.tau += n
        counts.add(out)
        assert np.array_equal(eng.rewards.cpu().numpy(), out['rewards']), k
        assert np.array_equal(terms, out['terminals']), k
        assert_env_state(eng, ref, k)
    assert_coverage(name, counts.report(name))


@pytest.mark.parametrize('name', ['stats-a3c', 'stats-q'])
def test_summaries_count_game_overs(name):
    """train_with_summary's bookkeeping (agent.py:91-131; tests/test_gpu_checkpoint.py
    test_summaries_match_reference_bookkeeping, shortened) when the terminals are game overs: every
    env's episode ends once in the run, so num_game is the number of envs, and the episode
    rewards are those of the hand replay on the oracle's unclipped rewards."""
    case = CASES[name]
    algo, E, n, iters = case['algo'], case['E'], case['n'], case['rollouts']
    eng, ref, _ = build(algo, A, E, n, case['lives'], seed=case['seed'], frames=64, scale=1.0, learning_rate=1e-3,
                        **case.get('opts', {}))
    scheduled(backprop(case))(eng, ref)
    counts = EpisodeCount()
    acc = np.zeros(E)
    tot, eps_done, losses, qs = 0.0, [], [], []
    for it in range(iters):
        eng.rollout_grad()
        eng.stats_accumulate()
        torch.cuda.synchronize()
        out = ref.iterate(forced_actions=eng.actions.cpu().numpy())
        counts.add(out)
        assert np.array_equal(eng.terminals.cpu().numpy(), out['terminals'])
        r, t = out['rewards_raw'].astype(np.float64), out['terminals']
        for s in range(n):
            tot += r[s].sum()
            for e in range(E):
                if t[s, e]:
                    eps_done.append(acc[e])
                    acc[e] = 0.0
                else:
                    acc[e] += r[s, e]
        loss = eng.loss.cpu().numpy().astype(np.float64)
        z = eng.z.cpu().numpy()[:n].reshape(n * E, -1).astype(np.float64)
        losses.append(loss[0] if algo == 'q' else loss[3] / (n * E))
        qs.append(z[:, :A].mean() if algo == 'q' else z[:, A].mean())
        eng.apply()
        ref.apply(out['clipped'])
        assert_env_state(eng, ref, it)
    c = counts.report(name)
    assert_coverage(name, c)
    st = eng.read_stats(reset=True)
    # the finished episodes are the scheduled ones: one per env, every one a game over
    assert len(eps_done) == E == c['game_overs'] == c['terminals']
    assert st['num_game'] == E and st['env_steps'] == iters * n * E and st['updates'] == iters
    assert st['avg_reward'] == pytest.approx(tot / (iters * n * E), rel=1e-12, abs=1e-15)
    assert st['avg_ep_reward'] == pytest.approx(np.mean(eps_done), rel=1e-12)
    assert st['max_ep_reward'] == max(eps_done) and st['min_ep_reward'] == min(eps_done)
    assert st['avg_loss'] == pytest.approx(np.mean(losses), rel=1e-6)
    assert st['avg_q'] == pytest.approx(np.mean(qs), rel=1e-5, abs=1e-7)
    assert int(ref.env.episode.min()) == 2 and int(ref.env.episode.max()) == 2      # every env in its second game


def test_every_case_of_the_table_runs():
    ran = set(PARITY) | {'host-a3c', 'host-q', 'gae-sync', 'gae-lstm-sync', 'stats-a3c', 'stats-q'}
    assert ran == set(CASES)
