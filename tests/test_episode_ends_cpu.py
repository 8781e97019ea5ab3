"""The precondition of tests/test_gpu_episode_ends.py, checked without a GPU: every case's seed,
shape and schedule put the game overs where its GPU test says they are.

The synthetic env's terminals depend on neither actions nor parameters (oracle/synthetic_env.py:
reward, life loss and episode length are hashes of env id, episode and step), so stepping
SyntheticAtari alone, in the order of the worker loop (agent.py:52-67: act, then new_random_game on
a terminal), gives exactly the terminals and game overs the engine and the oracle will see.  A game
over is a terminal whose new game is a reset (environment.py:28-33: lives == 0), where `episode`
advances; a lost life with lives left is a terminal but no game over.

CASES is the one table of both files.  The default coverage condition ('cells') is at least one
game over in every (rollout, t) cell of every back-propagated rollout (the overlap pipeline's last
rollout has no backward); a case that cannot meet it states its own."""
import numpy as np
import pytest

from oracle.synthetic_env import SyntheticAtari
from _engine_parity import schedule

# check: which comparison of the GPU file runs the case (the overlap forms back-propagate all but
# the last rollout); opts: engine options, the ones the env knows (random_start, action_repeat) used
# here too; cond: the coverage condition (see covered()).
OVERLAP = ('overlap', 'hogwild-overlap', 'lstm-overlap')
CASES = {
    'a3c-sync': dict(check='sync', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2001),
    'a3c-overlap': dict(check='overlap', algo='a3c', E=37, n=5, rollouts=6, lives=0, seed=2002),
    'q-sync': dict(check='sync', algo='q', E=16, n=4, rollouts=4, lives=3, seed=2007,
                   opts=dict(target_q_update_step=100)),
    'q-overlap': dict(check='overlap', algo='q', E=16, n=4, rollouts=5, lives=3, seed=2007,
                      opts=dict(target_q_update_step=100)),
    'double-q-overlap': dict(check='overlap', algo='q', E=16, n=4, rollouts=5, lives=0, seed=2008,
                             opts=dict(target_q_update_step=100, double_q=1)),
    'nature-sync': dict(check='sync', algo='a3c', E=13, n=3, rollouts=3, lives=5, seed=2004,
                        opts=dict(dqn_type='nature'), scale=2.0),
    'nature-overlap': dict(check='overlap', algo='a3c', E=9, n=3, rollouts=4, lives=3, seed=2009,
                           opts=dict(dqn_type='nature'), scale=2.0),
    'lstm-sync': dict(check='lstm-sync', algo='a3c', E=16, n=5, rollouts=3, lives=3, seed=2005),
    'lstm-overlap': dict(check='lstm-overlap', algo='a3c', E=16, n=5, rollouts=4, lives=3, seed=2005, scale=2.0),
    'gae-sync': dict(check='gae', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2010, opts=dict(gae_lambda=0.9)),
    'gae-lstm-sync': dict(check='gae-lstm', algo='a3c', E=16, n=5, rollouts=3, lives=3, seed=2011,
                          opts=dict(gae_lambda=0.9)),
    'frame84-sync': dict(check='sync', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2012, opts=dict(frame84=1)),
    # the episode ends in the middle of the repeat (env e: e % 3 raw steps early); after the reset
    # new_random_game draws no extra no-op (random_start = 1) or up to 29 of them
    'repeat3-start1': dict(check='sync', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2006,
                           opts=dict(action_repeat=3, random_start=1), cond='cells+midrepeat'),
    'repeat3-start30': dict(check='sync', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2006,
                            opts=dict(action_repeat=3, random_start=30), cond='cells+midrepeat'),
    'hogwild1': dict(check='hogwild1', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2013),
    'hogwild-overlap': dict(check='hogwild-overlap', algo='a3c', E=16, n=5, rollouts=4, lives=0, seed=2014),
    # E = 8 < n * K = 10: the schedule (period 10) ends env e at env step e, which is every step of
    # the first rollout and the first three of the second -- across the rollout boundary
    'host-a3c': dict(check='host', algo='a3c', E=8, n=5, rollouts=2, lives=3, seed=2015, frames=40, cond='first8'),
    'host-q': dict(check='host', algo='q', E=8, n=5, rollouts=2, lives=0, seed=2016, frames=40, cond='first8',
                   opts=dict(target_q_update_step=40)),
    # no schedule: with one life a lost life is the game over (lives == 0 on entry to new_game)
    'lives1-sync': dict(check='sync', algo='a3c', E=37, n=5, rollouts=4, lives=1, seed=9002, schedule=False,
                        cond='natural'),
    'lives1-overlap': dict(check='overlap', algo='a3c', E=37, n=5, rollouts=5, lives=1, seed=9002, schedule=False,
                           cond='natural'),
    'stats-a3c': dict(check='stats', algo='a3c', E=16, n=5, rollouts=3, lives=0, seed=2017, cond='cells+all'),
    'stats-q': dict(check='stats', algo='q', E=16, n=5, rollouts=3, lives=0, seed=2018, cond='cells+all',
                    opts=dict(target_q_update_step=100)),
    # A3C_FUSED_SCREEN=0: the unfused head (net_head.h head_act) and the separate screen launch
    'unfused-a3c-sync': dict(check='sync', algo='a3c', E=16, n=5, rollouts=3, lives=3, seed=2019, unfused=True),
    'unfused-q-sync': dict(check='sync', algo='q', E=16, n=4, rollouts=4, lives=0, seed=2020, unfused=True,
                           opts=dict(target_q_update_step=100)),
    'unfused-a3c-overlap': dict(check='overlap', algo='a3c', E=16, n=5, rollouts=4, lives=0, seed=2021, unfused=True),
}


def backprop(case):
    """How many of the case's rollouts are back-propagated."""
    return case['rollouts'] - 1 if case['check'] in OVERLAP else case['rollouts']


def simulate(case):
    """Step the env alone through the case's rollouts.  Returns dict: overs, terms [rollouts, n]
    (game overs / terminals per cell), midrepeat (game overs whose act ran fewer raw steps than
    action_repeat), lives0 (game overs by a lost last life rather than by the episode's length)."""
    opts = case.get('opts', {})
    E, n, r = case['E'], case['n'], int(opts.get('action_repeat', 1))
    env = SyntheticAtari(case['seed'], E, case.get('frames', 48), 6, case['lives'], int(opts.get('random_start', 30)), r)
    env.new_random_game()
    if case.get('schedule', True):
        env.ep_len[:] = (env.ep_step.astype(np.int64) + schedule(E, n, backprop(case), r)).astype(np.uint32)
    overs = np.zeros((case['rollouts'], n), np.int64)
    terms = np.zeros_like(overs)
    mid = lives0 = 0
    for k in range(case['rollouts']):
        for t in range(n):
            before = env.ep_step.copy()
            _, _, term = env.act(np.zeros(E, np.int32), is_training=True)
            ran = env.ep_step - before
            by_length = env.ep_step >= env.ep_len
            episode = env.episode.copy()
            if term.any():
                env.new_random_game(term)
            over = env.episode != episode
            assert not (over & ~term).any()
            terms[k, t] = term.sum()
            overs[k, t] = over.sum()
            mid += int((over & (ran < r)).sum())
            lives0 += int((over & ~by_length).sum())
    return dict(overs=overs, terms=terms, midrepeat=mid, lives0=lives0)


def covered(case, overs, extra=None):
    """The case's coverage condition on its game overs per (rollout, t) cell [>= backprop, n];
    returns the reason it fails, or None.  Used by this file on simulate() and by the GPU file on
    the counts its check collected."""
    K, n = backprop(case), case['n']
    cells = np.asarray(overs)[:K]
    cond = case.get('cond', 'cells')
    if cond.startswith('cells'):
        if not (cells >= 1).all():
            return f'cells without a game over: {np.argwhere(cells < 1).tolist()}'
        if cond == 'cells+all' and cells.sum() != case['E']:       # every env's episode ends, once
            return f"{int(cells.sum())} game overs, not one per env ({case['E']})"
    elif cond == 'first8':
        flat = cells.reshape(-1)
        if not (flat[:8] >= 1).all():
            return f'steps without a game over among the first 8: {np.argwhere(flat[:8] < 1).ravel().tolist()}'
    elif cond == 'natural':
        if cells.sum() < 3 or cells[:, 0].sum() < 1 or cells[:, n - 1].sum() < 1:
            return f'{int(cells.sum())} game overs, {int(cells[:, 0].sum())} at t = 0, {int(cells[:, n - 1].sum())} at t = n-1'
    else:
        raise ValueError(cond)
    return None


@pytest.mark.parametrize('name', list(CASES))
def test_case_meets_its_coverage_condition(name):
    case = CASES[name]
    K, n, E = backprop(case), case['n'], case['E']
    if case.get('cond', 'cells').startswith('cells'):
        assert E >= n * K, 'the schedule needs an env per cell'
    sim = simulate(case)
    print(f"{name}: game overs {int(sim['overs'].sum())} terminals {int(sim['terms'].sum())} "
          f"mid-repeat {sim['midrepeat']} by last life {sim['lives0']} cells {sim['overs'][:K].tolist()}")
    assert covered(case, sim['overs']) is None, covered(case, sim['overs'])
    assert sim['overs'][:K].sum() >= 3                       # no case passes without game overs
    if case.get('cond') == 'cells+midrepeat':
        assert sim['midrepeat'] >= 5                         # (10 of the 16 scheduled ends)
    if case.get('cond') == 'natural':
        assert sim['lives0'] == sim['overs'].sum()           # every game over here is a lost last life


def test_schedule_covers_every_cell_once_per_env():
    for E, n, K, r in ((16, 5, 3, 1), (37, 5, 5, 1), (16, 5, 3, 3), (13, 3, 3, 1)):
        d = schedule(E, n, K, r)
        assert d.shape == (E,) and (d >= 1).all()
        step = -(-d // r) - 1                                # the env step (act) in which the episode ends
        assert sorted(set(step.tolist())) == list(range(n * K))
        assert ((r * (step + 1) - d) == np.arange(E) % r).all()     # raw steps short of a full repeat


def test_schedule_alone_makes_the_game_overs():
    """Without the schedule the same seeds give no game over at all in these runs (episodes last
    200 steps at least, and lives 0 has no life to lose): what the GPU cases see is the schedule's."""
    for name in ('a3c-sync', 'a3c-overlap', 'repeat3-start1'):
        sim = simulate(dict(CASES[name], schedule=False))
        assert sim['overs'].sum() == 0 and sim['terms'].sum() == 0, name
