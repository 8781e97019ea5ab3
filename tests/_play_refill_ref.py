"""CPU restatement of play with refill (a3c_engine_play_ex, refill = 1; DESIGN §4e "Refill"): the
continuous form of the engine's batched evaluation.  Test infrastructure only (imported by
tests/test_*play_refill*.py); built on _play_ref's make_ref / ref_like states.

  * start: tau = 3; episodes idx = 0 .. min(E, n_episode)-1 start on envs e = idx as a wave does
    (new_random_game, the first screen into the 4 newest ring slots, LSTM state zero); the other
    envs are idle;
  * step: as play_ref's (forward, draw on the (tau, env id) Philox words, act with
    is_training=False, screen into ring slot tau+1, return += raw reward, length += 1);
  * an episode ends at a terminal, or when its own length reaches n_step (terminated = False; the
    emulator goes on: lives > 0); its words go to the per-episode outputs;
  * refill, in the same step: the envs that ended take the next unassigned episode indices in
    env-id order; one that gets idx < n_episode does new_random_game, its first screen goes into
    ring slots (tau+1-3 .. tau+1) mod R -- over the post-terminal screen --, return, length and
    LSTM h / c are zeroed; one that gets none is frozen for good;
  * tau += 1 per run step; the run ends when no env is live -- within ceil(n_episode/E) * n_step
    steps (asserted).
The engine's traced actions [bound, E] are replayed (forced_actions), as play_ref does."""
import numpy as np

from oracle import ref_cpu as Rc

from _play_ref import ENV_FIELDS, best_of


def step_bound(n_episode, n_step, E):
    return -(-n_episode // E) * n_step


def play_refill_ref(ref, n_episode, n_step, forced_actions=None, test_ep=None, greedy=False, forward=True):
    """Returns returns / lengths / terminated / episode_env / episode_tau0 [n_episode], best_reward,
    best_idx, steps (run steps in which any env was live), per (run step, env) over the step bound:
    live, sampled, u, eps, z, life_lost; and events: one (step, env, 'terminal' | 'cap', new idx or
    -1) per episode end, in the order the indices were handed out."""
    E, A, R = ref.E, ref.A, ref.R
    bound = step_bound(n_episode, n_step, E)
    q = ref.algo == 'q'
    mode1 = q or greedy
    if q and test_ep is None:
        eps_env = ref.ep_end.astype(np.float32)
    else:
        eps_env = np.full(E, max(float(test_ep or 0.0), 0.0), np.float32)
    zw = A + (0 if q else 1)
    returns = np.zeros(n_episode, np.float32)
    lengths = np.zeros(n_episode, np.int32)
    terminated = np.zeros(n_episode, bool)
    episode_env = np.zeros(n_episode, np.int32)
    episode_tau0 = np.zeros(n_episode, np.int64)
    live = np.zeros((bound, E), bool)
    sampled = np.full((bound, E), -1, np.int32)
    us = np.zeros((bound, E), np.float32)
    zs = np.full((bound, E, zw), np.nan)
    life_lost = np.zeros((bound, E), bool)
    events = []
    env = ref.env
    U = Rc.LSTM_UNITS
    n_act = min(E, n_episode)
    active = np.arange(E) < n_act
    tau = 3
    env.new_random_game(active)
    for e in range(n_act):
        s = ref.screen_of(env.frame[e])
        for c in range(4):
            ref.ring[e, (tau - 3 + c) % R] = s
        episode_env[e], episode_tau0[e] = e, tau
    hc = (np.zeros((E, U), ref.dtype), np.zeros((E, U), ref.dtype))
    ret = np.zeros(E, np.float32)
    length = np.zeros(E, np.int32)
    ep_idx = np.where(active, np.arange(E), -1)
    next_idx = n_act
    frozen = ~active
    steps = 0
    for t in range(bound):
        if frozen.all():
            break
        steps += 1
        now = ~frozen
        ref.tau = tau
        u, rnd = ref.draw_words(0)
        if forward:
            z, hc_new = ref._step_z(ref.states(tau), hc)
            if mode1:
                greedy_a = np.argmax(z[:, :A].astype(np.float32), axis=1).astype(np.int32)
                a = np.where(u < eps_env, rnd, greedy_a).astype(np.int32)
            else:
                pi, _, _ = Rc.softmax_stats(z[:, :A])
                a = Rc.sample_categorical(pi.astype(np.float32), u)
            zs[t][now] = z[now, :zw]
            sampled[t][now] = a[now]
            if ref.lstm:
                keep = now[:, None]
                hc = (np.where(keep, hc_new[0], hc[0]), np.where(keep, hc_new[1], hc[1]))
        else:
            a = np.zeros(E, np.int32)
        us[t] = u
        acts = a if forced_actions is None else np.asarray(forced_actions[t], np.int32)
        acts = np.where(now, acts, 0).astype(np.int32)
        saved = {f: getattr(env, f).copy() for f in ENV_FIELDS}
        lives0 = env.lives.copy()
        frame, reward, tm = env.act(acts, is_training=False)            # agent.py:373
        for f in ENV_FIELDS:                                            # idle envs do not advance
            v = getattr(env, f)
            v[frozen] = saved[f][frozen]
        live[t] = now
        life_lost[t] = now & (env.lives < lives0) & ~tm
        ret = np.where(now, ret + reward, ret).astype(np.float32)       # agent.py:377
        length += now
        for e in np.flatnonzero(now):
            ref.ring[e, (tau + 1) % R] = ref.screen_of(frame[e])
        ended = now & (tm | (length >= n_step))
        refilled = np.zeros(E, bool)
        for e in np.flatnonzero(ended):                                 # env-id order
            idx = ep_idx[e]
            returns[idx], lengths[idx], terminated[idx] = ret[e], length[e], bool(tm[e])
            new = -1
            if next_idx < n_episode:
                new, next_idx = next_idx, next_idx + 1
                refilled[e] = True
                ep_idx[e] = new
                episode_env[new], episode_tau0[new] = e, tau + 1
            events.append((t, int(e), 'terminal' if tm[e] else 'cap', new))
        if refilled.any():
            env.new_random_game(refilled)          # agent.py:363 (resets only where lives == 0)
            for e in np.flatnonzero(refilled):
                s = ref.screen_of(env.frame[e])
                for c in range(4):                                      # agent.py:366-367
                    ref.ring[e, (tau + 1 - 3 + c) % R] = s
            ret[refilled] = 0
            length[refilled] = 0
            keep = ~refilled[:, None]
            hc = (np.where(keep, hc[0], 0).astype(ref.dtype), np.where(keep, hc[1], 0).astype(ref.dtype))
        frozen = frozen | (ended & ~refilled)
        tau += 1
    assert frozen.all() and next_idx == n_episode and len(events) == n_episode, 'the step bound did not hold'
    best_reward, best_idx = best_of(returns)
    return dict(returns=returns, lengths=lengths, terminated=terminated, episode_env=episode_env,
                episode_tau0=episode_tau0, best_reward=best_reward, best_idx=best_idx, steps=steps, bound=bound,
                live=live, sampled=sampled, u=us, eps=np.broadcast_to(eps_env, (bound, E)).copy(), z=zs,
                life_lost=life_lost, events=events, last_tau=tau)


def schedule_facts(r):
    """What a schedule exercises: refills after a terminal / after a cap, the largest number of
    envs that ended in one step, and the envs left idle (ended, no episode left) before the last
    step."""
    ev = r['events']
    per_step = {}
    for t, _, _, _ in ev:
        per_step[t] = per_step.get(t, 0) + 1
    return dict(refill_terminal=sum(1 for _, _, k, n in ev if k == 'terminal' and n >= 0),
                refill_cap=sum(1 for _, _, k, n in ev if k == 'cap' and n >= 0),
                max_together=max(per_step.values()),
                idle_early=sum(1 for t, _, _, n in ev if n < 0 and t < r['steps'] - 1))
