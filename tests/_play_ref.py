"""CPU restatement of the engine's batched evaluation (a3c_engine_play), the batched form of
Agent.play (agent.py:351-391).  Test infrastructure only (imported by tests/test_play*.py).

Built from oracle.synthetic_env.SyntheticAtari, oracle.ref_cpu and oracle.philox through an
EngineRef of its own (its ring handling, screens, per-step forward and draw words):
  * episode idx = w*E + e is played by env e in wave w; ceil(n_episode/E) waves;
  * wave start: new_random_game of the wave's envs only (agent.py:363, environment.py:35-40; the
    emulator goes on where the env's last episode stopped), the first screen into the 4 newest ring
    slots (agent.py:366-367), LSTM state zeroed, tau = 3 + w*(n_step + 4);
  * step: forward, draw on the (tau, env id) Philox words, act with is_training=False
    (agent.py:373), screen into the ring, return += raw reward (the terminal step's too,
    agent.py:377), length += 1; a terminal ends the episode, no new game follows;
  * an env that is done or has no episode in the wave is frozen: SyntheticAtari.act steps every
    env, so the frozen envs' fields are saved and restored around the call.
The engine's traced actions are replayed (forced_actions), as _engine_parity does."""
import numpy as np

from oracle import ref_cpu as Rc
from oracle.engine_ref import EngineRef

ENV_FIELDS = ('episode', 'ep_step', 'ep_len', 'lives', 'frame', 'reward', 'terminal')


def make_ref(params, E, A, algo='a3c', lives=0, frames=48, seed=123, env_id_base=0, action_repeat=1,
             random_start=30, lstm=False, frame84=False, dqn_type='nips'):
    """An EngineRef for play: zeroed env state (lives = 0: the first new_random_game resets), no
    reset() -- the play context starts from zeros, not from the training envs."""
    return EngineRef(params, E, 1, A, algo, lives, frames, seed, env_id_base=env_id_base,
                     action_repeat=action_repeat, random_start=random_start, lstm=lstm, frame84=frame84,
                     dqn_type=dqn_type)


def ref_like(ref, E=None, env_id_base=None):
    """A fresh play restatement with the configuration and parameters of a training oracle."""
    env = ref.env
    return make_ref(ref.params, ref.E if E is None else E, ref.A, ref.algo, env.L0, env.P, ref.seed,
                    int(env.ids[0]) if env_id_base is None else env_id_base, env.action_repeat, env.random_start,
                    ref.lstm, ref.frame84, ref.dqn_type)


def best_of(returns):
    """agent.py:361, 382-385: strict >, from (0, 0), in idx order."""
    best_reward, best_idx = 0.0, 0
    for idx, r in enumerate(returns):
        if r > best_reward:
            best_reward, best_idx = float(r), idx
    return best_reward, best_idx


def play_ref(ref, n_episode, n_step, forced_actions=None, test_ep=None, greedy=False, forward=True):
    """Play on the restatement `ref` (make_ref / ref_like; its env and ring persist across calls, as
    the engine's play context does).  forced_actions [waves, n_step, E]: the engine's trace (entries
    of frozen envs are ignored).  forward=False skips the network (actions must be forced).
    Returns returns / lengths / terminated [n_episode], best_reward, best_idx, and per (wave, step,
    env): live (the env took this step), sampled, u, eps, z; life_lost (a live step that lost a life
    without a terminal); last_tau [waves] (tau after the wave's last step that any env took)."""
    E, A, R = ref.E, ref.A, ref.R
    waves = -(-n_episode // E)
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
    live = np.zeros((waves, n_step, E), bool)
    sampled = np.full((waves, n_step, E), -1, np.int32)
    us = np.zeros((waves, n_step, E), np.float32)
    zs = np.full((waves, n_step, E, zw), np.nan)
    life_lost = np.zeros((waves, n_step, E), bool)
    last_tau = np.zeros(waves, np.int64)
    env = ref.env
    U = Rc.LSTM_UNITS
    for w in range(waves):
        n_act = min(E, n_episode - w * E)
        active = np.arange(E) < n_act
        tau = 3 + w * (n_step + 4)
        env.new_random_game(active)
        for e in range(n_act):
            s = ref.screen_of(env.frame[e])
            for c in range(4):
                ref.ring[e, (tau - 3 + c) % R] = s
        hc = (np.zeros((E, U), ref.dtype), np.zeros((E, U), ref.dtype))
        ret = np.zeros(E, np.float32)
        length = np.zeros(E, np.int32)
        term = np.zeros(E, bool)
        frozen = ~active
        for t in range(n_step):
            if frozen.all():
                break
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
                zs[w, t][now] = z[now, :zw]
                sampled[w, t][now] = a[now]
                if ref.lstm:
                    keep = now[:, None]
                    hc = (np.where(keep, hc_new[0], hc[0]), np.where(keep, hc_new[1], hc[1]))
            else:
                a = np.zeros(E, np.int32)
            us[w, t] = u
            acts = a if forced_actions is None else np.asarray(forced_actions[w][t], np.int32)
            acts = np.where(now, acts, 0).astype(np.int32)
            saved = {f: getattr(env, f).copy() for f in ENV_FIELDS}
            lives0 = env.lives.copy()
            frame, reward, tm = env.act(acts, is_training=False)            # agent.py:373
            for f in ENV_FIELDS:                                            # frozen envs do not advance
                v = getattr(env, f)
                v[frozen] = saved[f][frozen]
            live[w, t] = now
            life_lost[w, t] = now & (env.lives < lives0) & ~tm
            ret = np.where(now, ret + reward, ret).astype(np.float32)       # agent.py:377
            length += now
            for e in np.flatnonzero(now):
                ref.ring[e, (tau + 1) % R] = ref.screen_of(frame[e])
            term |= now & tm
            frozen = frozen | tm
            tau += 1
        last_tau[w] = tau
        returns[w * E:w * E + n_act] = ret[:n_act]
        lengths[w * E:w * E + n_act] = length[:n_act]
        terminated[w * E:w * E + n_act] = term[:n_act]
    best_reward, best_idx = best_of(returns)
    return dict(returns=returns, lengths=lengths, terminated=terminated, best_reward=best_reward, best_idx=best_idx,
                live=live, sampled=sampled, u=us, eps=np.broadcast_to(eps_env, (waves, n_step, E)).copy(), z=zs,
                life_lost=life_lost, last_tau=last_tau, waves=waves)
