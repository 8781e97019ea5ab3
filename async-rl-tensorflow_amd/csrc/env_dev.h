// Synthetic Atari stand-in (device side), bit-identical to oracle/synthetic_env.py, with the
// reference's interface semantics: new_game environment.py:28-33, new_random_game :35-40,
// act :78-96 (action repeat, life-loss terminal when training).
#pragma once
#include "env.h"

#define GOLDEN_MULT 2654435761u

struct EnvState {
  uint32_t episode, ep_step, ep_len;
  int32_t lives, frame;
  float reward;
  uint32_t terminal;
};

__device__ inline EnvState env_load(const EnvBufs& b, int64_t i) {
  EnvState s;
  s.episode = b.episode[i]; s.ep_step = b.ep_step[i]; s.ep_len = b.ep_len[i];
  s.lives = b.lives[i]; s.frame = b.frame[i]; s.reward = b.reward[i]; s.terminal = b.terminal[i];
  return s;
}

__device__ inline void env_store(const EnvBufs& b, int64_t i, const EnvState& s, bool frame = true) {
  b.episode[i] = s.episode; b.ep_step[i] = s.ep_step; b.ep_len[i] = s.ep_len;
  b.lives[i] = s.lives; b.reward[i] = s.reward; b.terminal[i] = (uint8_t)s.terminal;
  if (frame) b.frame[i] = s.frame;
}

// self.env.reset() (environment.py:30)
__host__ __device__ inline void env_reset(EnvState& s, const EnvParams& p, uint32_t id) {
  s.episode += 1u;
  s.ep_step = 0;
  s.lives = p.L0;
  u32x4 x = philox4x32(s.episode, id, P_RESET, 0u, p.k0, p.k1);
  s.ep_len = 200u + x.x % 1801u;
  s.frame = (int32_t)(x.y % (uint32_t)p.P);
}

// frame index of a step whose draw was x.x, for `action`
__host__ __device__ inline int32_t env_frame_of(uint32_t xx, uint32_t action, const EnvParams& p) {
  return (int32_t)((xx + action * GOLDEN_MULT) % (uint32_t)p.P);
}

// self.env.step(action) (environment.py:42-43) without the frame: nothing here depends on the
// action, which only picks the frame (env_frame_of(returned x.x, action))
__host__ __device__ inline uint32_t env_step_core(EnvState& s, const EnvParams& p, uint32_t id) {
  const uint32_t st = s.ep_step + 1u;
  s.ep_step = st;
  u32x4 x = philox4x32(st, id, s.episode, P_STEP, p.k0, p.k1);
  const float u = u01(x.y);
  const float rp = 0.02f;
  s.reward = u < rp ? 1.0f : (u >= 1.0f - rp ? -1.0f : 0.0f);
  int32_t lives = s.lives;
  if (u01(x.z) < (1.0f / 256.0f) && lives > 0) lives -= 1;
  const bool over = st >= s.ep_len;
  if (over) lives = 0;
  s.lives = lives;
  s.terminal = (over || (p.L0 > 0 && lives == 0)) ? 1u : 0u;
  return x.x;
}

// self.env.step(action) (environment.py:42-43)
__host__ __device__ inline void env_step_raw(EnvState& s, const EnvParams& p, uint32_t id, uint32_t action) {
  s.frame = env_frame_of(env_step_core(s, p, id), action, p);
}

// Environment.new_random_game (environment.py:35-40) via new_game (:28-33)
__host__ __device__ inline void env_new_random_game(EnvState& s, const EnvParams& p, uint32_t id) {
  if (s.lives == 0) env_reset(s, p, id);
  env_step_raw(s, p, id, 0u);
  u32x4 x = philox4x32(s.ep_step, id, s.episode, P_NOOP, p.k0, p.k1);
  const uint32_t k = x.x % (uint32_t)p.random_start;
  for (uint32_t i = 0; i < k; ++i) env_step_raw(s, p, id, 0u);
}

// GymEnvironment.act (environment.py:78-96) up to the frame: the repeats' rewards, lives
// and terminal do not depend on the action; returns the last executed step's draw, whose
// frame is env_frame_of(draw, action) (so the act can run before the action is drawn)
__host__ __device__ inline uint32_t env_act_pre(EnvState& s, const EnvParams& p, uint32_t id, bool training) {
  float cum = 0.f;
  const int32_t start_lives = s.lives;
  uint32_t xx = 0;
  for (int r = 0; r < p.action_repeat; ++r) {
    xx = env_step_core(s, p, id);
    cum = cum + s.reward;
    if (training && start_lives > s.lives) {
      cum -= 1.0f;
      s.terminal = 1u;
    }
    if (s.terminal) break;
  }
  s.reward = cum;
  return xx;
}

// GymEnvironment.act (environment.py:78-96)
__host__ __device__ inline void env_act(EnvState& s, const EnvParams& p, uint32_t id, uint32_t action, bool training) {
  s.frame = env_frame_of(env_act_pre(s, p, id, training), action, p);
}


// ---- Catch (A3C_GAME_CATCH): a game with real dynamics whose whole state is the pool
// frame index f = (c * CATCH_ROWS + r) * CATCH_COLS + p -- ball column c, ball row r, paddle column
// p.  ep_step mirrors r, ep_len = CATCH_ROWS - 1, lives stays 0.  The ball falls one row per step;
// actions 0 stay, 1 left, 2 right (anything else: stay); at the landing (r = CATCH_ROWS - 1) the
// reward is +1 with the paddle under the ball, else -1, and the episode ends.  No Philox draw in a
// step, one in a reset.  The act is split for the fused head kernels: catch_act_pre is everything
// that does not depend on the action (rows, landing, terminal), catch_act_post the paddle move,
// the reward and the frame index.
// Two rule parameters (EnvParams; a3c_engine_set_catch_rules): the ball is drawn only in
// rows < catch_visible (the pool render), the paddle moves only in steps from a row >= catch_frozen,
// and the reset drops the ball where the paddle can still reach it.  10, 0 is the game above.
#define CATCH_COLS 8
#define CATCH_ROWS 10
#define CATCH_FRAMES (CATCH_COLS * CATCH_ROWS * CATCH_COLS)   // 640

// reset (and new_game / new_random_game: lives == 0 always holds, no no-op steps follow)
__host__ __device__ inline void catch_reset(EnvState& s, const EnvParams& p, uint32_t id) {
  s.episode += 1u;
  u32x4 x = philox4x32(s.episode, id, P_RESET, 0u, p.k0, p.k1);
  s.ep_step = 0;
  s.ep_len = CATCH_ROWS - 1;
  s.lives = 0;
  // the ball's column: uniform over the columns within M = 9 - frozen of the paddle's, the paddle's
  // free steps (frozen <= 2: M >= 7, lo = 0, hi = 7, c = x.x % 8)
  const int pc = (int)(x.y % CATCH_COLS), m = CATCH_ROWS - 1 - (int)p.catch_frozen;
  const int lo = pc - m > 0 ? pc - m : 0, hi = pc + m < CATCH_COLS - 1 ? pc + m : CATCH_COLS - 1;
  const uint32_t c = (uint32_t)lo + x.x % (uint32_t)(hi - lo + 1);
  s.frame = (int32_t)(c * CATCH_ROWS * CATCH_COLS + (uint32_t)pc);
  s.reward = 0.f;
  s.terminal = 0u;
}

// `repeat` steps of one action up to the action: ball row, landing, terminal (the loop of
// env_act_pre: stop at a terminal).  s.frame stays the pre-act frame, s.reward is 0 (the reward
// needs the action).  Returns the word catch_act_post finishes the act from: the pre-act frame
// reduced into [0, CATCH_FRAMES) | new row << 10 | paddle moves << 14 | landed in this act << 18.
// A step on a landed state changes nothing: reward 0, terminal 1, no move.  `frozen`: a step from a
// row < frozen advances the row and is no paddle move.
__host__ __device__ inline uint32_t catch_act_pre(EnvState& s, int repeat, int frozen) {
  const uint32_t f = (uint32_t)s.frame % (uint32_t)CATCH_FRAMES;
  uint32_t r = (f / CATCH_COLS) % CATCH_ROWS, moves = 0, landed = 0;
  for (int k = 0; k < repeat; ++k) {
    if (r < CATCH_ROWS - 1) {
      moves += (int)r >= frozen ? 1u : 0u;
      r += 1u;
      landed = r == CATCH_ROWS - 1 ? 1u : 0u;
    } else {
      landed = 0u;
    }
    if (r == CATCH_ROWS - 1) break;
  }
  s.ep_step = r;
  s.ep_len = CATCH_ROWS - 1;
  s.lives = 0;
  s.reward = 0.f;
  s.terminal = r == CATCH_ROWS - 1 ? 1u : 0u;
  return f | r << 10 | moves << 14 | landed << 18;
}

// the action's part: `moves` clamped paddle steps, the landing's reward, the post-act frame index
// (< CATCH_FRAMES for every word catch_act_pre returns: c, r', p' are each within their range)
__host__ __device__ inline int32_t catch_act_post(uint32_t w, uint32_t action, float& reward) {
  const int f = (int)(w & 1023u), r = (int)(w >> 10 & 15u), moves = (int)(w >> 14 & 15u);
  const int c = f / (CATCH_ROWS * CATCH_COLS);
  int p = f % CATCH_COLS + moves * ((action == 2u ? 1 : 0) - (action == 1u ? 1 : 0));
  p = p < 0 ? 0 : (p > CATCH_COLS - 1 ? CATCH_COLS - 1 : p);
  reward = (w >> 18 & 1u) ? (p == c ? 1.0f : -1.0f) : 0.f;
  return (c * CATCH_ROWS + r) * CATCH_COLS + p;
}

// GymEnvironment.act for Catch (is_training makes no difference: no life is ever lost); repeat = 1
// is the raw step of SimpleGymEnvironment.act
__host__ __device__ inline void catch_act(EnvState& s, int repeat, int frozen, uint32_t action) {
  const uint32_t w = catch_act_pre(s, repeat, frozen);
  s.frame = catch_act_post(w, action, s.reward);
}

// ---- the game picked at compile time (GAME: A3C_GAME_*), for the kernels that step an env -------
template <int GAME>
__host__ __device__ inline void game_new_game(EnvState& s, const EnvParams& p, uint32_t id) {
  if constexpr (GAME == A3C_GAME_CATCH) {
    catch_reset(s, p, id);
  } else {
    if (s.lives == 0) env_reset(s, p, id);
    env_step_raw(s, p, id, 0u);
  }
}

template <int GAME>
__host__ __device__ inline void game_new_random_game(EnvState& s, const EnvParams& p, uint32_t id) {
  if constexpr (GAME == A3C_GAME_CATCH) catch_reset(s, p, id);     // (random_start: the reset is the random start)
  else env_new_random_game(s, p, id);
}

template <int GAME>
__host__ __device__ inline void game_act(EnvState& s, const EnvParams& p, uint32_t id, uint32_t action, bool training,
                                         bool simple = false) {
  if constexpr (GAME == A3C_GAME_CATCH) {
    catch_act(s, simple ? 1 : p.action_repeat, p.catch_frozen, action);
  } else {
    if (simple) env_step_raw(s, p, id, action);
    else env_act(s, p, id, action, training);
  }
}
