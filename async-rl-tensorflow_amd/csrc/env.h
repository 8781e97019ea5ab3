#pragma once
#include "net.h"

#define SCREEN_H 210
#define SCREEN_W 160
#define IMG_OUT IMG

struct PreGeom;
PreGeom a3c_make_geom(int in_h, int in_w, int out_h, int out_w);
int a3c_pool_fill_launch(uint8_t* pool, int P, uint32_t k0, uint32_t k1, hipStream_t s,
                         int frame_bytes = SCREEN_H * SCREEN_W * 3);
// Catch (A3C_GAME_CATCH): frames 0..639 of an RGB pool of P >= 640 frames rendered from the frame index
// (visible_rows: the ball is drawn in the frames of rows < visible_rows; 10: all)
int a3c_pool_render_catch_launch(uint8_t* pool, int P, int visible_rows, hipStream_t s);
// preprocess.hip: Environment.screen of frames idx[0..n) of rgb into out; its kernels' output rows per workgroup
int a3c_launch_screen_atari(const uint8_t* rgb, const int32_t* idx, int64_t n, uint8_t* out, int64_t stride,
                            hipStream_t s);
int a3c_screen_rows();
int a3c_env_init_launch(const EnvParams& p, const EnvBufs& b, int E, const uint8_t* pool, uint8_t* ring,
                        int R, int64_t* counters, hipStream_t s, int frame84 = 0);
// screen of frame env.frame[(HIST-1)&1][e] of the pool into all HIST ring slots of env e
int a3c_env_init_screens_launch(const EnvBufs& b, int E, const uint8_t* pool, uint8_t* ring, int R, hipStream_t s);
// Agent.play's bookkeeping of one wave of episodes (agent.py:351-391), one entry per env: the raw
// reward sum (agent.py:377), the steps taken, whether the episode reached a terminal, and the
// frozen flag (done, or no episode in this wave) double-buffered by the wave's step parity --
// step t reads frozen[(t & 1) * E + e], k_play_observe writes frozen[((t + 1) & 1) * E + e]
struct PlayBook {
  float* ret;
  int32_t* len;
  uint8_t* term;
  uint8_t* frozen;
};
// start of a wave: new_random_game of envs e < n_active, their first screen into the HIST newest
// ring slots, bookkeeping zeroed, the other envs frozen, counters[0] = tau
int a3c_play_begin_launch(const EnvParams& p, const EnvBufs& b, int E, int n_active, int64_t tau, const PlayBook& bk,
                          const uint8_t* pool, uint8_t* ring, int R, int64_t* counters, int frame84, hipStream_t s);
// Play with refill (a3c_engine_play_ex, refill = 1): an env whose episode ends takes the next
// unassigned episode in the same step.  ep_idx / tstart are per env, sched is four words, the
// ep_* arrays are per episode ([n_episode]: the per-env PlayBook words only hold the episode in
// progress).  tstart and the next index are double-buffered by the run step's parity, as
// PlayBook::frozen is: step t reads copy t & 1 and writes the other.
struct PlayRefill {
  int32_t* ep_idx;         // [E] the episode env e plays (stale once the env is idle)
  int32_t* tstart;         // [2][E] the run step env e's episode started at
  int32_t* sched;          // [0], [1] next unassigned idx (by parity), [2] episodes not finished, [3] steps with a live env
  float* ep_ret;           // [n_episode] return
  int32_t* ep_len;         // [n_episode] length
  uint8_t* ep_term;        // [n_episode] ended at a terminal (not at the n_step cap)
  int32_t* ep_env;         // [n_episode] the env that played it
  int64_t* ep_tau0;        // [n_episode] tau of its first step
  int n_episode, n_step;
};
// start of a refill run, behind a3c_play_begin_launch(n_active = min(E, n_episode)): episode e on
// env e, sched = {n_active, n_active, n_episode, 0}
int a3c_play_refill_begin_launch(const PlayRefill& rf, int E, int n_active, int64_t tau, hipStream_t s);
// run step t's observe + refill in one launch (k_play_observe_refill; tau = HIST-1 + t): the
// refilled envs' first screens go into the HIST newest ring slots of the next step, their LSTM h / c
// (h_dst, c_dst: the copy the next step reads; nullptr without the LSTM head) are zeroed
int a3c_play_refill_launch(const EnvParams& p, const EnvBufs& b, const PlayBook& bk, const PlayRefill& rf, int E, int t,
                           int64_t tau, const float* rraw, const uint8_t* terms, int64_t* counters, const uint8_t* pool,
                           uint8_t* ring, int R, int frame84, const float* h_src, const float* c_src, float* h_dst,
                           float* c_dst, hipStream_t s);
int a3c_env_screen_launch(int E, const int32_t* frames, const uint8_t* pool, uint8_t* ring, int R,
                          const int64_t* counters, int t, hipStream_t s);
