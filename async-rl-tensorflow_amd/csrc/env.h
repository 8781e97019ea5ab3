#pragma once
#include "net.h"

#define SCREEN_H 210
#define SCREEN_W 160
#define IMG_OUT IMG

struct PreGeom;
PreGeom a3c_make_geom(int in_h, int in_w, int out_h, int out_w);
int a3c_pool_fill_launch(uint8_t* pool, int P, uint32_t k0, uint32_t k1, hipStream_t s,
                         int frame_bytes = SCREEN_H * SCREEN_W * 3);
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
int a3c_env_screen_launch(int E, const int32_t* frames, const uint8_t* pool, uint8_t* ring, int R,
                          const int64_t* counters, int t, hipStream_t s);
