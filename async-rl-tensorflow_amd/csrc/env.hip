// Batched synthetic Atari stand-in on device (gym/ALE is absent; SURVEY §2 OUT OF SCOPE) with the
// reference's interface semantics, bit-identical to oracle/synthetic_env.py:
//   new_game          environment.py:28-33
//   new_random_game   environment.py:35-40
//   act               environment.py:78-96 (action repeat, life-loss terminal when training)
//   observe clip      agent.py:154
// k_env_step fuses one env step with K1 (Environment.screen) and the K2 history push: the new
// 84x84 screen is written straight into the env's frame-ring slot, so the "shift" of
// history.py:13-15 costs nothing (states are read through StateAddr).
#include "env_dev.h"
#include "preprocess_dev.h"
#include "screen_atari.h"

// ---------------------------------------------------------------------------------------------
__global__ void k_pool_fill(uint8_t* __restrict__ pool, int64_t chunks_per_frame, int64_t total_chunks,
                            uint32_t k0, uint32_t k1) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_chunks;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = (uint32_t)(i / chunks_per_frame), j = (uint32_t)(i - (int64_t)f * chunks_per_frame);
    u32x4 x = philox4x32(j, f, P_POOL, 0u, k0, k1);
    ((uint4*)pool)[i] = make_uint4(x.x, x.y, x.z, x.w);
  }
}

// reset every env (state zeroed, lives = 0 so new_game resets), new_random_game, and fill the
// history with HIST copies of the first screen (agent.py:35-38).  tau := HIST-1; the env
// state lives at parity (tau & 1) of the double-buffered state arrays.
// (GAME: A3C_GAME_*; the Catch instantiations of this file's kernels are launched at its end)
template <int GAME = A3C_GAME_SYNTH>
__global__ void k_env_init_state(EnvParams p, EnvBufs b, int E, int64_t* __restrict__ counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) { counters[0] = HIST - 1; counters[1] = 0; counters[2] = 0; }   // tau, global, worker step
  if (e >= E) return;
  EnvState s = {0u, 0u, 0u, 0, 0, 0.f, 0u};
  game_new_random_game<GAME>(s, p, (uint32_t)(p.env_id_base + e));
  env_store(b, (int64_t)((HIST - 1) & 1) * E + e, s);
}

// screen of each env's current frame into all HIST ring slots (grid (parts, E))
__global__ void __launch_bounds__(256) k_env_init_screens(EnvBufs b, int E, const uint8_t* __restrict__ pool,
                                                          uint8_t* __restrict__ ring, int R, PreGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int e = blockIdx.y;
  const int32_t f = b.frame[(int64_t)((HIST - 1) & 1) * E + e];
  uint8_t* base = ring + (int64_t)e * R * PLANE;
  const int64_t fb = (int64_t)g.in_h * g.in_w * 3;
  for (int c = 0; c < HIST; ++c) {
    a3c_preprocess_part(pool + (int64_t)f * fb, base + (int64_t)(c % R) * PLANE, g, blockIdx.x, smem);
    __syncthreads();
  }
}

// screen of env e's post-act frame (written by the fused head+act kernel) into ring slot
// (tau + t + 1) mod R: Environment.screen (environment.py:49-53) + History.add (history.py:13-15).
// grid (bands, E): one output band per workgroup.
template <int ROWS>
__global__ void __launch_bounds__(256) k_env_screen(int E, const int32_t* __restrict__ frames,
                                                    const uint8_t* __restrict__ pool, uint8_t* __restrict__ ring,
                                                    int R, const int64_t* __restrict__ counters, int t) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int e = blockIdx.y;
  const int64_t tau = counters[0] + t;
  atari::screen_band<ROWS>(pool + (int64_t)frames[e] * (atari::IH * atari::IW * 3),
                           ring + (int64_t)e * R * PLANE + ((tau + 1) % R) * PLANE, blockIdx.x, smem);
}

// mode M2 (pre-sized frames): frame f of the pool copied into all HIST ring slots of env e (grid E)
__global__ void __launch_bounds__(256) k_env_init_copy84(EnvBufs b, int E, const uint8_t* __restrict__ pool,
                                                         uint8_t* __restrict__ ring, int R) {
  const int e = blockIdx.x;
  const int32_t f = b.frame[(int64_t)((HIST - 1) & 1) * E + e];
  const uint4* src = (const uint4*)(pool + (int64_t)f * PLANE);
  uint8_t* base = ring + (int64_t)e * R * PLANE;
  for (int i = threadIdx.x; i < PLANE / 16; i += blockDim.x) {
    const uint4 v = src[i];
    for (int c = 0; c < HIST; ++c) ((uint4*)(base + (int64_t)(c % R) * PLANE))[i] = v;
  }
}

// frame f, 16-byte chunk j = philox(j, f, P_POOL, 0): frame_bytes = 210*160*3 (RGB frames) or
// 84*84 (mode M2 -- the first 441 chunks of the same hash)
static int catch_init_state_launch(const EnvParams& p, const EnvBufs& b, int E, int64_t* counters, hipStream_t s);
static int catch_play_begin_state_launch(const EnvParams& p, const EnvBufs& b, int E, int n_active, int64_t tau,
                                         const PlayBook& bk, int64_t* counters, hipStream_t s);
int a3c_pool_fill_launch(uint8_t* pool, int P, uint32_t k0, uint32_t k1, hipStream_t s, int frame_bytes) {
  const int64_t cpf = frame_bytes / 16;
  const int64_t total = cpf * P;
  hipLaunchKernelGGL(k_pool_fill, dim3(4096), dim3(256), 0, s, pool, cpf, total, k0, k1);
  A3C_CHECK(hipGetLastError());
  return 0;
}

int a3c_env_init_launch(const EnvParams& p, const EnvBufs& b, int E, const uint8_t* pool, uint8_t* ring,
                        int R, int64_t* counters, hipStream_t s, int frame84) {
  PreGeom g = a3c_make_geom(SCREEN_H, SCREEN_W, IMG_OUT, IMG_OUT);
  if (p.game == A3C_GAME_CATCH) {
    if (int rc = catch_init_state_launch(p, b, E, counters, s)) return rc;
  } else {
    hipLaunchKernelGGL(k_env_init_state<>, dim3((E + 63) / 64), dim3(64), 0, s, p, b, E, counters);
  }
  A3C_CHECK(hipGetLastError());
  if (frame84) {
    hipLaunchKernelGGL(k_env_init_copy84, dim3(E), dim3(256), 0, s, b, E, pool, ring, R);
    A3C_CHECK(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(k_env_init_screens, dim3(g.parts, E), dim3(256), a3c_pre_smem_bytes(g), s, b, E, pool, ring, R, g);
  A3C_CHECK(hipGetLastError());
  return 0;
}

int a3c_env_init_screens_launch(const EnvBufs& b, int E, const uint8_t* pool, uint8_t* ring, int R, hipStream_t s) {
  PreGeom g = a3c_make_geom(SCREEN_H, SCREEN_W, IMG_OUT, IMG_OUT);
  hipLaunchKernelGGL(k_env_init_screens, dim3(g.parts, E), dim3(256), a3c_pre_smem_bytes(g), s, b, E, pool, ring, R, g);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---- Agent.play (agent.py:351-391): start of a wave of evaluation episodes --------------------
// new_random_game (agent.py:363, environment.py:35-40) of the wave's envs e < n_active only: the
// emulator continues where the env's previous episode stopped (it resets only when lives == 0).
// The play context keeps both parity copies of an env's state equal, so the state is read from
// copy 0 and written to both.  Zeroes the wave's return / length / terminated words, freezes the
// envs without an episode (both parity copies of the flag) and sets the play tau.
template <int GAME = A3C_GAME_SYNTH>
__global__ void k_play_begin(EnvParams p, EnvBufs b, int E, int n_active, int64_t tau, PlayBook bk,
                             int64_t* __restrict__ counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) counters[0] = tau;
  if (e >= E) return;
  const bool active = e < n_active;
  bk.frozen[e] = bk.frozen[E + e] = active ? 0 : 1;
  bk.ret[e] = 0.f;
  bk.len[e] = 0;
  bk.term[e] = 0;
  if (!active) return;
  EnvState s = env_load(b, e);
  game_new_random_game<GAME>(s, p, (uint32_t)(p.env_id_base + e));
  env_store(b, e, s);
  env_store(b, (int64_t)E + e, s);
}

// the first screen of every active env into its HIST newest ring slots, (tau - 3 .. tau) mod R
// (agent.py:366-367); grid (parts, E) as k_env_init_screens, frozen envs' rings untouched
__global__ void __launch_bounds__(256) k_play_begin_screens(EnvBufs b, const uint8_t* __restrict__ frozen,
                                                            const uint8_t* __restrict__ pool,
                                                            uint8_t* __restrict__ ring, int R, int64_t tau, PreGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int e = blockIdx.y;
  if (frozen[e]) return;
  const int32_t f = b.frame[e];
  uint8_t* base = ring + (int64_t)e * R * PLANE;
  const int64_t fb = (int64_t)g.in_h * g.in_w * 3;
  for (int c = 0; c < HIST; ++c) {
    a3c_preprocess_part(pool + (int64_t)f * fb, base + ((tau - (HIST - 1) + c) % R) * PLANE, g, blockIdx.x, smem);
    __syncthreads();
  }
}

// the same for pre-sized 84x84 pool frames (cfg.frame84): a copy (grid E)
__global__ void __launch_bounds__(256) k_play_begin_copy84(EnvBufs b, const uint8_t* __restrict__ frozen,
                                                           const uint8_t* __restrict__ pool,
                                                           uint8_t* __restrict__ ring, int R, int64_t tau) {
  const int e = blockIdx.x;
  if (frozen[e]) return;
  const int32_t f = b.frame[e];
  const uint4* src = (const uint4*)(pool + (int64_t)f * PLANE);
  uint8_t* base = ring + (int64_t)e * R * PLANE;
  for (int i = threadIdx.x; i < PLANE / 16; i += blockDim.x) {
    const uint4 v = src[i];
    for (int c = 0; c < HIST; ++c) ((uint4*)(base + ((tau - (HIST - 1) + c) % R) * PLANE))[i] = v;
  }
}

int a3c_play_begin_launch(const EnvParams& p, const EnvBufs& b, int E, int n_active, int64_t tau, const PlayBook& bk,
                          const uint8_t* pool, uint8_t* ring, int R, int64_t* counters, int frame84, hipStream_t s) {
  if (E < 1 || n_active < 1 || n_active > E || tau < HIST - 1 || R < HIST + 1)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_play_begin", "bad argument");
  if (p.game == A3C_GAME_CATCH) {
    if (int rc = catch_play_begin_state_launch(p, b, E, n_active, tau, bk, counters, s)) return rc;
  } else {
    hipLaunchKernelGGL(k_play_begin<>, dim3((E + 63) / 64), dim3(64), 0, s, p, b, E, n_active, tau, bk, counters);
  }
  A3C_CHECK(hipGetLastError());
  if (frame84) {
    hipLaunchKernelGGL(k_play_begin_copy84, dim3(E), dim3(256), 0, s, b, bk.frozen, pool, ring, R, tau);
  } else {
    PreGeom g = a3c_make_geom(SCREEN_H, SCREEN_W, IMG_OUT, IMG_OUT);
    hipLaunchKernelGGL(k_play_begin_screens, dim3(g.parts, E), dim3(256), a3c_pre_smem_bytes(g), s, b, bk.frozen, pool,
                       ring, R, tau, g);
  }
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---- play with refill: an env whose episode ends takes the next unassigned episode at once ------
static int catch_refill_set_smem();
static int catch_refill_launch(const EnvParams& p, const EnvBufs& b, const PlayBook& bk, const PlayRefill& rf, int E, int t,
                               int64_t tau, const float* rraw, const uint8_t* terms, int64_t* counters,
                               const uint8_t* pool, uint8_t* ring, int R, const float* h_src, const float* c_src,
                               float* h_dst, float* c_dst, hipStream_t s);
// start of the run, behind k_play_begin: episode e on env e < n_active, starting at tau
__global__ void k_play_refill_begin(PlayRefill rf, int E, int n_active, int64_t tau) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) { rf.sched[0] = rf.sched[1] = n_active; rf.sched[2] = rf.n_episode; rf.sched[3] = 0; }
  if (e >= E) return;
  rf.ep_idx[e] = e < n_active ? e : -1;
  rf.tstart[e] = rf.tstart[E + e] = 0;
  if (e < n_active) { rf.ep_env[e] = e; rf.ep_tau0[e] = tau; }
}

// One launch per step t of a refill run, behind the step's head kernel, in the place of
// k_play_observe: workgroup e is env e's observe, refill and first screens.  The play step is
// launch-bound (~9 us per launch at 256 envs), so the refill adds no launch: instead
// of one workgroup scanning the envs and a second kernel drawing the screens, every workgroup
// counts for itself, in chunks of RF_THREADS envs, the envs that end in this step -- those before
// it in env-id order (its rank) and all of them -- from words no workgroup writes in this launch:
//   frozen[par], tstart[par] (the run step the env's episode started at; its length after this step
//   is t + 1 - tstart), sched[par] (the next unassigned index) -- all double-buffered by the step
//   parity, this launch writes copy par ^ 1 -- and terms (the head kernel's).
// Counting is exact whatever the order: no atomics, the same indices on every run.  Then, for a
// live env:
//  * bookkeeping as k_play_observe (return += raw reward, length += 1, agent.py:377-379); the
//    episode ends at a terminal or when its own length reaches n_step (terminated = 0 then), and
//    its words go to the per-episode arrays;
//  * an env that ended takes index next + rank; if that is < n_episode it is refilled:
//    new_random_game (agent.py:363; both parity copies of the state), return / length /
//    terminated zeroed, the schedule record, the frozen flag of the next parity clear, LSTM h, c
//    zeroed in the copy the next step reads, and the new game's first screen into the HIST newest
//    ring slots of the next step, (tau+1-3 .. tau+1) mod R, over the post-terminal screen the step
//    wrote (agent.py:366-367) -- the whole-frame screen of the head kernels (atari::screen_frame,
//    bit-exact Environment.screen: the band kernel of k_play_begin_screens takes 130 us a frame,
//    too long for one workgroup inside a 37 us step) into the newest slot, then copied to the
//    other three; otherwise the env is frozen for good.
// A frozen env's LSTM h, c are carried into the copy the next step reads.  Workgroup 0 advances
// sched (next index, episodes not finished, steps with a live env) and tau.  tau is an argument
// (HIST-1 + t: a refill run's tau has no gaps), since workgroup 0 writes the counter.
#define RF_THREADS 512
template <int GAME = A3C_GAME_SYNTH>
__global__ void __launch_bounds__(RF_THREADS) k_play_observe_refill(EnvParams p, EnvBufs b, PlayBook bk, PlayRefill rf,
                                                             int E, int t, int64_t tau,
                                                             const float* __restrict__ rraw,
                                                             const uint8_t* __restrict__ terms,
                                                             int64_t* __restrict__ counters,
                                                             const uint8_t* __restrict__ pool,
                                                             uint8_t* __restrict__ ring, int R, int frame84,
                                                             const float* __restrict__ h_src,
                                                             const float* __restrict__ c_src, float* __restrict__ h_dst,
                                                             float* __restrict__ c_dst) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int32_t s_frame;
  const int e = blockIdx.x, tid = threadIdx.x, par = t & 1;
  const uint8_t* fz_in = bk.frozen + (int64_t)par * E;
  const int32_t* ts_in = rf.tstart + (int64_t)par * E;
  int rank = 0, total = 0, live_any = 0;
  for (int base = 0; base < E; base += RF_THREADS) {
    const int j = base + tid;
    const bool live = j < E && !fz_in[j];
    const bool ended = live && (terms[j] || t + 1 - ts_in[j] >= rf.n_step);
    rank += __syncthreads_count(ended && j < e);
    total += __syncthreads_count(ended);
    live_any |= __syncthreads_or(live);
  }
  const int next = rf.sched[par];
  if (e == 0 && tid == 0) {
    rf.sched[par ^ 1] = next + total < rf.n_episode ? next + total : rf.n_episode;
    rf.sched[2] -= total;
    rf.sched[3] += live_any ? 1 : 0;
    counters[0] = tau + 1;
  }
  const uint8_t fz = fz_in[e];
  const int32_t ts = ts_in[e];
  if (fz) {
    if (tid == 0) {
      bk.frozen[(int64_t)(par ^ 1) * E + e] = 1;
      rf.tstart[(int64_t)(par ^ 1) * E + e] = ts;
    }
    if (h_dst)
      for (int i = tid; i < LSTM_U; i += RF_THREADS) {
        h_dst[(int64_t)e * LSTM_U + i] = h_src[(int64_t)e * LSTM_U + i];
        c_dst[(int64_t)e * LSTM_U + i] = c_src[(int64_t)e * LSTM_U + i];
      }
    return;
  }
  const bool term = terms[e] != 0;
  const int32_t len = t + 1 - ts;
  const bool ended = term || len >= rf.n_step;
  const int idx = next + rank;
  const bool refill = ended && idx < rf.n_episode;      // (uniform over the workgroup)
  if (tid == 0) {
    const float ret = bk.ret[e] + rraw[e];
    bk.ret[e] = ret;
    bk.len[e] = len;
    if (term) bk.term[e] = 1;
    if (ended) {
      const int32_t old = rf.ep_idx[e];
      rf.ep_ret[old] = ret;
      rf.ep_len[old] = len;
      rf.ep_term[old] = term ? 1 : 0;
    }
    if (refill) {
      EnvState s = env_load(b, e);
      game_new_random_game<GAME>(s, p, (uint32_t)(p.env_id_base + e));
      env_store(b, e, s);
      env_store(b, (int64_t)E + e, s);
      s_frame = s.frame;
      bk.ret[e] = 0.f;
      bk.len[e] = 0;
      bk.term[e] = 0;
      rf.ep_idx[e] = idx;
      rf.ep_env[idx] = e;
      rf.ep_tau0[idx] = tau + 1;
    }
    bk.frozen[(int64_t)(par ^ 1) * E + e] = ended && !refill ? 1 : 0;
    rf.tstart[(int64_t)(par ^ 1) * E + e] = refill ? t + 1 : ts;
  }
  if (!refill) return;
  __syncthreads();
  if (h_dst)
    for (int i = tid; i < LSTM_U; i += RF_THREADS) h_dst[(int64_t)e * LSTM_U + i] = c_dst[(int64_t)e * LSTM_U + i] = 0.f;
  const int32_t f = s_frame;
  uint8_t* base = ring + (int64_t)e * R * PLANE;
  uint8_t* newest = base + ((tau + 1) % R) * PLANE;
  if (frame84)
    atari::copy_frame84<RF_THREADS>(pool + (int64_t)f * PLANE, newest);
  else
    atari::screen_frame<RF_THREADS>(pool + (int64_t)f * (atari::IH * atari::IW * 3), newest, smem, nullptr);
  __syncthreads();                           // the newest slot is written: copy it to the three before it
  for (int i = tid; i < PLANE / 16; i += RF_THREADS) {
    const uint4 v = ((const uint4*)newest)[i];
    for (int c = 0; c < HIST - 1; ++c) ((uint4*)(base + ((tau + 1 - (HIST - 1) + c) % R) * PLANE))[i] = v;
  }
}

int a3c_play_refill_begin_launch(const PlayRefill& rf, int E, int n_active, int64_t tau, hipStream_t s) {
  if (E < 1 || n_active < 1 || n_active > E || n_active > rf.n_episode || rf.n_step < 1)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_play_refill_begin", "bad argument");
  A3C_CHECK(hipFuncSetAttribute((const void*)k_play_observe_refill<>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                SCREEN_FRAME_SMEM));
  if (int rc = catch_refill_set_smem()) return rc;
  hipLaunchKernelGGL(k_play_refill_begin, dim3((E + 63) / 64), dim3(64), 0, s, rf, E, n_active, tau);
  A3C_CHECK(hipGetLastError());
  return 0;
}

int a3c_play_refill_launch(const EnvParams& p, const EnvBufs& b, const PlayBook& bk, const PlayRefill& rf, int E, int t,
                           int64_t tau, const float* rraw, const uint8_t* terms, int64_t* counters, const uint8_t* pool,
                           uint8_t* ring, int R, int frame84, const float* h_src, const float* c_src, float* h_dst,
                           float* c_dst, hipStream_t s) {
  if (E < 1 || R < HIST + 1 || t < 0 || tau < HIST - 1)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_play_refill", "bad argument");
  if (p.game == A3C_GAME_CATCH)     // (never with frame84: a3c_engine_create rejects the pair)
    return catch_refill_launch(p, b, bk, rf, E, t, tau, rraw, terms, counters, pool, ring, R, h_src, c_src, h_dst, c_dst, s);
  hipLaunchKernelGGL(k_play_observe_refill<>, dim3(E), dim3(RF_THREADS), frame84 ? 0 : SCREEN_FRAME_SMEM, s, p, b, bk, rf, E,
                     t, tau, rraw, terms, counters, pool, ring, R, frame84, h_src, c_src, h_dst, c_dst);
  A3C_CHECK(hipGetLastError());
  return 0;
}

template <int ROWS>
static void launch_env_screen(int E, const int32_t* frames, const uint8_t* pool, uint8_t* ring, int R,
                              const int64_t* counters, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_env_screen<ROWS>, dim3((atari::OH + ROWS - 1) / ROWS, E), dim3(256),
                     atari::Smem<ROWS>::BYTES, s, E, frames, pool, ring, R, counters, t);
}

int a3c_env_screen_launch(int E, const int32_t* frames, const uint8_t* pool, uint8_t* ring, int R,
                          const int64_t* counters, int t, hipStream_t s) {
  switch (a3c_screen_rows()) {
    case 7: launch_env_screen<7>(E, frames, pool, ring, R, counters, t, s); break;
    case 21: launch_env_screen<21>(E, frames, pool, ring, R, counters, t, s); break;
    case 28: launch_env_screen<28>(E, frames, pool, ring, R, counters, t, s); break;
    case 42: launch_env_screen<42>(E, frames, pool, ring, R, counters, t, s); break;
    case 12: launch_env_screen<12>(E, frames, pool, ring, R, counters, t, s); break;
    default: launch_env_screen<14>(E, frames, pool, ring, R, counters, t, s); break;
  }
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Catch (A3C_GAME_CATCH): the pool render kernel and the GAME = A3C_GAME_CATCH
// instantiations of this file's kernels, emitted behind the default-game ones.
// ---------------------------------------------------------------------------------------------
// Frames 0 .. CATCH_FRAMES-1 of the RGB pool, frame f = (c * CATCH_ROWS + r) * CATCH_COLS + p: black,
// the ball's cell (rows [21 r, 21 r + 21) x cols [20 c, 20 c + 20)) in (236,236,236), then the
// paddle (rows [200, 210) x cols [20 p, 20 p + 20)) in (92,186,92) over it.  One 16-byte chunk per
// thread and pass; frames >= CATCH_FRAMES of a larger pool are never read and stay as they are.
// visible_rows (EnvParams.catch_visible): the ball's cell is drawn only in the frames of
// ball rows r < visible_rows (10: every frame); the paddle always is.
#define CATCH_CELL_W (SCREEN_W / CATCH_COLS)      // 20
#define CATCH_CELL_H (SCREEN_H / CATCH_ROWS)      // 21
#define CATCH_PADDLE_Y (SCREEN_H - 10)            // 200
static_assert(CATCH_CELL_W * CATCH_COLS == SCREEN_W && CATCH_CELL_H * CATCH_ROWS == SCREEN_H, "Catch cells tile the screen");
__global__ void __launch_bounds__(256) k_pool_render_catch(uint8_t* __restrict__ pool, int visible_rows) {
  constexpr int64_t CPF = SCREEN_H * SCREEN_W * 3 / 16;   // 6300 chunks per frame
  constexpr int64_t TOTAL = CPF * CATCH_FRAMES;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < TOTAL; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i / CPF), j = (int)(i - (int64_t)f * CPF);
    const int p = f % CATCH_COLS, r = (f / CATCH_COLS) % CATCH_ROWS, c = f / (CATCH_COLS * CATCH_ROWS);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int byte = 16 * j + k, pix = byte / 3, ch = byte - 3 * pix;
      const int y = pix / SCREEN_W, x = pix - y * SCREEN_W;
      uint32_t v = 0u;
      if (r < visible_rows && y / CATCH_CELL_H == r && x / CATCH_CELL_W == c) v = 236u;
      if (y >= CATCH_PADDLE_Y && x / CATCH_CELL_W == p) v = ch == 1 ? 186u : 92u;
      w[k >> 2] |= v << (8 * (k & 3));
    }
    ((uint4*)pool)[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// P: the pool's frame count (>= CATCH_FRAMES, or nothing is written)
int a3c_pool_render_catch_launch(uint8_t* pool, int P, int visible_rows, hipStream_t s) {
  if (!pool || P < CATCH_FRAMES) return a3c_set_error(A3C_ERR_INVALID, "a3c_pool_render_catch", "the pool holds fewer than 640 frames");
  hipLaunchKernelGGL(k_pool_render_catch, dim3(4096), dim3(256), 0, s, pool, visible_rows);
  A3C_CHECK(hipGetLastError());
  return 0;
}

static int catch_init_state_launch(const EnvParams& p, const EnvBufs& b, int E, int64_t* counters, hipStream_t s) {
  hipLaunchKernelGGL(k_env_init_state<A3C_GAME_CATCH>, dim3((E + 63) / 64), dim3(64), 0, s, p, b, E, counters);
  return 0;
}

static int catch_play_begin_state_launch(const EnvParams& p, const EnvBufs& b, int E, int n_active, int64_t tau,
                                         const PlayBook& bk, int64_t* counters, hipStream_t s) {
  hipLaunchKernelGGL(k_play_begin<A3C_GAME_CATCH>, dim3((E + 63) / 64), dim3(64), 0, s, p, b, E, n_active, tau, bk,
                     counters);
  return 0;
}

static int catch_refill_set_smem() {
  A3C_CHECK(hipFuncSetAttribute((const void*)k_play_observe_refill<A3C_GAME_CATCH>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, SCREEN_FRAME_SMEM));
  return 0;
}

static int catch_refill_launch(const EnvParams& p, const EnvBufs& b, const PlayBook& bk, const PlayRefill& rf, int E, int t,
                               int64_t tau, const float* rraw, const uint8_t* terms, int64_t* counters,
                               const uint8_t* pool, uint8_t* ring, int R, const float* h_src, const float* c_src,
                               float* h_dst, float* c_dst, hipStream_t s) {
  hipLaunchKernelGGL(k_play_observe_refill<A3C_GAME_CATCH>, dim3(E), dim3(RF_THREADS), SCREEN_FRAME_SMEM, s, p, b, bk, rf,
                     E, t, tau, rraw, terms, counters, pool, ring, R, 0, h_src, c_src, h_dst, c_dst);
  A3C_CHECK(hipGetLastError());
  return 0;
}
