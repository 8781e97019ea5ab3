// The C5 LSTM head's three matrix passes on gfx950's bf16 matrix cores (A3C_PREC_BF16 as
// NetLayout::lstm_prec): single bf16 operands rounded to nearest even (v_cvt_pk_bf16_f32),
// v_mfma_f32_16x16x32_bf16, fp32 accumulation.  Parameters, the carried and saved state, the
// elementwise cell update and cell backward, masks and the bias gradient stay fp32 (lstm.hip's).
//
//  k_lstm_prep_bf       once per parameter version, into the 2 MB of the fp32 transpose: rn(W)^T
//                       [1024][512] (k-contiguous for the forward) and rn(W) [512][1024] (W's rows
//                       are already k-contiguous for the BPTT product).
//  k_lstm_fwd_bf        k_lstm_fwd's split (16 envs x 16 units x 4 gates, 8 waves = gate x K half,
//                       cell update in the epilogue); the [x, h_prev] rows are rounded once where
//                       they are staged into LDS (16.5 KB against 32.5), the wave's W fragment is
//                       8 16-byte loads a lane, 8 MFMAs a wave in two chains.
//  k_lstm_bptt_step_bf  k_lstm_bptt_step's split (16 envs x 32 columns, 8 waves = column half x
//                       K quarter) and epilogue; da_{t+1} is rounded as it is loaded (DA stays fp32).
//  k_lstm_dw_bf         dW = rn([x, hp])^T rn(da), K = n*E unsplit, + db = column sums of the
//                       unrounded da, one launch: 32 x 64 tiles (256 workgroups), K slices of 64
//                       rounded at the LDS store with the next slice's loads in flight, the n operand
//                       first in the MFMA so every store is 16 bytes a lane.  No atomics.
#include "lstm.h"

typedef float lb_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 lb_b2 __attribute__((ext_vector_type(2)));
typedef uint32_t lb_u4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t lb_pk(float x0, float x1) {   // (rn(x0), rn(x1)) as one dword
  const lb_f2 v = {x0, x1};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, lb_b2));
}
__device__ inline lb_u4 lb_pk8(const f32x4 a, const f32x4 b) {   // eight consecutive k
  return (lb_u4){lb_pk(a[0], a[1]), lb_pk(a[2], a[3]), lb_pk(b[0], b[1]), lb_pk(b[2], b[3])};
}
#define LB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define LB_HALF ((int64_t)LSTM_K * LSTM_G)   // bf16 elements of one prepared copy

// a 32 k x 64 c tile of W through LDS: rn(W) rows straight out (8 lanes a 128-byte run), the
// transposed rows after the barrier (4 lanes a 64-byte run)
__global__ void __launch_bounds__(256) k_lstm_prep_bf(const float* __restrict__ W, uint16_t* __restrict__ prep) {
  __shared__ float tile[32][65];
  const int tid = threadIdx.x, c0 = blockIdx.x * 64, k0 = blockIdx.y * 32;
  {
    const int row = tid >> 3, c8 = (tid & 7) * 8;
    const float* p = W + (int64_t)(k0 + row) * LSTM_G + c0 + c8;
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tile[row][c8 + i] = a[i];
      tile[row][c8 + 4 + i] = b[i];
    }
    ST_WT_R(*(lb_u4*)(prep + LB_HALF + (int64_t)(k0 + row) * LSTM_G + c0 + c8), lb_pk8(a, b));
  }
  __syncthreads();
  const int c = tid >> 2, kq = (tid & 3) * 8;
  f32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = tile[kq + i][c];
    b[i] = tile[kq + 4 + i][c];
  }
  ST_WT_R(*(lb_u4*)(prep + (int64_t)(c0 + c) * LSTM_K + k0 + kq), lb_pk8(a, b));
}

int a3c_lstm_prep_bf_launch(const float* W, uint16_t* prep, hipStream_t s) {
  static_assert(LSTM_G % 64 == 0 && LSTM_K % 32 == 0, "whole tiles");
  hipLaunchKernelGGL(k_lstm_prep_bf, dim3(LSTM_G / 64, LSTM_K / 32), dim3(256), 0, s, W, prep);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// cell step: k_lstm_fwd's workgroup (16 envs x 16 units x 4 gates, wave = (gate g, K half kh), the fc
// fold in slice order + bias + ReLU with l3_out unrounded from unit tile 0, the h half of terminal or
// absent envs zeroed after the product: rn(keep h) = keep rn(h)); the staged rows and W are bf16
#define LB_LD (FC + 8)            // bf16 per LDS row: 528 B, row r starts 4 r banks on
__global__ void __launch_bounds__(512) k_lstm_fwd_bf(const float* __restrict__ X, const float* __restrict__ bias,
                                                     LstmStep st, int64_t B) {
  __shared__ __attribute__((aligned(16))) uint16_t As[2][LT][LB_LD];
  __shared__ float Gs[2][4][LT][LT + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = w & 3, kh = w >> 2, i16 = lane & 15, j4 = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * LT;
  const int u0 = blockIdx.y * LT;
  const uint16_t* pw = (const uint16_t*)st.wt + (int64_t)(g * LSTM_U + u0 + i16) * LSTM_K + kh * FC + 8 * j4;
  bf16x8 b[FC / 32];
#pragma unroll
  for (int it = 0; it < FC / 32; ++it) b[it] = *(const bf16x8*)(pw + 32 * it);
  // stage [x, h_prev] of the tile's 16 envs: 2 x 16 x 64 chunks of 4 floats, 4 per thread
  constexpr int NCH = 2 * LT * (FC / 4);
  static_assert(NCH == 4 * 512 && LSTM_U == FC, "tile staging");
  f32x4 xin[2], hin[2];
  if (st.fc_part) {
    f32x4 p[2][FC_NS];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + 512 * q, row = c >> 6, c4 = c & 63;
      const int64_t e = min(e0 + row, B - 1);
#pragma unroll
      for (int x = 0; x < FC_NS; ++x) p[q][x] = *(const f32x4*)(st.fc_part + ((int64_t)x * B + e) * FC + 4 * c4);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + 512 * q, row = c >> 6, c4 = c & 63;
      const int64_t e = min(e0 + row, B - 1);
      hin[q] = *(const f32x4*)(st.h_src + e * FC + 4 * c4);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + 512 * q, row = c >> 6, c4 = c & 63;
      const f32x4 fb = *(const f32x4*)(st.fc_bias + 4 * c4);
      f32x4 v = p[q][0];
#pragma unroll
      for (int x = 1; x < FC_NS; ++x) v += p[q][x];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r] + fb[r], 0.f);
      xin[q] = v;
      if (blockIdx.y == 0 && e0 + row < B) *(f32x4*)(st.l3_out + (e0 + row) * FC + 4 * c4) = v;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + 512 * q, row = c >> 6, c4 = c & 63;
      const int64_t e = min(e0 + row, B - 1);
      xin[q] = *(const f32x4*)(X + e * FC + 4 * c4);
      hin[q] = *(const f32x4*)(st.h_src + e * FC + 4 * c4);
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 512 * q, row = c >> 6, c4 = c & 63;
    *(uint2*)&As[0][row][4 * c4] = make_uint2(lb_pk(xin[q][0], xin[q][1]), lb_pk(xin[q][2], xin[q][3]));
    *(uint2*)&As[1][row][4 * c4] = make_uint2(lb_pk(hin[q][0], hin[q][1]), lb_pk(hin[q][2], hin[q][3]));
  }
  __syncthreads();
  // lane (i16, j4): A[env i16][k 8 j4 ..], B[k 8 j4 ..][unit i16] -> acc[r] at (env 4 j4 + r, unit i16)
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const uint16_t* ar = &As[kh][i16][8 * j4];
#pragma unroll
  for (int it = 0; it < FC / 32; it += 2) {
    acc0 = LB_MFMA(*(const bf16x8*)(ar + 32 * it), b[it], acc0);
    acc1 = LB_MFMA(*(const bf16x8*)(ar + 32 * it + 32), b[it + 1], acc1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = acc0[r] + acc1[r];
    if (kh) {
      const int64_t e = e0 + 4 * j4 + r;
      if (e >= B || (st.prev_terms && st.prev_terms[e])) v = 0.f;
    }
    Gs[kh][g][4 * j4 + r][i16] = v;
  }
  __syncthreads();
  if (tid >= LT * LT) return;
  // cell update of (env r, unit c)
  const int r = tid >> 4, c = tid & 15;
  const int64_t e = e0 + r;
  if (e >= B) return;
  const int u = u0 + c;
  const int64_t o = e * LSTM_U + u;
  const bool keep = !(st.prev_terms && st.prev_terms[e]);
  const float cprev = keep ? st.c_src[o] : 0.f;
  float pre[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) pre[q] = Gs[0][q][r][c] + Gs[1][q][r][c] + bias[q * LSTM_U + u];
  const float ig = sigmoidf_(pre[0]);
  const float jg = tanhf(pre[1]);
  const float fg = sigmoidf_(pre[2] + 1.0f);     // forget_bias = 1.0
  const float og = sigmoidf_(pre[3]);
  const float cn = cprev * fg + ig * jg;
  const float hn = tanhf(cn) * og;
  if (st.hp) st.hp[o] = keep ? st.h_src[o] : 0.f;
  if (st.cp) st.cp[o] = cprev;
  if (st.gates) {
    float* gp = st.gates + e * LSTM_G + u;
    gp[0] = ig;
    gp[LSTM_U] = jg;
    gp[2 * LSTM_U] = fg;
    gp[3 * LSTM_U] = og;
  }
  st.c[o] = cn;
  st.h[o] = hn;
}

int a3c_lstm_fwd_bf_launch(const float* bias, const float* x, const LstmStep& st, int64_t B, hipStream_t s) {
  if (B <= 0) return 0;
  if (!st.wt || !bias || !st.h_src || !st.c_src || !st.h || !st.c || (!x && !st.fc_part) ||
      (st.fc_part && (!st.fc_bias || !st.l3_out)) ||
      (((uintptr_t)x | (uintptr_t)st.h_src | (uintptr_t)st.wt | (uintptr_t)st.fc_part | (uintptr_t)st.fc_bias) & 15))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_lstm_step", "bad argument");
  hipLaunchKernelGGL(k_lstm_fwd_bf, dim3((unsigned)((B + LT - 1) / LT), LSTM_U / LT), dim3(512), 0, s, x, bias, st, B);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// d[x, hp]_{t+1} = rn(da_{t+1}) rn(W)^T for 16 envs x 32 of the 512 columns, 8 waves = (16-column half
// ct, K quarter kq of 256 = 8 MFMA steps); W: the prepared [512][1024] copy; k_lstm_bptt_step's epilogue
__global__ void __launch_bounds__(512) k_lstm_bptt_step_bf(int64_t E, const uint16_t* __restrict__ W, BpttStep q) {
  __shared__ float Ps[4][2][LT][LT + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ct = w & 1, kq = w >> 1, i16 = lane & 15, j4 = lane >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * LT;
  const int n0 = blockIdx.y * 32;
  const int64_t er = min(e0 + i16, E - 1);
  constexpr int KQ = LSTM_G / 4;                 // 256
  const float* pa = q.DAn + er * LSTM_G + kq * KQ + 8 * j4;
  const uint16_t* pb = W + (int64_t)(n0 + 16 * ct + i16) * LSTM_G + kq * KQ + 8 * j4;   // B^T rows = W rows
  f32x4 a[KQ / 16];
  bf16x8 b[KQ / 32];
#pragma unroll
  for (int it = 0; it < KQ / 32; ++it) {
    a[2 * it] = *(const f32x4*)(pa + 32 * it);
    a[2 * it + 1] = *(const f32x4*)(pa + 32 * it + 4);
    b[it] = *(const bf16x8*)(pb + 32 * it);
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < KQ / 32; it += 2) {
    acc0 = LB_MFMA(__builtin_bit_cast(bf16x8, lb_pk8(a[2 * it], a[2 * it + 1])), b[it], acc0);
    acc1 = LB_MFMA(__builtin_bit_cast(bf16x8, lb_pk8(a[2 * it + 2], a[2 * it + 3])), b[it + 1], acc1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) Ps[kq][ct][4 * j4 + r][i16] = acc0[r] + acc1[r];
  __syncthreads();
  const int r = tid >> 5, c = tid & 31;
  const int64_t e = e0 + r;
  if (e >= E) return;
  const float v = (Ps[0][c >> 4][r][c & 15] + Ps[1][c >> 4][r][c & 15]) +
                  (Ps[2][c >> 4][r][c & 15] + Ps[3][c >> 4][r][c & 15]);
  const int col = n0 + c;
  if (col < FC) {
    const int64_t xi = e * FC + col;
    q.dxn[xi] = q.xn[xi] > 0.f ? v : 0.f;
  } else if (q.cell) {
    const int u = col - FC;
    const float keep = q.terms[e] ? 0.f : 1.f;     // the carry into step t+1 was zeroed
    const int64_t i = e * LSTM_U + u;
    lstm_cell_bwd(e, u, q.dH[i] + keep * v, keep * q.dcp[i], q.G, q.C, q.CP, q.dcp, q.DA);
  }
}

// dW[m][n] = sum_k rn(A[k][m]) rn(da[k][n]), A = x (m < 256) or hp, k over the n*E samples.  Workgroup:
// 32 m x 64 n, wave (wm, wn) the 16 x 32 block as two MFMA tiles.  Both operands arrive as rows of k:
// a thread loads quads of rows k and k + 1 and stores packed (k, k + 1) dwords into [row][k] tiles
// (72 bf16 a row); rows past K are zero.  Grid x = the n tile: the workgroups of one XCD (id & 7)
// share two n tiles' da columns, the large operand.  The m-tile-0 workgroups add the unrounded da
// they load: per k pair over the slices in order, then the 32 pairs in order.
#define DW_MT 32
#define DW_NT 64
#define DW_BK 64
#define DW_LD 72
struct LstmDw {
  const float *x, *hp, *da;
  float *dw, *db;
  int K;
};
__global__ void __launch_bounds__(256) k_lstm_dw_bf(LstmDw a) {
  __shared__ __attribute__((aligned(16))) uint16_t Ms[DW_MT][DW_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ns[DW_NT][DW_LD];
  static_assert(sizeof(Ns) >= 512 * 4 * sizeof(float), "the column partials fit the n tile");
  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 7, wn = (tid >> 6) & 1, i16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * DW_NT, m0 = blockIdx.y * DW_MT, K = a.K;
  const float* A = (m0 < FC ? a.x + m0 : a.hp + (m0 - FC)) + 4 * (tid & 7);   // (both [K][256])
  const float* Bp = a.da + n0;
  const bool do_colsum = blockIdx.y == 0;     // (block-uniform)
  f32x4 ra[2], rb[4];
  float cs[2][4] = {};
  auto load = [&](int k0) {
    const int k = k0 + 2 * (tid >> 3);
    ra[0] = ra[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (k < K) ra[0] = *(const f32x4*)(A + (int64_t)k * FC);
    if (k + 1 < K) ra[1] = *(const f32x4*)(A + (int64_t)(k + 1) * FC);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = tid + 256 * j, kb = k0 + 2 * (p >> 4);
      const float* q = Bp + (int64_t)kb * LSTM_G + 4 * (p & 15);
      rb[2 * j] = rb[2 * j + 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kb < K) rb[2 * j] = *(const f32x4*)q;
      if (kb + 1 < K) rb[2 * j + 1] = *(const f32x4*)(q + LSTM_G);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int c = 0; c < 4; ++c) *(uint32_t*)&Ms[4 * (tid & 7) + c][2 * (tid >> 3)] = lb_pk(ra[0][c], ra[1][c]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = tid + 256 * j;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        *(uint32_t*)&Ns[4 * (p & 15) + c][2 * (p >> 4)] = lb_pk(rb[2 * j][c], rb[2 * j + 1][c]);
        if (do_colsum) cs[j][c] += rb[2 * j][c] + rb[2 * j + 1][c];
      }
    }
  };
  f32x4 acc[2] = {};
  load(0);
  store();
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += DW_BK) {
    const bool more = k0 + DW_BK < K;
    if (more) load(k0 + DW_BK);
#pragma unroll
    for (int ks = 0; ks < DW_BK / 32; ++ks) {
      const bf16x8 mf = *(const bf16x8*)&Ms[wm * 16 + i16][32 * ks + 8 * g];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[ni] = LB_MFMA(*(const bf16x8*)&Ns[wn * 32 + 16 * ni + i16][32 * ks + 8 * g], mf, acc[ni]);
    }
    __syncthreads();
    if (more) {
      store();
      __syncthreads();
    }
  }
  // the n operand went first: acc[ni][c] is (m = .. + i16, n = .. + 4 g + c), 16 bytes a lane
  const int m = m0 + wm * 16 + i16;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    ST_WT_G(*(f32x4*)(a.dw + (int64_t)m * LSTM_G + n0 + wn * 32 + 16 * ni + 4 * g), acc[ni]);
  if (do_colsum) {   // (the loop ended on a barrier)
    float* red = (float*)&Ns[0][0];
#pragma unroll
    for (int j = 0; j < 2; ++j) *(f32x4*)&red[(tid + 256 * j) * 4] = (f32x4){cs[j][0], cs[j][1], cs[j][2], cs[j][3]};
    __syncthreads();
    if (tid < DW_NT) {
      float sum = 0.f;
      for (int kp = 0; kp < DW_BK / 2; ++kp) sum += red[(kp * 16 + (tid >> 2)) * 4 + (tid & 3)];
      a.db[n0 + tid] = sum;
    }
  }
}

static int bptt_step_bf(int t, int64_t E, const BpttStep& b, const void* W, hipStream_t s) {
  // t = -1: dx_0 only (x half of the columns)
  hipLaunchKernelGGL(k_lstm_bptt_step_bf, dim3((unsigned)((E + LT - 1) / LT), (t >= 0 ? LSTM_K : FC) / 32), dim3(512), 0,
                     s, E, (const uint16_t*)W, b);
  A3C_CHECK(hipGetLastError());
  return 0;
}

int a3c_lstm_bptt_bf_launch(const uint16_t* prep, int n, int64_t E, const LstmSeq& q, const float* dh, float* dx,
                            float* dw, float* db, float* ws, hipStream_t s, int parts) {
  if (n < 1 || E < 1 || E > 0x7fffffff / 8) return a3c_set_error(A3C_ERR_INVALID, "a3c_lstm_bptt", "bad shape");
  if (parts & LSTM_BPTT_CHAIN)
    if (int rc = a3c_lstm_bptt_chain(n, E, q, dh, dx, ws, s, bptt_step_bf, prep + LB_HALF)) return rc;
  if (!(parts & LSTM_BPTT_DW)) return 0;
  static_assert(LSTM_G % DW_NT == 0 && LSTM_K % DW_MT == 0 && FC % DW_MT == 0, "whole tiles, none across x | hp");
  const LstmDw a = {q.x, q.hp, ws, dw, db, (int)(n * E)};   // (da: the first block of ws)
  hipLaunchKernelGGL(k_lstm_dw_bf, dim3(LSTM_G / DW_NT, LSTM_K / DW_MT), dim3(256), 0, s, a);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---- C-ABI ------------------------------------------------------------------------------
static int lstm_prec_ok(int precision, const char* what) {
  if (precision != A3C_PREC_FP32 && precision != A3C_PREC_BF16)
    return a3c_set_error(A3C_ERR_INVALID, what, "precision: A3C_PREC_FP32 or A3C_PREC_BF16");
  return 0;
}

extern "C" int a3c_lstm_prepare(const float* w, void* w_prep, int precision, void* stream) {
  if (int rc = lstm_prec_ok(precision, "a3c_lstm_prepare")) return rc;
  if (!w || !w_prep || ((uintptr_t)w | (uintptr_t)w_prep) & 15)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_lstm_prepare", "null or unaligned");
  return precision == A3C_PREC_BF16 ? a3c_lstm_prep_bf_launch(w, (uint16_t*)w_prep, (hipStream_t)stream)
                                    : a3c_lstm_transpose_launch(w, (float*)w_prep, (hipStream_t)stream);
}

extern "C" int a3c_lstm_step_prec(const void* w_prep, const float* b, const float* x, const float* h_src,
                                  const float* c_src, const uint8_t* prev_terms, int64_t B, float* hp, float* cp,
                                  float* gates, float* h, float* c, const float* fc_part, const float* fc_bias,
                                  float* l3_out, int precision, void* stream) {
  static_assert(FC_NS == A3C_LSTM_FC_PARTS, "the header's count of fc partials");
  if (int rc = lstm_prec_ok(precision, "a3c_lstm_step_prec")) return rc;
  if (B < 0) return a3c_set_error(A3C_ERR_INVALID, "a3c_lstm_step_prec", "B < 0");
  LstmStep st = {(const float*)w_prep, h_src, c_src, prev_terms, hp, cp, gates, h, c};
  st.fc_part = fc_part; st.fc_bias = fc_bias; st.l3_out = l3_out;
  return precision == A3C_PREC_BF16 ? a3c_lstm_fwd_bf_launch(b, x, st, B, (hipStream_t)stream)
                                    : a3c_lstm_fwd_launch(b, x, st, B, (hipStream_t)stream);
}

extern "C" int a3c_lstm_bptt_prec(const void* w, int n, int64_t E, const float* x, const float* hp, const float* cp,
                                  const float* gates, const float* c, const uint8_t* terms, const float* dh,
                                  float* dx, float* dw, float* db, void* workspace, int precision, void* stream) {
  if (int rc = lstm_prec_ok(precision, "a3c_lstm_bptt_prec")) return rc;
  if (!w || !x || !hp || !cp || !gates || !c || !terms || !dh || !dx || !dw || !db || !workspace || ((uintptr_t)w & 15))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_lstm_bptt_prec", "null or unaligned argument");
  float* ws = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  LstmSeq q = {x, hp, cp, gates, c, terms};
  return precision == A3C_PREC_BF16
             ? a3c_lstm_bptt_bf_launch((const uint16_t*)w, n, E, q, dh, dx, dw, db, ws, (hipStream_t)stream)
             : a3c_lstm_bptt_launch((const float*)w, n, E, q, dh, dx, dw, db, ws, (hipStream_t)stream);
}
