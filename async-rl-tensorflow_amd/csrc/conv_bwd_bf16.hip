// The NIPS trunk's fused conv backward in bf16 compute mode: k_conv_bwd_bf.
//
// k_conv_bwd's contract (net_bwd.hip) -- one workgroup per group of samples, the same BwdPlan, the same
// per-workgroup slab (dW1 unscaled by 1/255, dW2, db1, db2), so k_slab_group, k_finalize, the norms and
// the clip run unchanged behind it -- with every product on v_mfma_f32_16x16x32_bf16: both operands
// rounded to nearest even once (rn), fp32 accumulators carried over the workgroup's samples, the ReLU mask
// and the two bias sums from the unrounded values.  One variant: 4 waves, for sync and overlap launches.
//
//  (a) dW2[(kh,kw,ci)][co] += sum_q rn(l1[2oy+kh][2ox+kw][ci]) rn(dl2[q][co])       M 256, N 32, K 81 -> 160
//  (b) dl1 = col2im(rn(dl2) rn(W2)^T) * (l1 > 0) per stride-2 parity class (wave = class (py, px)):
//      100 positions in 7 M-tiles, K = 2x2 taps x 32 co = 128
//  (c) dW1[(kh,kw,cin)][c1] += sum_p x[4py+kh][4px+kw][cin] rn(dl1[p][c1])           M 256, N 16, K 400 -> 480
//      (x: the u8 plane, exact in bf16; one term of dl1 where k_conv_bwd multiplies three)
//
// MFMA fragments (16x16x32): A lane (m = lane & 15, g = lane >> 4) holds A[m][8 g .. 8 g + 7], B lane
// (n = lane & 15, g) holds B[8 g .. 8 g + 7][n], D lane holds D[4 g + r][n], r = 0..3.  Every operand is
// therefore stored in LDS with its K index contiguous, 16 bytes per lane and K step:
//
//  l1p   rn(l1) for (a)'s A operand and (b)'s mask.  [ci][y][par][xh]: column x = 2 xh + par, rows of 12
//        bf16 (10 used), 976 bytes per ci (40 rows + 16).  (a)'s K order is k = 16 oy + ox (ox 9..15 and
//        row oy = 9 are padding): a lane's 8 k are ox = ox0 .. ox0 + 7 (ox0 = 0 or 8) of one output row, at
//        columns 2 ox + kw = entries ox + (kw >> 1) of parity kw & 1.  One aligned read of 5 dwords (entries
//        ox0 .. ox0 + 9) per parity feeds kw = par as it stands and kw = par + 2 shifted by one entry
//        (v_alignbit).  Entries past a row's 10 are the next row's or padding: finite, and their k has a
//        zero in the B operand.  An exact zero of l1 is stored as -0: the product is unchanged and the
//        sign bit is the ReLU mask of the unrounded value (a positive l1 that rounds to zero stays +0).
//        The 976-byte ci stride puts the ci lanes of a read 52 dwords apart: 160 modelled cycles a sample
//        and wave against 320 at 960 bytes (the floor is 60; not tuned further).
//  dl2t  rn(dl2)^T for (a)'s B operand: [co][k] in rows of 176 bf16 (160 used; 88 dwords: every lane group of a
//        ds_read_b128 covers the 64 banks once -- rows of 160 or 168 take two passes).  The padding k stay zero
//        from the start.
//  dl2r  rn(dl2) for (b)'s A operand: [q][co] in rows of 40 bf16 (32 used; 20 dwords: 234 modelled cycles a
//        sample against 272 unpadded), row 81 zero for the taps that fall off the 9x9 grid.
//  dlb   rn(dl1) for (c)'s B operand: [c1][k], k = 24 oy + ox (ox 20..23 zero from the start) in 16-byte
//        slots placed by dlb_slot, k_conv_bwd's layout for one term.
//  x8    the sample's four u8 planes, DMA'd global -> LDS under (a) and (b).
// tools/lds_bank_sim.py --bf16 prints the modelled LDS-array cycles of these reads.
//
// Nothing overlays: (b) writes dlb while (a)'s operands are still live, so a sample takes three barriers
// (LDS free, staging done, dl1 + x8 complete).  The next sample's l1 and dl2 rows are loaded into
// registers right after the staging and held across the three phases.
#include "net.h"
#include "net_bwd.h"

#define BF_L1_CI 976                              // bytes per ci of l1p
#define BF_L1_ROW 24                              // bytes per (y, par) row: 12 bf16
#define BF_L1P (C1_N * BF_L1_CI + 16)             // 15632
#define BF_D2T_ROW 352                            // bytes per co of dl2t: 176 bf16
#define BF_D2T (C2_N * BF_D2T_ROW)                // 11264
#define BF_D2R_ROW 80                             // bytes per q of dl2r: 40 bf16
#define BF_D2R ((C2_Q + 1) * BF_D2R_ROW)          // 6560
#define BF_DLB_LD 480                             // bf16 per c1 of dlb
#define BF_DLB (C1_N * BF_DLB_LD * 2)             // 15360
#define BF_X8 (HIST * PLANE)                      // 28224
#define BF_RED (256 * 16)                         // 4096: the bias partials at the end
static_assert(BF_X8 + BF_L1P + BF_D2T + BF_D2R + BF_DLB + BF_RED == CB_BF_SMEM, "LDS of k_conv_bwd_bf");
static_assert(BF_X8 % 16 == 0 && BF_L1P % 16 == 0 && BF_D2T % 16 == 0 && BF_D2R % 16 == 0, "16-byte regions");

__device__ inline int bf_dlb_slot(int G, int n) { return 4 * (G >> 2) + ((G + ((n >> 1) & 2)) & 3); }
__device__ inline uint32_t bf_rn(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
__device__ inline uint32_t bf_rn2(float lo, float hi) { return bf_rn(lo) | (bf_rn(hi) << 16); }
// rn(l1) with an exact zero as -0 (the mask bit of l1p)
__device__ inline uint32_t bf_rn_l1(float v) { return v > 0.f ? bf_rn(v) : 0x8000u; }
__device__ inline bf16x8 bf_frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(bf16x8, make_uint4(a, b, c, d));
}
__device__ inline void bf_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
k_conv_bwd_bf(StateAddr sa, int64_t B, int per_wg, const float* __restrict__ act_l1, const float* __restrict__ dl2,
              const float* __restrict__ W2, float* __restrict__ slab) {
  WGLOG(6);
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* x8 = smem;
  uint8_t* l1p = x8 + BF_X8;
  uint8_t* dl2t = l1p + BF_L1P;
  uint8_t* dl2r = dl2t + BF_D2T;
  uint16_t* dlb = (uint16_t*)(dl2r + BF_D2R);
  float* red = (float*)((uint8_t*)dlb + BF_DLB);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i16 = lane & 15, j4 = lane >> 4;
  const int64_t tau0 = sa.tau_ptr ? *sa.tau_ptr : 0;
  const int64_t b0 = (int64_t)blockIdx.x * per_wg;
  const int64_t b1 = min(B, b0 + per_wg);
  WG_T0();
  unsigned long long* srec = span_rec(sa, tau0);
  span_begin(srec);

  // every operand region zero once: the padding k of dl2t and dlb, dl2r's off-grid row and l1p's row tails
  // are never written again
  for (int i = tid; i < (BF_L1P + BF_D2T + BF_D2R + BF_DLB) / 16; i += 256) ((uint4*)l1p)[i] = make_uint4(0u, 0u, 0u, 0u);

  // (b): this wave's parity class and its four W2 taps, rounded once:
  // w2b[2 dy + dx] = rn(W2[py + 2 dy][px + 2 dx][ci = i16][co = 8 j4 .. + 7])
  const int py = wid >> 1, px = wid & 1;
  bf16x8 w2b[4];
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    const float* w = W2 + (((py + 2 * (tp >> 1)) * C2_K + px + 2 * (tp & 1)) * C1_N + i16) * C2_N + 8 * j4;
    const f32x4 lo = *(const f32x4*)w, hi = *(const f32x4*)(w + 4);
    w2b[tp] = bf_frag(bf_rn2(lo[0], lo[1]), bf_rn2(lo[2], lo[3]), bf_rn2(hi[0], hi[1]), bf_rn2(hi[2], hi[3]));
  }

  f32x4 accW2[4][2], accW1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) accW2[t][0] = accW2[t][1] = accW1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db1acc = 0.f;
  f32x4 db2acc = {0.f, 0.f, 0.f, 0.f};   // co = 4 (tid & 7) .. + 3 over this thread's rows of dl2

  // Staging tasks.  l1: task i = tid + 256 u < 800 is channels 4 (i & 3) .. + 3 of the columns x = 4 j + par
  // and x + 2 of row y ((i >> 2) = 5 (2 y + par) + j): two f32x4 loads, four dword stores (entries 2 j,
  // 2 j + 1 of a row).  dl2: task i < 648 is co = 4 (i & 7) .. + 3 of position q = i >> 3.
  constexpr int NL1 = 4, ND2 = 3;
  f32x4 rl1[NL1][2], rd2[ND2];
  auto load_sample = [&](int64_t b) {
    const float* gl1 = act_l1 + b * C1_P * C1_N;
    const f32x4* gd2 = (const f32x4*)(dl2 + b * FLAT);
#pragma unroll
    for (int u = 0; u < NL1; ++u) {
      const int i = min(tid + 256 * u, 799), r = i >> 2, yp = r / 5, j = r - 5 * yp;
      const float* g = gl1 + ((yp >> 1) * C1_O + 4 * j + (yp & 1)) * C1_N + 4 * (i & 3);
      rl1[u][0] = *(const f32x4*)g;
      rl1[u][1] = *(const f32x4*)(g + 2 * C1_N);
    }
#pragma unroll
    for (int u = 0; u < ND2; ++u) rd2[u] = gd2[min(tid + 256 * u, C2_Q * 8 - 1)];
  };
  if (b0 < b1) load_sample(b0);

  // (c): wave wid owns the 4 M-tiles (kh = 4 (wid >> 1) + (row >> 2), kw = t + 4 (wid & 1), cin = row & 3)
  const int xoff_c = (i16 & 3) * PLANE + (4 * (wid >> 1) + (i16 >> 2)) * IMG + 4 * (wid & 1);

  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();   // the previous sample's (c) is done with dlb and x8 (first sample: the zeroing)
    // ---- staging: registers -> l1p, dl2t, dl2r; db2 from the unrounded rows ----
#pragma unroll
    for (int u = 0; u < NL1; ++u) {
      const int i = tid + 256 * u;
      if (i < 800) {
        const int r = i >> 2, yp = r / 5, j = r - 5 * yp;
        uint8_t* d = l1p + 4 * (i & 3) * BF_L1_CI + yp * BF_L1_ROW + 4 * j;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          *(uint32_t*)(d + c * BF_L1_CI) = bf_rn_l1(rl1[u][0][c]) | (bf_rn_l1(rl1[u][1][c]) << 16);
      }
    }
#pragma unroll
    for (int u = 0; u < ND2; ++u) {
      const int i = tid + 256 * u;
      if (i < C2_Q * 8) {
        const int q = i >> 3, co = 4 * (i & 7), oy = q / C2_O, k = 16 * oy + q - C2_O * oy;
        const f32x4 v = rd2[u];
        db2acc += v;
        *(uint2*)(dl2r + q * BF_D2R_ROW + 2 * co) = make_uint2(bf_rn2(v[0], v[1]), bf_rn2(v[2], v[3]));
#pragma unroll
        for (int c = 0; c < 4; ++c) *(uint16_t*)(dl2t + (co + c) * BF_D2T_ROW + 2 * k) = (uint16_t)bf_rn(v[c]);
      }
    }
    // the state planes are read in (c) only: DMA them global -> LDS now, under (a) and (b)
#pragma unroll
    for (int c = 0; c < HIST; ++c) {
      const uint8_t* g = state_plane(sa, b, c, tau0);
      for (int ch = wid; ch * 1024 < PLANE; ch += 4) {
        const int off = ch * 1024 + lane * 16;
        if (off < PLANE) glds16(g + off, x8 + c * PLANE + ch * 1024);
      }
    }
    if (b + 1 < b1) load_sample(b + 1);   // held in registers across the three phases
    bf_lds_barrier();                     // staging complete (the DMA and the loads stay in flight)

    // ---- (a): wave = kh, tiles t = kw; chunk c holds output rows 2 c and 2 c + 1 ----
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int oy = min(2 * c + (j4 >> 1), C2_O - 1);   // (row 9: any address, its B operand is zero)
      const uint8_t* ap = l1p + i16 * BF_L1_CI + (2 * (C2_S * oy + wid)) * BF_L1_ROW + 16 * (j4 & 1);
      const uint8_t* bp = dl2t + i16 * BF_D2T_ROW + 64 * c + 16 * j4;
      const bf16x8 bq0 = *(const bf16x8*)bp, bq1 = *(const bf16x8*)(bp + 16 * BF_D2T_ROW);
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const uint2 e01 = *(const uint2*)(ap + par * BF_L1_ROW), e23 = *(const uint2*)(ap + par * BF_L1_ROW + 8);
        const uint32_t e4 = *(const uint32_t*)(ap + par * BF_L1_ROW + 16);
        const bf16x8 a0 = bf_frag(e01.x, e01.y, e23.x, e23.y);
        const bf16x8 a2 = bf_frag(__builtin_amdgcn_alignbit(e01.y, e01.x, 16), __builtin_amdgcn_alignbit(e23.x, e01.y, 16),
                                  __builtin_amdgcn_alignbit(e23.y, e23.x, 16), __builtin_amdgcn_alignbit(e4, e23.y, 16));
        accW2[par][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bq0, accW2[par][0], 0, 0, 0);
        accW2[par][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bq1, accW2[par][1], 0, 0, 0);
        accW2[par + 2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bq0, accW2[par + 2][0], 0, 0, 0);
        accW2[par + 2][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bq1, accW2[par + 2][1], 0, 0, 0);
      }
    }

    // ---- (b): dl1 of class (py, px), 100 positions (ay, cx) in 7 M-tiles; K chunk = tap (dy, dx) ----
#pragma unroll 1
    for (int mt = 0; mt < 7; ++mt) {
      const int pc = min(16 * mt + i16, 99);
      const int ay = pc / 10, cx = pc - 10 * ay;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      bf16x8 av[4];
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) {
        const int dy = tp >> 1, dx = tp & 1;
        // dl2 position (ay - dy, cx - dx); off the 9x9 grid -> the zero row
        const bool v = (dy ? ay > 0 : ay < C2_O) && (dx ? cx > 0 : cx < C2_O);
        const int qq = v ? (ay - dy) * C2_O + cx - dx : C2_Q;
        av[tp] = *(const bf16x8*)(dl2r + qq * BF_D2R_ROW + 16 * j4);
      }
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[tp], w2b[tp], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pr = 16 * mt + 4 * j4 + r;   // D row: this position, channel i16
        if (pr < 100) {
          const int ayr = pr / 10, cxr = pr - 10 * ayr;
          const int y = 2 * ayr + py, x = 2 * cxr + px;
          const uint16_t m = *(const uint16_t*)(l1p + i16 * BF_L1_CI + (2 * y + px) * BF_L1_ROW + 2 * cxr);
          const float g = (m & 0x8000u) ? 0.f : acc[r];   // l1 > 0, from the unrounded value
          db1acc += g;
          const int k = 24 * y + x;
          dlb[i16 * BF_DLB_LD + 8 * bf_dlb_slot(k >> 3, i16) + (k & 7)] = (uint16_t)bf_rn(g);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's x8 DMA landed
    bf_lds_barrier();                                   // dl1 complete, and every wave's x8 DMA

    // ---- (c): 15 K chunks of 32 padded positions; lane group j4 takes the 8 ox of block G = 4 c + j4 =
    // 3 oy + blk.  One dword of x holds the pixels of kw & 3 = 0..3 for one ox: 8 dwords feed the 4 tiles ----
    auto load_chunk = [&](int c, uint32_t (&d)[8], bf16x8& bv) {
      const int G = 4 * c + j4, oy = G / 3, blk = G - 3 * oy;
      const uint32_t* xp = (const uint32_t*)(x8 + xoff_c + 4 * oy * IMG + 32 * blk);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = xp[j];
      bv = *(const bf16x8*)(dlb + i16 * BF_DLB_LD + 8 * bf_dlb_slot(G, i16));
    };
    auto mma_chunk = [&](const uint32_t (&d)[8], const bf16x8& bv) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        uint32_t a[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float f0 = (float)((d[2 * jj] >> (8 * t)) & 255u);
          const float f1 = (float)((d[2 * jj + 1] >> (8 * t)) & 255u);
          a[jj] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
        }
        accW1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf_frag(a[0], a[1], a[2], a[3]), bv, accW1[t], 0, 0, 0);
      }
    };
    uint32_t d0[8], d1[8];
    bf16x8 v0, v1;
    load_chunk(0, d0, v0);
#pragma unroll 1
    for (int c = 0; c < 15; c += 2) {
      const bool has1 = c + 1 < 15;
      if (has1) load_chunk(c + 1, d1, v1);
      mma_chunk(d0, v0);
      if (c + 2 < 15) load_chunk(c + 2, d0, v0);
      if (has1) mma_chunk(d1, v1);
    }
  }

  // ---- this workgroup's partial slab (k_conv_bwd's layout) ----
  float* out = slab + (int64_t)blockIdx.x * CB_SLAB;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int krow = 16 * (4 * wid + t) + 4 * j4 + r;   // dW2 row (kh = wid, kw = t, ci = 4 j4 + r)
      ST_WT_C(out[CB_OFF_W2 + krow * C2_N + i16], accW2[t][0][r]);
      ST_WT_C(out[CB_OFF_W2 + krow * C2_N + 16 + i16], accW2[t][1][r]);
    }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // D row 4 j4 + r of tile t: kh = 4 (wid >> 1) + j4, kw = t + 4 (wid & 1), cin = r
      const int krow = ((4 * (wid >> 1) + j4) * C1_K + t + 4 * (wid & 1)) * HIST + r;
      ST_WT_C(out[CB_OFF_W1 + krow * C1_N + i16], accW1[t][r]);
    }
  // db1: lanes with equal i16 (the 4 j4 groups), then the waves, in a fixed order
  db1acc += __shfl_xor(db1acc, 16, 64);
  db1acc += __shfl_xor(db1acc, 32, 64);
  __syncthreads();
  if (lane < 16) red[wid * 16 + lane] = db1acc;
  __syncthreads();
  if (tid < C1_N) out[CB_OFF_B1 + tid] = ((red[tid] + red[16 + tid]) + red[32 + tid]) + red[48 + tid];
  // db2: the 32 threads that share tid & 7, in thread order
  __syncthreads();
  *(f32x4*)(red + 4 * tid) = db2acc;
  __syncthreads();
  if (tid < C2_N) {
    float v = 0.f;
    for (int g = 0; g < 32; ++g) v += red[4 * (8 * g + (tid >> 2)) + (tid & 3)];
    out[CB_OFF_B2 + tid] = v;
  }
  span_end(srec);
  WG_T1(act_l1 + b0 * C1_P * C1_N);   // debug: over this workgroup's own (consumed) l1 rows
}

int a3c_conv_bwd_bf_launch(const StateAddr& sa, int64_t B, const BwdPlan& p, const float* act_l1, const float* dl2,
                           const float* W2, float* slab, int smem, hipStream_t s) {
  hipLaunchKernelGGL(k_conv_bwd_bf, dim3((unsigned)p.nwg), dim3(256), smem, s, sa, B, p.per_wg, act_l1, dl2, W2, slab);
  A3C_CHECK(hipGetLastError());
  return 0;
}

void a3c_conv_bwd_bf_set_smem(int smem) {
  (void)hipFuncSetAttribute((const void*)k_conv_bwd_bf, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
}
