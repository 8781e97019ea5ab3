// The NIPS trunk's two fc backward GEMMs on gfx950's bf16 matrix cores (A3C_PREC_BF16 as
// NetLayout::fcbwd_prec): both operands rounded to nearest-even bf16 once, where they are
// staged (v_cvt_pk_bf16_f32), one v_mfma_f32_16x16x32_bf16 per K step, fp32 accumulation.  l2, dl3,
// dl2 and the parameters stay fp32; Wfc is rounded from the fp32 parameters at its LDS store (no
// prepared copy).  The MFMA takes the n operand first, so a lane's four accumulators are four
// consecutive n of one row m and every store is 16 bytes per lane.  No atomics: every sum has one order
// that depends on B alone.
//
//  k_fc_dw_bf   dWfc[2592][256] = rn(l2)^T rn(dl3), K = B.  A workgroup owns a 32 x 64 tile (81 strips x
//               4 column tiles: 2592 = 81 * 32, no ragged M) and splits K over its 4 waves: wave w takes
//               the 32-sample slices w, w + 4, w + 8, .. and multiplies the whole tile (2 x 4 MFMA tiles)
//               over them out of its own 7,680 B of LDS, with no workgroup barrier in the loop and two
//               slices of global loads in flight per wave (8 per workgroup).  Both operands arrive with
//               the sample as the strided index and are transposed into k-contiguous rows as packed
//               (k, k + 1) dwords.  Samples past B are operand zeros; every wave runs the same number of
//               slices.  The 4 partial tiles are folded through LDS in wave order, then stored once.
//               The 4 column tiles of a strip take consecutive workgroups of one XCD (they share the
//               l2 strip); strip 0's also sum the unrounded dl3 columns: the bias gradient.
//  k_fc_dx_bf   dl2[B][2592] = (rn(dl3) rn(Wfc)^T) * (l2 > 0), K = 256 staged whole.  A wave holds its
//               32 sample rows of rn(dl3) as MFMA fragments for the workgroup's life (64 VGPRs); the
//               workgroup (4 waves, 128 rows) walks a range of 32-column chunks of Wfc (a contiguous
//               32 KB of the parameters each), rounded into a double-buffered LDS chunk: the next chunk's
//               global loads are in flight under the MFMAs and the masked stores, one barrier a chunk.
//               The mask is the forward's ReLU bits (one word per row and chunk) or the fp32 l2 quads,
//               loaded before the chunk's products.
#include "net_bwd.h"

typedef float fb_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 fb_b2 __attribute__((ext_vector_type(2)));
typedef uint32_t fb_u4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t fb_pk(float x0, float x1) {   // (rn(x0), rn(x1)) as one dword
  const fb_f2 v = {x0, x1};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, fb_b2));
}

// ---------------------------------------------------------------------------------------
// dW
// ---------------------------------------------------------------------------------------
#define FW_MT 32               // tile rows (l2 columns)
#define FW_NT 64               // tile columns (dl3 columns)
#define FW_KS 32               // samples per slice: one MFMA K step
#define FW_LD 40               // bf16 per staged row (32 + 8: 80 B, 16-byte aligned fragments)
#define FW_G 4                 // K groups = waves
#define FW_STRIPS (FLAT / FW_MT)
#define FW_NTILES (FC / FW_NT)
#define FW_STAGE ((FW_MT + FW_NT) * FW_LD * 2)    // 7680 B per wave
#define FW_SMEM (FW_G * FW_MT * FW_NT * 4)        // 32768 B: the fold's 4 partial tiles (the stages overlay them)
static_assert(FLAT % FW_MT == 0 && FC % FW_NT == 0 && FW_NTILES == 4, "whole tiles; 4 column tiles an XCD round");
static_assert(FW_G * FW_STAGE <= FW_SMEM && FW_SMEM <= 48 * 1024, "LDS budget beside the rollout");

struct FwRegs {
  f32x4 a[4], b[8];   // l2: 2 (k, k + 1) quad pairs; dl3: 4
};

// slice s of a wave: lane pair p = lane + 64 j is samples 32 s + 2 (p >> 3) and + 1, l2 columns m0 + 4 (p & 7)
// (dl3: 2 (p >> 4), columns n0 + 4 (p & 15)); samples past B are zeros
__device__ inline void fw_load(const float* __restrict__ l2, const float* __restrict__ dl3, int B, int m0, int n0,
                               int s, int lane, FwRegs& r) {
  const int k0 = s * FW_KS;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = lane + 64 * j, k = k0 + 2 * (p >> 3);
    const float* q = l2 + (int64_t)k * FLAT + m0 + 4 * (p & 7);
    r.a[2 * j] = r.a[2 * j + 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (k < B) r.a[2 * j] = *(const f32x4*)q;
    if (k + 1 < B) r.a[2 * j + 1] = *(const f32x4*)(q + FLAT);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = lane + 64 * j, k = k0 + 2 * (p >> 4);
    const float* q = dl3 + (int64_t)k * FC + n0 + 4 * (p & 15);
    r.b[2 * j] = r.b[2 * j + 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (k < B) r.b[2 * j] = *(const f32x4*)q;
    if (k + 1 < B) r.b[2 * j + 1] = *(const f32x4*)(q + FC);
  }
}

// one slice of the wave: round its registers into the wave's stage, then the tile's 8 MFMAs out of it.  The
// stage is the wave's own: LDS operations of one wave execute in order, so no workgroup barrier stands here
__device__ inline void fw_slice(uint16_t (*Ms)[FW_LD], uint16_t (*Ns)[FW_LD], int lane, const FwRegs& r,
                                f32x4 (&acc)[2][4], bool do_cs, float (&cs)[4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = lane + 64 * j;
#pragma unroll
    for (int c = 0; c < 4; ++c) *(uint32_t*)&Ms[4 * (p & 7) + c][2 * (p >> 3)] = fb_pk(r.a[2 * j][c], r.a[2 * j + 1][c]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = lane + 64 * j;
#pragma unroll
    for (int c = 0; c < 4; ++c) *(uint32_t*)&Ns[4 * (p & 15) + c][2 * (p >> 4)] = fb_pk(r.b[2 * j][c], r.b[2 * j + 1][c]);
    if (do_cs)
#pragma unroll
      for (int c = 0; c < 4; ++c) cs[c] += r.b[2 * j][c] + r.b[2 * j + 1][c];
  }
  __builtin_amdgcn_wave_barrier();
  const int i16 = lane & 15, g = lane >> 4;
  bf16x8 mf[2], nf[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) mf[i] = *(const bf16x8*)&Ms[16 * i + i16][8 * g];
#pragma unroll
  for (int i = 0; i < 4; ++i) nf[i] = *(const bf16x8*)&Ns[16 * i + i16][8 * g];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf[ni], mf[mi], acc[mi][ni], 0, 0, 0);
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256) k_fc_dw_bf(const float* __restrict__ l2, const float* __restrict__ dl3, int B,
                                                  float* __restrict__ dW, float* __restrict__ colsum) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[FW_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // workgroup id -> XCD id & 7 (the dispatcher's round-robin); on it, 4 consecutive workgroups are one strip's column tiles
  const int id = blockIdx.x, j = id >> 3;
  const int strip = (j >> 2) * 8 + (id & 7), n0 = (j & 3) * FW_NT;
  if (strip >= FW_STRIPS) return;
  const int m0 = strip * FW_MT;
  const bool do_cs = strip == 0;     // (block-uniform)
  uint16_t(*Ms)[FW_LD] = (uint16_t(*)[FW_LD])(smem + w * FW_STAGE);
  uint16_t(*Ns)[FW_LD] = Ms + FW_MT;
  // every wave runs 2 * pairs slices: those past the last sample load nothing and multiply zeros
  const int pairs = ((B + FW_KS - 1) / FW_KS + 2 * FW_G - 1) / (2 * FW_G);
  float cs[4] = {};
  f32x4 acc[2][4] = {};
  FwRegs r0, r1;
  fw_load(l2, dl3, B, m0, n0, w, lane, r0);
  fw_load(l2, dl3, B, m0, n0, w + FW_G, lane, r1);
  for (int t = 0; t < pairs; ++t) {
    const int s = w + 2 * FW_G * t;
    const FwRegs c0 = r0;
    fw_load(l2, dl3, B, m0, n0, s + 2 * FW_G, lane, r0);
    fw_slice(Ms, Ns, lane, c0, acc, do_cs, cs);
    const FwRegs c1 = r1;
    fw_load(l2, dl3, B, m0, n0, s + 3 * FW_G, lane, r1);
    fw_slice(Ms, Ns, lane, c1, acc, do_cs, cs);
  }
  // the fold: partial tiles [wave][32][64] over the stages, summed in wave order
  float* red = (float*)smem;
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      *(f32x4*)&red[w * (FW_MT * FW_NT) + (16 * mi + (lane & 15)) * FW_NT + 16 * ni + 4 * (lane >> 4)] = acc[mi][ni];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = tid + 256 * i;
    f32x4 v = *(const f32x4*)&red[4 * q];
#pragma unroll
    for (int g = 1; g < FW_G; ++g) v += *(const f32x4*)&red[g * (FW_MT * FW_NT) + 4 * q];
    ST_WT_G(*(f32x4*)(dW + (int64_t)(m0 + (q >> 4)) * FC + n0 + 4 * (q & 15)), v);
  }
  if (do_cs) {   // per-lane partials (a lane's samples in order), then wave by wave, sample-pair group by group
    __syncthreads();
    *(f32x4*)&red[4 * tid] = (f32x4){cs[0], cs[1], cs[2], cs[3]};
    __syncthreads();
    if (tid < FW_NT) {
      float sum = 0.f;
      for (int g = 0; g < 16; ++g) sum += red[(16 * g + (tid >> 2)) * 4 + (tid & 3)];
      colsum[n0 + tid] = sum;
    }
  }
}

// ---------------------------------------------------------------------------------------
// dX
// ---------------------------------------------------------------------------------------
#define FX_ROWS 128            // sample rows per workgroup: 32 per wave
#define FX_NC 32               // dl2 columns (Wfc rows) per chunk: one mask word
#define FX_CHUNKS (FLAT / FX_NC)
#define FX_LD (FC + 8)         // bf16 per staged Wfc row (528 B: 16-byte aligned fragments)
#define FX_SMEM (2 * FX_NC * FX_LD * 2)   // 33792 B
static_assert(FLAT % FX_NC == 0 && FX_NC == 32 && FC % 32 == 0, "whole chunks, one mask word each");
static_assert(FX_SMEM <= 48 * 1024, "LDS budget beside the rollout");

template <bool BITS>
__global__ void __launch_bounds__(256) k_fc_dx_bf(const float* __restrict__ dl3, const float* __restrict__ W,
                                                  const float* __restrict__ l2, const uint32_t* __restrict__ bits, int B,
                                                  int cpw, float* __restrict__ dl2) {
  __shared__ __attribute__((aligned(16))) uint16_t Ws[2][FX_NC][FX_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * cpw, nch = min(cpw, FX_CHUNKS - c0);
  const int mrow = blockIdx.y * FX_ROWS + w * 32 + i16;   // and + 16
  // the wave's rows of rn(dl3): fragment (mi, ks) is row mrow + 16 mi, k 32 ks + 8 g .. + 7
  bf16x8 af[2][FC / 32];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ks = 0; ks < FC / 32; ++ks) {
      f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
      if (mrow + 16 * mi < B) {
        const float* q = dl3 + (int64_t)(mrow + 16 * mi) * FC + 32 * ks + 8 * g;
        x0 = *(const f32x4*)q;
        x1 = *(const f32x4*)(q + 4);
      }
      const fb_u4 u = {fb_pk(x0[0], x0[1]), fb_pk(x0[2], x0[3]), fb_pk(x1[0], x1[1]), fb_pk(x1[2], x1[3])};
      af[mi][ks] = __builtin_bit_cast(bf16x8, u);
    }
  // a chunk is FX_NC whole rows of Wfc: 8192 contiguous floats, quad tid + 256 i of them per thread
  f32x4 r[8];
  auto load = [&](int c) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = *(const f32x4*)(W + (int64_t)c * (FX_NC * FC) + 4 * (tid + 256 * i));
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = tid + 256 * i;
      *(uint2*)&Ws[buf][q >> 6][4 * (q & 63)] = make_uint2(fb_pk(r[i][0], r[i][1]), fb_pk(r[i][2], r[i][3]));
    }
  };
  load(c0);
  store(0);
  __syncthreads();
  for (int ci = 0; ci < nch; ++ci) {
    const int c = c0 + ci, buf = ci & 1;
    const bool more = ci + 1 < nch;     // (block-uniform)
    if (more) load(c + 1);
    uint32_t mw[2] = {0u, 0u};
    f32x4 mq[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int m = mrow + 16 * mi;
      if (BITS) {
        if (m < B) mw[mi] = bits[(int64_t)m * FX_CHUNKS + c];
      } else {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          mq[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (m < B) mq[mi][ni] = *(const f32x4*)(l2 + (int64_t)m * FLAT + c * FX_NC + 16 * ni + 4 * g);
        }
      }
    }
    f32x4 acc[2][2] = {};
#pragma unroll
    for (int ks = 0; ks < FC / 32; ++ks) {
      bf16x8 nf[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) nf[ni] = *(const bf16x8*)&Ws[buf][16 * ni + i16][32 * ks + 8 * g];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf[ni], af[mi][ks], acc[mi][ni], 0, 0, 0);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int m = mrow + 16 * mi;
      if (m >= B) continue;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        f32x4 v = acc[mi][ni];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const bool keep = BITS ? ((mw[mi] >> (16 * ni + 4 * g + cc)) & 1u) != 0 : mq[mi][ni][cc] > 0.f;
          v[cc] = keep ? v[cc] : 0.f;
        }
        ST_WT_G(*(f32x4*)(dl2 + (int64_t)m * FLAT + c * FX_NC + 16 * ni + 4 * g), v);
      }
    }
    if (more) store(buf ^ 1);   // (last read before the barrier that ended chunk ci - 1)
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
int a3c_fc_dw_bf_launch(const float* l2, const float* dl3, int64_t B, float* dW, float* colsum, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_dw_bf, dim3((FW_STRIPS + 7) / 8 * 8 * FW_NTILES), dim3(256), 0, s, l2, dl3, (int)B, dW, colsum);
  A3C_CHECK(hipGetLastError());
  return 0;
}

int a3c_fc_dx_bf_launch(const float* dl3, const float* W, const float* l2, const uint32_t* l2bits, int64_t B, float* dl2,
                        hipStream_t s) {
  // column ranges of whole chunks, as many as give about one workgroup per CU (speed only: K is whole in every one)
  const int rb = (int)((B + FX_ROWS - 1) / FX_ROWS);
  const int want = (256 + rb - 1) / rb < FX_CHUNKS ? (256 + rb - 1) / rb : FX_CHUNKS;
  const int cpw = FX_CHUNKS / want;
  const dim3 grid((FX_CHUNKS + cpw - 1) / cpw, rb);
  if (l2bits)
    hipLaunchKernelGGL(k_fc_dx_bf<true>, grid, dim3(256), 0, s, dl3, W, l2, l2bits, (int)B, cpw, dl2);
  else
    hipLaunchKernelGGL(k_fc_dx_bf<false>, grid, dim3(256), 0, s, dl3, W, l2, l2bits, (int)B, cpw, dl2);
  A3C_CHECK(hipGetLastError());
  return 0;
}

extern "C" int a3c_fc_bwd_bf16(const float* l2, const float* dl3, const float* Wfc, const float* mask_f32,
                               const uint32_t* maskbits, int64_t B, float* dW, float* colsum, float* dl2, void* stream) {
  // one pass alone (the timing tool): dW and colsum both null -- dX only; dl2 null -- dW only, no mask
  const bool dw = dW || colsum, dx = dl2 != nullptr;
  if (!l2 || !dl3 || !Wfc || (!dw && !dx) || (dw && (!dW || !colsum)) || B <= 0 || B > 0x7fffffff / FLAT)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_fc_bwd_bf16", "null pointer or B out of range");
  if (dx ? (mask_f32 != nullptr) == (maskbits != nullptr) : mask_f32 || maskbits)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_fc_bwd_bf16", "exactly one of mask_f32 and maskbits (none without dl2)");
  if ((((uintptr_t)l2 | (uintptr_t)dl3 | (uintptr_t)Wfc | (uintptr_t)mask_f32 | (uintptr_t)dW | (uintptr_t)dl2) & 15) ||
      (((uintptr_t)maskbits | (uintptr_t)colsum) & 3))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_fc_bwd_bf16", "matrices must be 16-byte aligned");
  int rc = dw ? a3c_fc_dw_bf_launch(l2, dl3, B, dW, colsum, (hipStream_t)stream) : 0;
  if (!rc && dx) rc = a3c_fc_dx_bf_launch(dl3, Wfc, mask_f32, maskbits, B, dl2, (hipStream_t)stream);
  return rc;
}
