// The nature trunk's fc 3136 -> 512 on gfx950's bf16 matrix cores (A3C_PREC_BF16 as NetLayout::fc_prec,
// DESIGN §4p): the forward and the two backward GEMMs with both operands rounded to nearest-even
// bf16 where they are staged into LDS (v_cvt_pk_bf16_f32), one product per K step, fp32
// accumulation.  Parameters, saved activations, bias, ReLU, masks and the bias column sums stay fp32;
// W4 is rounded from the fp32 parameters at the LDS store (no prepared copy).
//
// Shared by the three passes: 256 threads, a 64 x 64 output tile, wave w the 32 x 32 block
// (w >> 1, w & 1) as 2 x 2 v_mfma_f32_16x16x32_bf16 tiles; K slices of 64 staged k-contiguous
// ([row][k], 72 bf16 a row, 18432 B of LDS for both operands, one buffer: room beside the other
// stream's workgroups), the next slice's global loads in flight in registers under the MFMAs.  The
// MFMA takes the n operand first: a lane's four accumulators are then four consecutive n of one
// row m, so every store is 16 bytes per lane and a 16-lane group writes 64 contiguous bytes, with
// no LDS round trip.  No atomics: every reduction has one fixed order.
//
//  k_nat_fc_fwd   l4 = relu(rn(l3) rn(W4) + b4).  M = B is short and K = 3136 long: K is split over
//                 grid z into up to 7 chunks of whole slices, each into its own slab of the forward
//                 workspace, and k_nat_fc_fold adds them in chunk order with bias + ReLU (one chunk:
//                 the epilogue is in the tile).  l3 arrives k-contiguous; W4[k][n] arrives along n and
//                 is loaded as quad pairs at k and k + 1, stored as packed (k, k + 1) dwords.
//  k_nat_fc_dw    dW4 = rn(l3)^T rn(dl4) straight into grads, K = the samples unsplit (no slab), both
//                 operands as quad pairs of sample rows.  The 8 n tiles of an m tile share its l3
//                 columns (the large operand) and take consecutive workgroups of one XCD.  The
//                 m tile 0 workgroups also sum the unrounded dl4 columns: the bias gradient.
//  k_nat_fc_dx    dl3 = (rn(dl4) rn(W4)^T) * (l3 > 0): K = 512, both operands k-contiguous as stored;
//                 the mask quads are loaded before the K loop, the stores are the pass's traffic.
#include "nature.h"

typedef float fc_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 fc_b2 __attribute__((ext_vector_type(2)));
#define FC_T 64          // tile rows and columns
#define FC_BK 64         // K slice
#define FC_LD 72         // bf16 per LDS row (64 + 8: 144 B, 16-byte aligned fragments)
#define FC_FWD_SPLIT 7   // 49 slices: 7 chunks of 7
typedef uint16_t FcTile[FC_T][FC_LD];

__device__ inline uint32_t fc_pk(float x0, float x1) {   // (rn(x0), rn(x1)) as one dword
  const fc_f2 v = {x0, x1};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, fc_b2));
}

// a 64-row x 64-k tile of an operand that is contiguous along k: quad i of a thread is row
// (tid + 256 i) >> 4, k 4 ((tid + 256 i) & 15); rows past `rows` are zero
__device__ inline void fc_load_kc(const float* __restrict__ src, int64_t ld, int row0, int rows, int k0, int tid,
                                  f32x4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + 256 * i, row = row0 + (q >> 4);
    r[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (row < rows) r[i] = *(const f32x4*)(src + (int64_t)row * ld + k0 + 4 * (q & 15));
  }
}
__device__ inline void fc_store_kc(FcTile& t, int tid, const f32x4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + 256 * i;
    *(uint2*)&t[q >> 4][4 * (q & 15)] = make_uint2(fc_pk(r[i][0], r[i][1]), fc_pk(r[i][2], r[i][3]));
  }
}
// a 64-k x 64-column tile of an operand whose rows are the k index: pair j of a thread is the quads
// at rows k0 + 2 (p >> 4) and + 1, columns col0 + 4 (p & 15), p = tid + 256 j; rows past kend are zero
__device__ inline void fc_load_rows(const float* __restrict__ src, int64_t ld, int col0, int k0, int kend, int tid,
                                    f32x4 (&r)[4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = tid + 256 * j, k = k0 + 2 * (p >> 4);
    const float* q = src + (int64_t)k * ld + col0 + 4 * (p & 15);
    r[2 * j] = r[2 * j + 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (k < kend) r[2 * j] = *(const f32x4*)q;
    if (k + 1 < kend) r[2 * j + 1] = *(const f32x4*)(q + ld);
  }
}
__device__ inline void fc_store_rows(FcTile& t, int tid, const f32x4 (&r)[4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = tid + 256 * j;
#pragma unroll
    for (int c = 0; c < 4; ++c) *(uint32_t*)&t[4 * (p & 15) + c][2 * (p >> 4)] = fc_pk(r[2 * j][c], r[2 * j + 1][c]);
  }
}

// one staged slice: acc[mi][ni][c] += at m = 16 mi + (lane & 15), n = 16 ni + 4 (lane >> 4) + c of the wave's block
__device__ inline void fc_mma(const FcTile& Ms, const FcTile& Ns, int wm, int wn, int lane, f32x4 (&acc)[2][2]) {
  const int i16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < FC_BK / 32; ++ks) {
    bf16x8 mf[2], nf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      mf[i] = *(const bf16x8*)&Ms[wm * 32 + 16 * i + i16][32 * ks + 8 * g];
      nf[i] = *(const bf16x8*)&Ns[wn * 32 + 16 * i + i16][32 * ks + 8 * g];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf[ni], mf[mi], acc[mi][ni], 0, 0, 0);
  }
}

// the K loop over [kbeg, kend): load(k0, ra, rb) fills a slice's registers, store(ra, rb) rounds them
// into the one LDS buffer (two barriers a slice), slice s + 1 loading while slice s multiplies
template <class Load, class Store>
__device__ inline void fc_loop(int kbeg, int kend, const FcTile& Ms, const FcTile& Ns, int wm, int wn, int lane,
                               f32x4 (&acc)[2][2], Load load, Store store) {
  f32x4 ra[4], rb[4];
  load(kbeg, ra, rb);
  store(ra, rb);
  __syncthreads();
  for (int k0 = kbeg; k0 < kend; k0 += FC_BK) {
    const bool more = k0 + FC_BK < kend;
    if (more) load(k0 + FC_BK, ra, rb);
    fc_mma(Ms, Ns, wm, wn, lane, acc);
    __syncthreads();
    if (more) {
      store(ra, rb);
      __syncthreads();
    }
  }
}

struct FcFwd {
  const float *l3, *W, *bias;
  float *l4, *slab;
  int B, per, nsplit;   // per: K floats per chunk
};
__global__ void __launch_bounds__(256) k_nat_fc_fwd(FcFwd a) {
  __shared__ __attribute__((aligned(16))) FcTile Ms, Ns;
  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 7, wn = (tid >> 6) & 1;
  const int n0 = blockIdx.x * FC_T, m0 = blockIdx.y * FC_T, z = blockIdx.z;
  const int kbeg = z * a.per, kend = min(NT_FLAT, kbeg + a.per);
  f32x4 acc[2][2] = {};
  fc_loop(
      kbeg, kend, Ms, Ns, wm, wn, lane, acc,
      [&](int k0, f32x4(&ra)[4], f32x4(&rb)[4]) {
        fc_load_kc(a.l3, NT_FLAT, m0, a.B, k0, tid, ra);
        fc_load_rows(a.W, NT_FC, n0, k0, kend, tid, rb);
      },
      [&](const f32x4(&ra)[4], const f32x4(&rb)[4]) {
        fc_store_kc(Ms, tid, ra);
        fc_store_rows(Ns, tid, rb);
      });
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + wm * 32 + 16 * mi + (lane & 15);
    if (m >= a.B) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int n = n0 + wn * 32 + 16 * ni + 4 * (lane >> 4);
      f32x4 v = acc[mi][ni];
      if (a.nsplit == 1) {
        const f32x4 b = *(const f32x4*)(a.bias + n);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c] + b[c], 0.f);
        ST_WT_R(*(f32x4*)(a.l4 + (int64_t)m * NT_FC + n), v);
      } else {
        ST_WT_R(*(f32x4*)(a.slab + ((int64_t)z * a.B + m) * NT_FC + n), v);
      }
    }
  }
}
// l4 = relu(slab 0 + slab 1 + .. + bias), one quad per thread
__global__ void __launch_bounds__(256) k_nat_fc_fold(const float* __restrict__ slab, const float* __restrict__ bias,
                                                     float* __restrict__ l4, int64_t quads, int nsplit) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  f32x4 v = *(const f32x4*)(slab + 4 * i);
  for (int s = 1; s < nsplit; ++s) v += *(const f32x4*)(slab + 4 * (s * quads + i));
  const f32x4 b = *(const f32x4*)(bias + 4 * (i % (NT_FC / 4)));
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c] + b[c], 0.f);
  ST_WT_R(*(f32x4*)(l4 + 4 * i), v);
}

#define FC_DW_MT (NT_FLAT / FC_T)   // 49 m tiles
#define FC_DW_NT (NT_FC / FC_T)     // 8 n tiles
static_assert(NT_FLAT % FC_T == 0 && NT_FC % FC_T == 0 && NT_FLAT % FC_BK == 0 && NT_FC % FC_BK == 0, "whole tiles");
static_assert(FC_DW_NT == 8 && FC_T * FC_LD * 2 >= 512 * 4 * 4, "8 n tiles an XCD round; the column partials fit one tile");
__global__ void __launch_bounds__(256) k_nat_fc_dw(const float* __restrict__ l3, const float* __restrict__ dl4, int B,
                                                   float* __restrict__ dW, float* __restrict__ colsum) {
  __shared__ __attribute__((aligned(16))) FcTile Ms, Ns;
  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 7, wn = (tid >> 6) & 1;
  // workgroup id -> XCD id & 7 (the dispatcher's round-robin); on it, 8 consecutive workgroups are one m tile's n tiles
  const int id = blockIdx.x, j = id >> 3;
  const int mt = (j >> 3) * 8 + (id & 7), n0 = (j & 7) * FC_T;
  if (mt >= FC_DW_MT) return;
  const int m0 = mt * FC_T;
  const bool do_colsum = mt == 0;     // (block-uniform)
  float cs[2][4] = {};
  f32x4 acc[2][2] = {};
  fc_loop(
      0, B, Ms, Ns, wm, wn, lane, acc,
      [&](int k0, f32x4(&ra)[4], f32x4(&rb)[4]) {
        fc_load_rows(l3, NT_FLAT, m0, k0, B, tid, ra);
        fc_load_rows(dl4, NT_FC, n0, k0, B, tid, rb);
      },
      [&](const f32x4(&ra)[4], const f32x4(&rb)[4]) {
        fc_store_rows(Ms, tid, ra);
        fc_store_rows(Ns, tid, rb);
        if (do_colsum)
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < 4; ++c) cs[p][c] += rb[2 * p][c] + rb[2 * p + 1][c];
      });
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int m = m0 + wm * 32 + 16 * mi + (lane & 15), n = n0 + wn * 32 + 16 * ni + 4 * (lane >> 4);
      ST_WT_G(*(f32x4*)(dW + (int64_t)m * NT_FC + n), acc[mi][ni]);
    }
  if (do_colsum) {   // per-pair partials through LDS (the loop ended on a barrier), summed over the 32 k pairs in order
    float* red = (float*)&Ms[0][0];
#pragma unroll
    for (int p = 0; p < 2; ++p) *(f32x4*)&red[(tid + 256 * p) * 4] = (f32x4){cs[p][0], cs[p][1], cs[p][2], cs[p][3]};
    __syncthreads();
    if (tid < FC_T) {
      float sum = 0.f;
      for (int kp = 0; kp < FC_BK / 2; ++kp) sum += red[(kp * 16 + (tid >> 2)) * 4 + (tid & 3)];
      colsum[n0 + tid] = sum;
    }
  }
}

__global__ void __launch_bounds__(256) k_nat_fc_dx(const float* __restrict__ dl4, const float* __restrict__ W,
                                                   const float* __restrict__ l3, int B, float* __restrict__ dl3) {
  __shared__ __attribute__((aligned(16))) FcTile Ms, Ns;
  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 7, wn = (tid >> 6) & 1;
  const int n0 = blockIdx.x * FC_T, m0 = blockIdx.y * FC_T;
  const int mrow = m0 + wm * 32 + (lane & 15), ncol = n0 + wn * 32 + 4 * (lane >> 4);
  f32x4 mask[2][2];   // l3 at this lane's outputs, in flight under the K loop
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      mask[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (mrow + 16 * mi < B) mask[mi][ni] = *(const f32x4*)(l3 + (int64_t)(mrow + 16 * mi) * NT_FLAT + ncol + 16 * ni);
    }
  f32x4 acc[2][2] = {};
  fc_loop(
      0, NT_FC, Ms, Ns, wm, wn, lane, acc,
      [&](int k0, f32x4(&ra)[4], f32x4(&rb)[4]) {
        fc_load_kc(dl4, NT_FC, m0, B, k0, tid, ra);
        fc_load_kc(W, NT_FC, n0, NT_FLAT, k0, tid, rb);
      },
      [&](const f32x4(&ra)[4], const f32x4(&rb)[4]) {
        fc_store_kc(Ms, tid, ra);
        fc_store_kc(Ns, tid, rb);
      });
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    if (mrow + 16 * mi >= B) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      f32x4 v = acc[mi][ni];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = mask[mi][ni][c] > 0.f ? v[c] : 0.f;
      ST_WT_G(*(f32x4*)(dl3 + (int64_t)(mrow + 16 * mi) * NT_FLAT + ncol + 16 * ni), v);
    }
  }
}

int a3c_nat_fc_fwd_launch(const float* l3, const float* W, const float* bias, float* l4, int64_t B, float* slab,
                          int max_split, hipStream_t s) {
  const int slices = NT_FLAT / FC_BK;
  const int want = max_split < FC_FWD_SPLIT ? (max_split < 1 ? 1 : max_split) : FC_FWD_SPLIT;
  const int per = (slices + want - 1) / want;
  FcFwd a = {l3, W, bias, l4, slab, (int)B, per * FC_BK, (slices + per - 1) / per};
  if (a.nsplit > 1 && !slab) return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_fc_fwd_launch", "fc: no slab workspace");
  hipLaunchKernelGGL(k_nat_fc_fwd, dim3(FC_DW_NT, (unsigned)((B + FC_T - 1) / FC_T), (unsigned)a.nsplit), dim3(256), 0,
                     s, a);
  A3C_CHECK(hipGetLastError());
  if (a.nsplit > 1) {
    const int64_t quads = B * (NT_FC / 4);
    hipLaunchKernelGGL(k_nat_fc_fold, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, slab, bias, l4, quads,
                       a.nsplit);
    A3C_CHECK(hipGetLastError());
  }
  return 0;
}
int a3c_nat_fc_dw_launch(const float* l3, const float* dl4, int64_t B, float* dW, float* colsum, hipStream_t s) {
  hipLaunchKernelGGL(k_nat_fc_dw, dim3((FC_DW_MT + 7) / 8 * 8 * FC_DW_NT), dim3(256), 0, s, l3, dl4, (int)B, dW, colsum);
  A3C_CHECK(hipGetLastError());
  return 0;
}
int a3c_nat_fc_dx_launch(const float* dl4, const float* W, const float* l3, int64_t B, float* dl3, hipStream_t s) {
  hipLaunchKernelGGL(k_nat_fc_dx, dim3(FC_DW_MT, (unsigned)((B + FC_T - 1) / FC_T)), dim3(256), 0, s, dl4, W, l3,
                     (int)B, dl3);
  A3C_CHECK(hipGetLastError());
  return 0;
}
