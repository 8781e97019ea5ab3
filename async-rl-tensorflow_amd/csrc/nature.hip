// The "nature" trunk of the reference's A3C Network (network.py:30-42: conv 8x8/4 32, conv 4x4/2
// 64, conv 3x3/1 64, fc 3136 -> 512, all ReLU; heads network.py:60-79) on gfx950's bf16 matrix
// cores.  The reference computes in fp32: the fp32 mode splits every fp32 operand into three
// round-to-nearest bf16 terms and sums six products (fp32-class results); the bf16 compute mode
// (A3C_PREC_BF16) rounds each operand once.  What runs (DESIGN §4d has the measurements
// of the forms that lost: the fp32 MFMA tiles, per-layer forward passes, a fused dX, the fc on
// these tiles -- all removed):
//
//  k_nat_w_terms<NT>   the prepared block: the conv weights as bf16 terms [term][cout][k], once per
//                      rollout (a3c_nat_prep_launch) or into the workspace of a per-op call
//  k_nat_conv23        fp32 mode: conv1 + conv2 + conv3 forward of one state per workgroup, the
//                      activations kept in LDS as terms between the layers (launched as NAT_C2F)
//  k_nat_conv123_b1    the same in the bf16 mode, one term per operand
//  k_nat_gemm_bf<MODE, LAYER, BN, TA, TB, NBUF, PF>
//                      the implicit-GEMM tile kernel of the conv backward passes, operands gathered
//                      straight from the NHWC activations (no im2col buffer in HBM), split into
//                      TA / TB terms at the LDS store, reduced on v_mfma_f32_32x32x16_bf16.  4 waves,
//                      each a 32x32 block of a 64x64 (BN = 64) or 128x32 (BN = 32) tile.
//    NG_DX    dX = col2im(dY W^T) * (X > 0), one stride parity class (py, px) per grid z: the output
//             pixels y = S i + py, x = S j + px are reached only by taps kh = py + S th, kw = px + S tw,
//             so K = (th, tw, cout) holds only real taps (conv2: 2x2x64 instead of 4x4x64)
//    NG_DW    dW[k][cout] = sum over (sample, pixel) of patch(k) dY, the reduction split over grid z
//             into per-split slabs (+ the column sums of dY: the bias gradient), folded in a fixed
//             order by k_slab_group + k_finalize (net_bwd.hip) -- deterministic, no atomics
//    NG_DW1   the same for conv1 (patches from the u8 ring; the 1/255 is the finalize's scale)
//  fc 3136 -> 512 and its backward: gemm.hip (split-K slabs with the bias + ReLU epilogue; the
//  weight gradient in-workgroup split-K); with NetLayout::fc_prec A3C_PREC_BF16 nature_fc.hip's
//  three kernels on single bf16 operands.  Head (k_nat_head): head_row<512> + the action draw and the
//  fused env act of net_head.h; the rollout step's head + screen kernels: net_fwd.hip; head
//  backward: k_head_bwd<512> (net_bwd.hip).
#include "nature.h"
#include "net_bwd.h"
#include "net_head.h"

// (the values are part of the kernels' symbol names, which profiles/ and tools/ record: 0 and 1
// were the forward modes, whose passes k_nat_conv23 / k_nat_conv123_b1 run)
enum { NG_DX = 2, NG_DW1, NG_DW };

// conv layer geometry (NHWC input H x W x C, TF weights [KH][KW][C][OC], VALID, stride S)
template <int LAYER> struct NG;
template <> struct NG<1> { static constexpr int H = IMG, W = IMG, C = HIST, KH = 8, KW = 8, S = 4, OH = NT1_O, OW = NT1_O, OC = NT1_N; };
template <> struct NG<2> { static constexpr int H = NT1_O, W = NT1_O, C = NT1_N, KH = 4, KW = 4, S = 2, OH = NT2_O, OW = NT2_O, OC = NT2_N; };
template <> struct NG<3> { static constexpr int H = NT2_O, W = NT2_O, C = NT2_N, KH = 3, KW = 3, S = 1, OH = NT3_O, OW = NT3_O, OC = NT3_N; };

// (bias and scale were the removed forward modes' and are read by nothing: they stay because the
// kernels' argument layout does -- without them the compiler merges the argument loads of the dX
// and conv1 dW tiles differently and allocates other registers, and these kernels are to stay the
// instructions that were measured)
struct NatGemm {
  StateAddr sa;        // NG_DW1: the u8 state planes of sample b (b = t E + e)
  const float* X;      // fp32 NHWC input activation [B][H][W][C] (NG_DW; NG_DX: its ReLU mask)
  const float* Wt;     // NG_DX: TF weights [KH][KW][C][OC]
  const float* bias;   // unused
  const float* dY;     // [B][OH][OW][OC]
  float* Y;            // NG_DX: dX [B][H][W][C]
  float* slab;         // NG_DW*: [nsplit][M][N]
  float* colsum;       // NG_DW*: [nsplit][N]
  int M, N, K;         // NG_DX: M per parity class; NG_DW*: M = KH KW C, N = OC, K = B OH OW (reduction)
  int kchunk;          // NG_DW*: reduction rows per split (a multiple of the K slice)
  float scale;         // unused
  int xcd;             // XCD-grouped tile order (nat_tile_of)
};

// The dispatcher deals workgroups round-robin over the 8 XCDs (linear id % 8), each with its own
// L2.  The workgroups that read the same operands -- the m-tiles of one reduction chunk (dW: the
// same dY rows and overlapping patches), the stride-parity classes of one m-tile (dX: the same dY
// rows) -- would land on 8 different XCDs and each fetch them from HBM; here a group of them takes
// consecutive ids of one XCD instead (grid x extent 1: id = y + Y z).
template <int MODE>
__device__ inline void nat_tile_of(int xcd, int& by, int& bz) {
  by = (int)blockIdx.y; bz = (int)blockIdx.z;
  if (!xcd || gridDim.x != 1) return;
  constexpr bool DWM = MODE == NG_DW || MODE == NG_DW1;
  const int G = DWM ? (int)gridDim.z : (int)gridDim.y;     // groups sharing data
  const int S = DWM ? (int)gridDim.y : (int)gridDim.z;     // workgroups per group
  const int L = by + (int)gridDim.y * bz;
  const int full = G / 8 * 8;
  int g, m;
  if (L < full * S) {
    const int blk = L / (8 * S), rem = L - blk * 8 * S;
    m = rem / 8; g = blk * 8 + rem % 8;
  } else {
    const int cl = G - full, rem = L - full * S;
    m = rem / cl; g = full + rem % cl;
  }
  if (DWM) { bz = g; by = m; } else { by = g; bz = m; }
}

// the frame-ring planes of sample b = t E + e without 64-bit divisions: slot0 = the ring slot of
// plane 0 of t = 0, reduced once per launch
struct RingRows {
  const uint8_t* base;
  int64_t env_stride, plane_bytes;
  int E, R, slot0;
  uint64_t emagic;     // ceil(2^40 / E): t = b E^-1 by a multiply (b E < 2^40)
  __device__ void init(const StateAddr& sa, int64_t tau0) {
    base = sa.base; env_stride = sa.env_stride; plane_bytes = sa.plane_bytes; E = sa.E; R = sa.R;
    emagic = ((1ull << 40) + (uint64_t)E - 1) / (uint64_t)E;
    int64_t s0 = (tau0 + sa.tau_offset - (sa.L - 1)) % sa.R;
    slot0 = (int)(s0 < 0 ? s0 + sa.R : s0);
  }
  __device__ int step_of(int b) const { return (int)(((uint64_t)b * emagic) >> 40); }
  __device__ const uint8_t* plane(int e, int t, int c) const {
    int s = slot0 + t + c;
    while (s >= R) s -= R;
    return base + e * env_stride + s * plane_bytes;
  }
};

// ---------------------------------------------------------------------------------------
// The conv backward passes on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 32 cycles per 32x32x16
// against 512 for a v_mfma_f32_32x32x2f32 chain of the same depth: the fp32 MFMA form of this tile
// lost on the dX and conv1 dW passes alone and in the whole bench, DESIGN §4d,
// profiles/round6/r6bf3_nature_pass_ab.txt).  Geometry at compile time (every index division by a
// constant).  Each fp32 operand is split at the LDS store into
// three round-to-nearest bf16 terms x = hi + mid + lo (v_cvt_pk_bf16_f32; exact to ~2^-24 relative)
// and the tile sums the six products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi (the dropped
// ones are below 2^-24 of the product): fp32-class results, as the NIPS conv2 (net_fwd.hip).
// conv1's dW (TA = 1): a u8 pixel is exact in one bf16 term, three products.
// LDS holds the terms k-contiguous ([row][k], 40 bf16 a row) for the MFMA's 8-deep lane fragments;
// operands that arrive along rows (the dW passes' A and B) are loaded as
// quad pairs at k and k + 1 and stored as packed (k, k + 1) dwords.
// ---------------------------------------------------------------------------------------
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

// NT terms (1 or 3) of the pair (x0, x1), each a packed bf16x2 dword
template <int NT>
__device__ inline void nat_split2(float x0, float x1, uint32_t (&o)[NT]) {
  const f32x2v v = {x0, x1};
  const bf16x2v h = __builtin_convertvector(v, bf16x2v);
  o[0] = __builtin_bit_cast(uint32_t, h);
  if constexpr (NT == 3) {
    const f32x2v r1 = v - __builtin_convertvector(h, f32x2v);
    const bf16x2v m = __builtin_convertvector(r1, bf16x2v);
    const f32x2v r2 = r1 - __builtin_convertvector(m, f32x2v);
    o[1] = __builtin_bit_cast(uint32_t, m);
    o[2] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r2, bf16x2v));
  }
}

// TB = 1 (with TA = 1): the bf16 compute mode (A3C_PREC_BF16) -- both operands rounded
// once at the LDS store, one product per K step, a third of the LDS
template <int MODE, int LAYER, int BN, int TA, int TB, int NBUF, int PF>
__global__ void __launch_bounds__(256) k_nat_gemm_bf(NatGemm a) {
  using G = NG<LAYER>;
  constexpr int BM = 4096 / BN, BK = 32, LD = 40;
  constexpr int WN = BN / 32;
  constexpr bool A_KC = MODE == NG_DX;                           // A quads along k (else pairs of row quads)
  constexpr bool B_NC = MODE != NG_DX;                           // B quads along n: pairs of row quads
  constexpr bool DW = MODE == NG_DW || MODE == NG_DW1;
  constexpr bool U8 = MODE == NG_DW1;
  static_assert(MODE == NG_DX || MODE == NG_DW || MODE == NG_DW1, "the backward passes");
  static_assert(TB == 3 || (TB == 1 && TA == 1), "one B term: the bf16 mode, one A term as well");
  static_assert(TA == 3 || (TA == 1 && (U8 || TB == 1)), "one A term: the exact u8 pixels, or the bf16 mode");
  constexpr int AQ = BM * BK / 4 / 256;                          // A quads per thread (2 or 4)
  constexpr int BQ0 = BN * BK / 4 / 256;
  constexpr int BQ = B_NC && BQ0 < 2 ? 2 : BQ0;                  // B quads per thread (pairs: >= 2)
  constexpr int BPAIRS = BN * BK / 8;                            // B_NC: quad pairs per slice
  constexpr int P = G::OH * G::OW;
  constexpr int TW = G::KW / G::S;
  constexpr int NI = G::H / G::S, NJ = G::W / G::S;
  static_assert(MODE != NG_DX || (G::H % G::S == 0 && G::KH % G::S == 0), "parity classes");
  static_assert(!U8 || G::C == 4, "u8 planes: the 4 history frames");
  static_assert((BM / 4) % 4 == 0 && (BN / 4) % 4 == 0, "pair mapping: 4 quads of a row per lane group");
  __shared__ __attribute__((aligned(16))) uint16_t As[NBUF][TA][BM][LD];   // NBUF 1: a third of the LDS,
  __shared__ __attribute__((aligned(16))) uint16_t Bs[NBUF][TB][BN][LD];   // two barriers per slice
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  int by, bz;
  nat_tile_of<MODE>(a.xcd, by, bz);
  const int m0 = by * BM, n0 = blockIdx.x * BN;
  const int kbeg = DW ? bz * a.kchunk : 0;
  const int kend = DW ? min(a.K, kbeg + a.kchunk) : a.K;
  const int py = MODE == NG_DX ? bz / G::S : 0, px = MODE == NG_DX ? bz % G::S : 0;
  RingRows ring;
  if constexpr (U8) ring.init(a.sa, a.sa.tau_ptr ? *a.sa.tau_ptr : 0);
  // pair p of row quads: 4 lanes along the row's quads (64 contiguous bytes), then 16 k pairs
  auto pair_q = [](int p, int nrowq) { (void)nrowq; return ((p >> 2) / (BK / 2)) * 4 + (p & 3); };
  auto pair_k = [](int p) { return ((p >> 2) % (BK / 2)) * 2; };

  int ar[AQ], ac[AQ];          // A_KC: tile row m, k offset; else: reduction row, m offset
  bool aval[AQ];
  int64_t abase[AQ];
  int ai[AQ], aj[AQ];
  int mk[AQ][3];
#pragma unroll
  for (int i = 0; i < AQ; ++i) {
    if constexpr (A_KC) {
      const int q = tid + 256 * i;
      ar[i] = q >> 3; ac[i] = (q & 7) * 4;
    } else if constexpr (U8) {
      // conv1 dW: quads i = (half h = i >> 1, row i & 1) of one 8-pixel patch row: a lane loads
      // kw 0..7 of (cin, kh) as one 8-byte load per row; lanes run along the k pairs
      static_assert(AQ == 4 && BM == 128, "u8 octets: 16 octets x 16 k pairs");
      ar[i] = 2 * (tid % (BK / 2)) + (i & 1); ac[i] = ((tid / (BK / 2)) * 2 + (i >> 1)) * 4;
    } else {
      const int pp = tid + 256 * (i >> 1);
      ar[i] = pair_k(pp) + (i & 1); ac[i] = pair_q(pp, BM / 4) * 4;
    }
    abase[i] = 0; ai[i] = aj[i] = 0;
    if constexpr (A_KC) {
      const int m = m0 + ar[i];
      aval[i] = m < a.M;
      const int mm = aval[i] ? m : 0;
      const int b = mm / (NI * NJ), r = mm - b * (NI * NJ);
      abase[i] = b; ai[i] = r / NJ; aj[i] = r - (r / NJ) * NJ;
    } else {
      const int m = m0 + ac[i];
      aval[i] = m < a.M;
      const int mm = aval[i] ? m : 0;
      if constexpr (U8) {
        mk[i][0] = (mm >> 3) & 7; mk[i][1] = mm & 7; mk[i][2] = mm >> 6;
      } else {
        mk[i][0] = mm / (G::KW * G::C);
        mk[i][1] = (mm / G::C) % G::KW;
        mk[i][2] = mm % G::C;
      }
    }
  }
  int br[BQ], bc[BQ];          // B_NC: k row, n offset; else: n row, k offset
  bool bok[BQ];
#pragma unroll
  for (int j = 0; j < BQ; ++j) {
    if constexpr (B_NC) {
      const int pp = tid + 256 * (j >> 1);
      bok[j] = pp < BPAIRS;
      br[j] = pair_k(pp) + (j & 1); bc[j] = pair_q(pp, BN / 4) * 4;
    } else {
      const int q = tid + 256 * j;
      bok[j] = true;
      br[j] = q >> 3; bc[j] = (q & 7) * 4;
    }
  }

  auto load_a = [&](int i, int k0) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (A_KC) {
      const int k = k0 + ac[i];
      if (!aval[i] || k >= kend) return v;
      const int th = k / (TW * G::OC), rem = k - th * (TW * G::OC), tw = rem / G::OC, oc0 = rem - tw * G::OC;
      const int oy = ai[i] - th, ox = aj[i] - tw;
      if (oy >= 0 && oy < G::OH && ox >= 0 && ox < G::OW)
        v = *(const f32x4*)(a.dY + ((abase[i] * G::OH + oy) * G::OW + ox) * G::OC + oc0);
    } else {
      const int r = k0 + ar[i];
      if (!aval[i] || r >= kend) return v;
      const int b = r / P, pos = r - b * P, oy = pos / G::OW, ox = pos - oy * G::OW;
      const int y = oy * G::S + mk[i][0], x = ox * G::S + mk[i][1];
      if constexpr (U8) {
        const int t = ring.step_of(b);
        const uint32_t d = *(const uint32_t*)(ring.plane(b - t * ring.E, t, mk[i][2]) + y * IMG + x);
        v[0] = (float)(d & 255u); v[1] = (float)((d >> 8) & 255u); v[2] = (float)((d >> 16) & 255u); v[3] = (float)(d >> 24);
      } else {
        v = *(const f32x4*)(a.X + (((int64_t)b * G::H + y) * G::W + x) * G::C + mk[i][2]);
      }
    }
    return v;
  };
  auto load_b = [&](int j, int k0) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!bok[j]) return v;
    if constexpr (B_NC) {                                          // (DW) dY rows
      const int k = k0 + br[j], n = n0 + bc[j];
      if (k >= kend || n >= a.N) return v;
      v = *(const f32x4*)(a.dY + (int64_t)k * G::OC + n);
    } else {
      const int n = n0 + br[j], k = k0 + bc[j];
      if (n >= a.N || k >= kend) return v;
      const int th = k / (TW * G::OC), rem = k - th * (TW * G::OC), tw = rem / G::OC, oc0 = rem - tw * G::OC;
      const int kh = py + G::S * th, kw = px + G::S * tw;
      v = *(const f32x4*)(a.Wt + (((int64_t)kh * G::KW + kw) * G::C + n) * G::OC + oc0);
    }
    return v;
  };

  // bias gradient: column sums of dY from the B registers (before the split), one fixed order
  const bool do_colsum = DW && a.colsum && by == 0;
  constexpr int CSN = BQ / 2 > 0 ? BQ / 2 : 1;
  float cs[CSN][4];
#pragma unroll
  for (int jj = 0; jj < CSN; ++jj)
#pragma unroll
    for (int c = 0; c < 4; ++c) cs[jj][c] = 0.f;

  auto store = [&](int buf, const f32x4 (&ra)[AQ], const f32x4 (&rbv)[BQ]) {
    if constexpr (A_KC) {
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        uint32_t lo[TA], hi[TA];
        nat_split2<TA>(ra[i][0], ra[i][1], lo);
        nat_split2<TA>(ra[i][2], ra[i][3], hi);
#pragma unroll
        for (int t = 0; t < TA; ++t) *(uint2*)&As[buf][t][ar[i]][ac[i]] = make_uint2(lo[t], hi[t]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < AQ; i += 2)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          uint32_t w[TA];
          nat_split2<TA>(ra[i][c], ra[i + 1][c], w);
#pragma unroll
          for (int t = 0; t < TA; ++t) *(uint32_t*)&As[buf][t][ac[i] + c][ar[i]] = w[t];
        }
    }
    if constexpr (B_NC) {
#pragma unroll
      for (int j = 0; j < BQ; j += 2) {
        if (!bok[j]) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          uint32_t w[TB];
          nat_split2<TB>(rbv[j][c], rbv[j + 1][c], w);
#pragma unroll
          for (int t = 0; t < TB; ++t) *(uint32_t*)&Bs[buf][t][bc[j] + c][br[j]] = w[t];
          if (DW && do_colsum) cs[j / 2][c] += rbv[j][c] + rbv[j + 1][c];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < BQ; ++j) {
        uint32_t lo[TB], hi[TB];
        nat_split2<TB>(rbv[j][0], rbv[j][1], lo);
        nat_split2<TB>(rbv[j][2], rbv[j][3], hi);
#pragma unroll
        for (int t = 0; t < TB; ++t) *(uint2*)&Bs[buf][t][br[j]][bc[j]] = make_uint2(lo[t], hi[t]);
      }
    }
  };

  f32x16 acc = {};
  const int r = lane & 31, h = lane >> 5;
  // conv1 dW: the 8 pixels kw 0..7 of quad i's (cin, kh) row -> quads i (kw 0..3) and i + 2 (kw 4..7)
  auto load_a8 = [&](int i, int k0, f32x4& lo, f32x4& hi) {
    const int r = k0 + ar[i];
    uint2 d = make_uint2(0u, 0u);
    if (aval[i] && r < kend) {
      const int b = r / P, pos = r - b * P, oy = pos / G::OW, ox = pos - oy * G::OW;
      const int y = oy * G::S + mk[i][0], x = ox * G::S;
      const int t = ring.step_of(b);
      const uint32_t* q = (const uint32_t*)(ring.plane(b - t * ring.E, t, mk[i][2]) + y * IMG + x);
      d.x = q[0];
      d.y = q[1];
    }
    lo = (f32x4){(float)(d.x & 255u), (float)((d.x >> 8) & 255u), (float)((d.x >> 16) & 255u), (float)(d.x >> 24)};
    hi = (f32x4){(float)(d.y & 255u), (float)((d.y >> 8) & 255u), (float)((d.y >> 16) & 255u), (float)(d.y >> 24)};
  };
  auto load_all = [&](int k0, f32x4 (&ra)[AQ], f32x4 (&rbv)[BQ]) {
    if constexpr (U8) {
      load_a8(0, k0, ra[0], ra[2]);
      load_a8(1, k0, ra[1], ra[3]);
    } else {
#pragma unroll
      for (int i = 0; i < AQ; ++i) ra[i] = load_a(i, k0);
    }
#pragma unroll
    for (int j = 0; j < BQ; ++j) rbv[j] = load_b(j, k0);
  };
  auto compute = [&](int buf) {
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 af[TA], bv[TB];
#pragma unroll
      for (int t = 0; t < TA; ++t) af[t] = *(const bf16x8*)&As[buf][t][wm * 32 + r][16 * s + 8 * h];
#pragma unroll
      for (int t = 0; t < TB; ++t) bv[t] = *(const bf16x8*)&Bs[buf][t][wn * 32 + r][16 * s + 8 * h];
      if constexpr (TB == 1) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[0], acc, 0, 0, 0);
      } else if constexpr (TA == 1) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[0], acc, 0, 0, 0);
      } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], bv[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bv[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bv[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bv[0], acc, 0, 0, 0);
      }
    }
  };
  if constexpr (PF == 2) {
    // two register sets: slice s + 2 loads while slice s computes (s + 1 waits in registers)
    f32x4 ra0[AQ], rb0[BQ], ra1[AQ], rb1[BQ];
    load_all(kbeg, ra0, rb0);
    store(0, ra0, rb0);
    if (kbeg + BK < kend) load_all(kbeg + BK, ra1, rb1);
    if (kbeg + 2 * BK < kend) load_all(kbeg + 2 * BK, ra0, rb0);
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += 2 * BK) {
      compute(0);
      if constexpr (NBUF == 1) __syncthreads();
      if (k0 + BK < kend) {
        store(NBUF - 1, ra1, rb1);
        if (k0 + 3 * BK < kend) load_all(k0 + 3 * BK, ra1, rb1);
      }
      __syncthreads();
      if (k0 + BK >= kend) break;
      compute(NBUF - 1);
      if constexpr (NBUF == 1) __syncthreads();
      if (k0 + 2 * BK < kend) {
        store(0, ra0, rb0);
        if (k0 + 4 * BK < kend) load_all(k0 + 4 * BK, ra0, rb0);
      }
      __syncthreads();
    }
  } else if constexpr (NBUF == 1) {
    f32x4 ra[AQ], rbv[BQ];
    load_all(kbeg, ra, rbv);
    store(0, ra, rbv);
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
      const bool more = k0 + BK < kend;
      if (more) load_all(k0 + BK, ra, rbv);
      compute(0);
      __syncthreads();
      if (more) {
        store(0, ra, rbv);
        __syncthreads();
      }
    }
  } else {
    f32x4 ra[AQ], rbv[BQ];
    load_all(kbeg, ra, rbv);
    store(0, ra, rbv);
    __syncthreads();
    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
      const bool more = k0 + BK < kend;
      if (more) load_all(k0 + BK, ra, rbv);
      compute(buf);
      if (more) store(buf ^ 1, ra, rbv);
      __syncthreads();
      buf ^= 1;
    }
  }

  const int col = n0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
    if (row >= a.M || col >= a.N) continue;
    float v = acc[q];
    if constexpr (MODE == NG_DX) {
      const int b = row / (NI * NJ), rr = row - b * (NI * NJ), i = rr / NJ, j = rr - (rr / NJ) * NJ;
      const int64_t o = (((int64_t)b * G::H + py + G::S * i) * G::W + px + G::S * j) * G::C + col;
      a.Y[o] = a.X[o] > 0.f ? v : 0.f;
    } else {
      const int trow = MODE == NG_DW1 ? ((((row >> 3) & 7) * 8 + (row & 7)) * 4 + (row >> 6)) : row;
      a.slab[((int64_t)bz * a.M + trow) * a.N + col] = v;
    }
  }
  if constexpr (DW) {
    if (do_colsum) {      // (block-uniform) per-pair partials through LDS, summed over the k pairs in order
      float* red = (float*)&As[0][0][0][0];
#pragma unroll
      for (int j = 0; j < BQ; j += 2) {
        const int pp = tid + 256 * (j >> 1);
        if (pp < BPAIRS) *(f32x4*)&red[pp * 4] = (f32x4){cs[j / 2][0], cs[j / 2][1], cs[j / 2][2], cs[j / 2][3]};
      }
      __syncthreads();
      if (tid < BN && n0 + tid < a.N) {
        const int nq = tid >> 2, c = tid & 3;
        float sum = 0.f;
        for (int kp = 0; kp < BK / 2; ++kp) sum += red[((((nq >> 2) * (BK / 2) + kp) << 2) | (nq & 3)) * 4 + c];
        a.colsum[(int64_t)bz * a.N + n0 + tid] = sum;
      }
    }
  }
}

template <int MODE, int LAYER, int BN, int TA, int TB, int NBUF, int PF>
static int nat_go_bf(NatGemm a, unsigned gz, hipStream_t s) {
  constexpr int BM = 4096 / BN;
  if (a.M <= 0 || a.N <= 0) return 0;
  a.xcd = 1;   // (the hardware tile order lost, 1.27M against 1.33M: DESIGN §4d, profiles/round6/r6pf4_nature_knob_bench_ab.txt)
  const dim3 grid((unsigned)((a.N + BN - 1) / BN), (unsigned)((a.M + BM - 1) / BM), gz);
  hipLaunchKernelGGL((k_nat_gemm_bf<MODE, LAYER, BN, TA, TB, NBUF, PF>), grid, dim3(256), 0, s, a);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// The prepared block: the conv weights as round-to-nearest bf16 terms (w = hi + mid + lo to ~2^-24
// relative, as the NIPS conv1, net_fwd.hip), k-contiguous per output channel, for the per-state
// forward kernels below.
// ---------------------------------------------------------------------------------------
__device__ inline uint32_t nat_bf16_rn(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

// NT = 3: the three terms; NT = 1 (the bf16 mode): rn(w) alone, in the first term's place
template <int NT>
__device__ inline void nat_terms3(float w, uint16_t* dst, int64_t tstride) {
#pragma clang fp contract(off)
  const uint32_t h = nat_bf16_rn(w);
  if constexpr (NT == 1) {
    dst[0] = (uint16_t)h;
    return;
  }
  const float r1 = w - __uint_as_float(h << 16);
  const uint32_t m = nat_bf16_rn(r1);
  const float r2 = r1 - __uint_as_float(m << 16);
  const uint32_t l = nat_bf16_rn(r2);
  dst[0] = (uint16_t)h;
  dst[tstride] = (uint16_t)m;
  dst[2 * tstride] = (uint16_t)l;
}

// the prepared block: conv1 [3][32][256] with k' = (cin, kh, kw); conv2 [3][64][512] and conv3
// [3][64][576] with k in TF order (kh, kw, cin) -- one thread per (cout, k)
template <int NT>
__global__ void __launch_bounds__(256) k_nat_w_terms(const float* __restrict__ W1, const float* __restrict__ W2,
                                                     const float* __restrict__ W3, uint16_t* __restrict__ wt) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < NT1_N * NT_K1) {
    const int n = i / NT_K1, k = i - n * NT_K1;
    const int c = k >> 6, kh = (k >> 3) & 7, kw = k & 7;
    nat_terms3<NT>(W1[((kh * 8 + kw) * HIST + c) * NT1_N + n], wt + n * NT_K1 + k, NT1_N * NT_K1);
    return;
  }
  i -= NT1_N * NT_K1;
  if (i < NT2_N * NT_K2) {
    const int n = i / NT_K2, k = i - n * NT_K2;
    nat_terms3<NT>(W2[k * NT2_N + n], wt + A3C_NAT_W2T_OFF / 2 + n * NT_K2 + k, NT2_N * NT_K2);
    return;
  }
  i -= NT2_N * NT_K2;
  if (i < NT3_N * NT_K3) {
    const int n = i / NT_K3, k = i - n * NT_K3;
    nat_terms3<NT>(W3[k * NT3_N + n], wt + A3C_NAT_W3T_OFF / 2 + n * NT_K3 + k, NT3_N * NT_K3);
  }
}

__device__ inline uint2 nat_u8x4_bf16(uint32_t d) {   // 4 pixels -> 4 bf16 (exact: the upper halves of their f32)
  const float f0 = (float)(d & 255u), f1 = (float)((d >> 8) & 255u);
  const float f2 = (float)((d >> 16) & 255u), f3 = (float)(d >> 24);
  return make_uint2(__builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u),
                    __builtin_amdgcn_perm(__float_as_uint(f3), __float_as_uint(f2), 0x07060302u));
}

// ---------------------------------------------------------------------------------------
// conv1 + conv2 + conv3 forward fused, one workgroup per sample (the rollout's B = E states).
// conv1: the sample's 4 u8 planes staged as bf16 rows, M = 400 pixels, N = 32, K = 256 in (cin, kh,
// kw) order on v_mfma_f32_16x16x32_bf16 (the u8 pixel exact in one term: three products); its
// output (x/255 + bias, ReLU) goes out for the backward and, as three bf16 terms, into LDS.  conv2
// (M = 81 pixels, N = 64, K = 16 taps x 32) and then conv3 (M = 49, N = 64, K = 9 taps x 64) run
// with the six products of the term split (as k_nat_gemm_bf); l2 goes out (the backward's operand)
// and, as terms, into the LDS the l1 terms held, for conv3.  Wave w owns output channels
// 16w..16w+15 of conv2 / conv3, its weight fragments (the prepared terms, [term][cout][k]) streamed
// from L2 with a 3-tap register ring.  The per-layer tile passes it replaced were K-chain-bound at
// this batch (324 / 392 tiles and a fold; conv1 its own launch: 1.47M against 1.51M with it inside;
// DESIGN §4d, profiles/round6/r6fu_nature_fusion_ab.txt, r6sp1_nature_split_ab.txt).
// ---------------------------------------------------------------------------------------
// l1 terms: [term][y 20][x parity 2][x / 2 10][32 bf16]: a 16-lane fragment read walks consecutive
// output pixels, which sit at x = 2 ox + kw -- parity-split rows put them one row apart.
// l2 terms: [term][81][72 bf16] over the same LDS after conv2.
#ifndef C23_R1          // (A/B builds: -DC23_R1=40, rows padded for the fragment reads' banks: 96 KB)
#define C23_R1 32          // unpadded: 77 KB, same time alone, room beside the backward (r6r32: 1.64M vs 1.59M)
#endif
#define C23_T1 (NT1_O * 2 * (NT1_O / 2) * C23_R1)   // bf16 per l1 term: 16000
#define C23_R2 72
#define C23_T2 (NT2_P * C23_R2)                     // 5832
static_assert(3 * C23_T2 <= 3 * C23_T1, "l2 terms overlay the l1 terms");

__device__ inline f32x4 c23_mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  return acc;
}

#define C123_PR 88                                   // bf16 per staged plane row (84 + 4)
static_assert(HIST * IMG * C123_PR <= 3 * C23_T1, "planes fit the term LDS");
#ifndef C23_PD     // weight-fragment prefetch distance in K steps (the ring holds C23_PD + 1 steps)
#define C23_PD 2
#endif
#ifndef C23_BATCH  // 1: the plane staging issues all its loads before the first conversion
#define C23_BATCH 1
#endif
__global__ void __launch_bounds__(256) k_nat_conv23(const uint16_t* __restrict__ w2t, const float* __restrict__ b2,
                                                    const uint16_t* __restrict__ w3t, const float* __restrict__ b3,
                                                    float* __restrict__ l2, float* __restrict__ l3, StateAddr sa,
                                                    const uint16_t* __restrict__ w1t, const float* __restrict__ b1,
                                                    float* __restrict__ l1, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t sm[3 * C23_T1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.x;
  // the engine's live launch span (a3c_engine_span_stats 1, bench.py's roofline)
  unsigned long long* srec = span_rec(sa, sa.tau_ptr ? *sa.tau_ptr : 0);
  span_begin(srec);
  {
    // ---- the 4 history planes of state b as bf16 [cin][84][88] ----
    RingRows ring;
    ring.init(sa, sa.tau_ptr ? *sa.tau_ptr : 0);
    const int st = ring.step_of((int)b), e = (int)b - st * ring.E;
#if C23_BATCH
    // every dword of the 4 planes in flight at once (28 per thread), then converted and stored
    constexpr int NQ = HIST * PLANE / 4, PQ = PLANE / 4, PER = (NQ + 255) / 256;
    const uint32_t* pl4[HIST];
#pragma unroll
    for (int c = 0; c < HIST; ++c) pl4[c] = (const uint32_t*)ring.plane(e, st, c);
    uint32_t pv[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = tid + 256 * i, c = q / PQ;
      pv[i] = q < NQ ? pl4[c < HIST ? c : 0][q - c * PQ] : 0u;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = tid + 256 * i;
      if (q < NQ) {
        const int c = q / PQ, r = q - c * PQ, y = r / (IMG / 4), x4 = (r - y * (IMG / 4)) * 4;
        *(uint2*)&sm[(c * IMG + y) * C123_PR + x4] = nat_u8x4_bf16(pv[i]);
      }
    }
#else
#pragma unroll
    for (int c = 0; c < HIST; ++c) {
      const uint32_t* src = (const uint32_t*)ring.plane(e, st, c);
      for (int q = tid; q < PLANE / 4; q += 256) {
        const int y = q / (IMG / 4), x4 = (q - y * (IMG / 4)) * 4;
        *(uint2*)&sm[(c * IMG + y) * C123_PR + x4] = nat_u8x4_bf16(src[q]);
      }
    }
#endif
    __syncthreads();
    // ---- conv1: 25 m-tiles x 2 n-tiles of 16; wave w: n-tile w & 1, m-tiles (w >> 1) + 2 i ----
    const int n1 = 16 * (w & 1) + i16;
    const int mh = w >> 1;
    int base1[13];
    f32x4 acc1[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) {
      const int m = min(16 * (mh + 2 * i) + i16, NT1_P - 1);
      const int oy = m / NT1_O, ox = m - oy * NT1_O;
      base1[i] = 4 * oy * C123_PR + 4 * ox;
      acc1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t* wb1 = w1t + n1 * NT_K1 + 8 * g;
    bf16x8 q1[C23_PD + 1][3];
    auto ldb1 = [&](int ks, bf16x8 (&dst)[3]) {
#pragma unroll
      for (int t = 0; t < 3; ++t) dst[t] = *(const bf16x8*)(wb1 + t * NT1_N * NT_K1 + ks * 32);
    };
#pragma unroll
    for (int q = 0; q < C23_PD; ++q) ldb1(q, q1[q]);
#pragma unroll
    for (int ks = 0; ks < NT_K1 / 32; ++ks) {
      if (ks + C23_PD < NT_K1 / 32) ldb1(ks + C23_PD, q1[(ks + C23_PD) % (C23_PD + 1)]);
      const int cin = ks >> 1, kh = 4 * (ks & 1) + g;
      const uint16_t* rp = sm + (cin * IMG + kh) * C123_PR;
#pragma unroll
      for (int i = 0; i < 13; ++i) {
        if (mh + 2 * i >= NT1_P / 16) continue;          // (wave-uniform) the 25 tiles
        const uint2 u0 = *(const uint2*)(rp + base1[i]), u1 = *(const uint2*)(rp + base1[i] + 4);
        const bf16x8 a = __builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y));
        const bf16x8* bb = q1[ks % (C23_PD + 1)];
        acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb[2], acc1[i], 0, 0, 0);
        acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb[1], acc1[i], 0, 0, 0);
        acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb[0], acc1[i], 0, 0, 0);
      }
    }
    __syncthreads();   // the planes are no longer read: their LDS takes the l1 terms
    const float bn1 = b1[n1];
#pragma unroll
    for (int i = 0; i < 13; ++i) {
      if (mh + 2 * i >= NT1_P / 16) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * (mh + 2 * i) + 4 * g + r;
        const float v = fmaxf(acc1[i][r] * scale + bn1, 0.f);
        l1[(b * NT1_P + m) * NT1_N + n1] = v;
        const int y = m / NT1_O, x = m - y * NT1_O;
        const int slot = (y * 2 + (x & 1)) * (NT1_O / 2) + (x >> 1);
        const float hf = __uint_as_float(nat_bf16_rn(v) << 16);
        const float r1 = v - hf;
        const float mf = __uint_as_float(nat_bf16_rn(r1) << 16);
        sm[0 * C23_T1 + slot * C23_R1 + n1] = (uint16_t)(__float_as_uint(hf) >> 16);
        sm[1 * C23_T1 + slot * C23_R1 + n1] = (uint16_t)(__float_as_uint(mf) >> 16);
        sm[2 * C23_T1 + slot * C23_R1 + n1] = (uint16_t)nat_bf16_rn(r1 - mf);
      }
    }
  }
  __syncthreads();
  // ---- conv2: 6 m-tiles of 16 pixels (81 valid) x this wave's 16 channels, 16 taps ----
  const int n = 16 * w + i16;
  int base2[6];
#pragma unroll
  for (int mt = 0; mt < 6; ++mt) {
    const int m = min(16 * mt + i16, NT2_P - 1);
    const int oy = m / NT2_O, ox = m - oy * NT2_O;
    base2[mt] = (oy * 2 * 2) * (NT1_O / 2) + ox;           // slot of (y = 2 oy, parity 0, x/2 = ox)
  }
  f32x4 acc2[6];
#pragma unroll
  for (int mt = 0; mt < 6; ++mt) acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const uint16_t* wb2 = w2t + (int64_t)n * NT_K2 + 8 * g;
  bf16x8 bq[C23_PD + 1][3];
  auto ldb2 = [&](int tap, bf16x8 (&dst)[3]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) dst[t] = *(const bf16x8*)(wb2 + (int64_t)t * NT2_N * NT_K2 + tap * 32);
  };
#pragma unroll
  for (int q = 0; q < C23_PD; ++q) ldb2(q, bq[q]);
#pragma unroll
  for (int tap = 0; tap < 16; ++tap) {
    if (tap + C23_PD < 16) ldb2(tap + C23_PD, bq[(tap + C23_PD) % (C23_PD + 1)]);
    const int kh = tap >> 2, kw = tap & 3;
    const int toff = (kh * 2 + (kw & 1)) * (NT1_O / 2) + (kw >> 1);
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
      bf16x8 a[3];
      const uint16_t* ap = sm + (base2[mt] + toff) * C23_R1 + 8 * g;
#pragma unroll
      for (int t = 0; t < 3; ++t) a[t] = *(const bf16x8*)(ap + t * C23_T1);
      acc2[mt] = c23_mfma6(a, bq[tap % (C23_PD + 1)], acc2[mt]);
    }
  }
  __syncthreads();   // every wave is done reading the l1 terms
  // ---- conv2 epilogue: bias + ReLU, l2 out, l2 terms into LDS ----
  {
    const float bn = b2[n];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * g + r;
        if (m < NT2_P) {
          const float v = fmaxf(acc2[mt][r] + bn, 0.f);
          l2[(b * NT2_P + m) * NT2_N + n] = v;
          const float hf = __uint_as_float(nat_bf16_rn(v) << 16);
          const float r1 = v - hf;
          const float mf = __uint_as_float(nat_bf16_rn(r1) << 16);
          const float r2 = r1 - mf;
          sm[0 * C23_T2 + m * C23_R2 + n] = (uint16_t)(__float_as_uint(hf) >> 16);
          sm[1 * C23_T2 + m * C23_R2 + n] = (uint16_t)(__float_as_uint(mf) >> 16);
          sm[2 * C23_T2 + m * C23_R2 + n] = (uint16_t)nat_bf16_rn(r2);
        }
      }
  }
  // weight ring of conv3 starts under the barrier
  const uint16_t* wb3 = w3t + (int64_t)n * NT_K3 + 8 * g;
  auto ldb3 = [&](int st, bf16x8 (&dst)[3]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) dst[t] = *(const bf16x8*)(wb3 + (int64_t)t * NT3_N * NT_K3 + st * 32);
  };
#pragma unroll
  for (int q = 0; q < C23_PD; ++q) ldb3(q, bq[q]);
  __syncthreads();
  // ---- conv3: 4 m-tiles of 16 pixels (49 valid), 18 K steps (9 taps x 2 channel halves) ----
  int base3[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = min(16 * mt + i16, NT3_P - 1);
    const int oy = m / NT3_O, ox = m - oy * NT3_O;
    base3[mt] = oy * NT2_O + ox;
  }
  f32x4 acc3[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc3[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 18; ++st) {
    if (st + C23_PD < 18) ldb3(st + C23_PD, bq[(st + C23_PD) % (C23_PD + 1)]);
    const int tap = st >> 1, kh = tap / 3, kw = tap - kh * 3;
    const int off = (kh * NT2_O + kw) * C23_R2 + 32 * (st & 1) + 8 * g;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      bf16x8 a[3];
      const uint16_t* ap = sm + base3[mt] * C23_R2 + off;
#pragma unroll
      for (int t = 0; t < 3; ++t) a[t] = *(const bf16x8*)(ap + t * C23_T2);
      acc3[mt] = c23_mfma6(a, bq[st % (C23_PD + 1)], acc3[mt]);
    }
  }
  const float b3n = b3[n];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * mt + 4 * g + r;
      if (m < NT3_P) l3[(b * NT3_P + m) * NT3_N + n] = fmaxf(acc3[mt][r] + b3n, 0.f);
    }
  span_end(srec);
}

// ---------------------------------------------------------------------------------------
// The bf16 compute mode's forward (A3C_PREC_BF16): conv1 -> conv2 -> conv3 of one state
// per workgroup with one bf16 term per operand, rn(x) . rn(W), one v_mfma_f32_16x16x32_bf16 per K
// step, fp32 accumulators, bias + ReLU in fp32; l1 / l2 / l3 go out as fp32 (the backward's
// operands), rn(l1) and rn(l2) stay in LDS as the next layer's operand.
// LDS, 32000 B (k_nat_conv23: 76800), three tenants over one region:
//   planes  [cin 4][y 84][88 B] u8, 29568 B: staged as they are in the frame ring (a quarter of
//           the bf16 rows); conv1's A fragment is a lane's 8 pixels kw 0..7 of one (cin, kh) patch
//           row = two dword reads, converted in registers (exact: a pixel is the upper half of its
//           f32).  A wave owns both 16-channel n-tiles of its m-tiles (w + 4 i of the 25), so each
//           converted fragment feeds two MFMAs.
//   l1      [y 20][x parity 2][x / 2 10][40 bf16], 32000 B, over the planes once conv1 has read
//           them: the parity-split rows of k_nat_conv23 (conv2's 16 consecutive output pixels sit
//           one row apart), rows padded 32 -> 40 so that the 16 lanes of a fragment read hit 16
//           different 16-byte bank groups (80 B apart) -- the padding the three-term kernel had no
//           room for
//   l2      [81][72 bf16], 11664 B, over l1 once conv2 has read it
// Wave w owns output channels 16 w .. 16 w + 15 of conv2 and conv3; every layer's weight fragments
// (k_nat_w_terms<1>: [cout][k], the first term's place of the prepared block) stream from L2
// through the C23_PD + 1 deep register ring.
// ---------------------------------------------------------------------------------------
#define B1_PR 88                                    // bytes per staged u8 plane row (84 + 4)
#define B1_R1 40                                    // bf16 per l1 pixel (32 + 8)
#define B1_R2 72                                    // bf16 per l2 pixel (64 + 8)
#define B1_PLANES (HIST * IMG * B1_PR)              // 29568 B
#define B1_L1 (NT1_P * B1_R1 * 2)                   // 32000 B
#define B1_L2 (NT2_P * B1_R2 * 2)                   // 11664 B
#define B1_LDS (B1_L1 > B1_PLANES ? B1_L1 : B1_PLANES)
static_assert(B1_L2 <= B1_LDS && B1_LDS % 16 == 0, "l2 overlays l1");
static_assert(NT1_P % 16 == 0 && (NT1_P / 16 + 3) / 4 == 7, "conv1: 25 m-tiles dealt over 4 waves, 7 slots");

__global__ void __launch_bounds__(256) k_nat_conv123_b1(StateAddr sa, const uint16_t* __restrict__ w1r,
                                                        const float* __restrict__ b1, const uint16_t* __restrict__ w2r,
                                                        const float* __restrict__ b2, const uint16_t* __restrict__ w3r,
                                                        const float* __restrict__ b3, float* __restrict__ l1,
                                                        float* __restrict__ l2, float* __restrict__ l3, float scale) {
  __shared__ __attribute__((aligned(16))) uint8_t smb[B1_LDS];
  uint16_t* sm = (uint16_t*)smb;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.x;
  unsigned long long* srec = span_rec(sa, sa.tau_ptr ? *sa.tau_ptr : 0);   // (as k_nat_conv23)
  span_begin(srec);
  {
    // ---- the 4 history planes of state b, u8 [cin][84][88]: every dword in flight, then stored ----
    RingRows ring;
    ring.init(sa, sa.tau_ptr ? *sa.tau_ptr : 0);
    const int st = ring.step_of((int)b), e = (int)b - st * ring.E;
    constexpr int NQ = HIST * PLANE / 4, PQ = PLANE / 4, PER = (NQ + 255) / 256;
    const uint32_t* pl4[HIST];
#pragma unroll
    for (int c = 0; c < HIST; ++c) pl4[c] = (const uint32_t*)ring.plane(e, st, c);
    uint32_t pv[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = tid + 256 * i, c = q / PQ;
      pv[i] = q < NQ ? pl4[c < HIST ? c : 0][q - c * PQ] : 0u;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = tid + 256 * i;
      if (q < NQ) {
        const int c = q / PQ, r = q - c * PQ, y = r / (IMG / 4), x4 = (r - y * (IMG / 4)) * 4;
        *(uint32_t*)&smb[(c * IMG + y) * B1_PR + x4] = pv[i];
      }
    }
  }
  __syncthreads();
  {
    // ---- conv1: wave w takes m-tiles w + 4 i (25 of 16 pixels), both n-tiles of 16 channels ----
    constexpr int MT = 7, NTILES = NT1_P / 16;
    int base1[MT];
    f32x4 acc1[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = min(16 * (w + 4 * i) + i16, NT1_P - 1);
      const int oy = m / NT1_O, ox = m - oy * NT1_O;
      base1[i] = 4 * oy * B1_PR + 4 * ox;
      acc1[i][0] = acc1[i][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t* wb1 = w1r + i16 * NT_K1 + 8 * g;
    bf16x8 q1[C23_PD + 1][2];
    auto ldb1 = [&](int ks, bf16x8 (&dst)[2]) {
#pragma unroll
      for (int j = 0; j < 2; ++j) dst[j] = *(const bf16x8*)(wb1 + j * 16 * NT_K1 + ks * 32);
    };
#pragma unroll
    for (int q = 0; q < C23_PD; ++q) ldb1(q, q1[q]);
#pragma unroll
    for (int ks = 0; ks < NT_K1 / 32; ++ks) {
      if (ks + C23_PD < NT_K1 / 32) ldb1(ks + C23_PD, q1[(ks + C23_PD) % (C23_PD + 1)]);
      const int cin = ks >> 1, kh = 4 * (ks & 1) + g;        // k' = (cin, kh, kw): a lane's 8 k are kw 0..7
      const uint8_t* rp = smb + (cin * IMG + kh) * B1_PR;
      const bf16x8* bb = q1[ks % (C23_PD + 1)];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (w + 4 * i >= NTILES) continue;                    // (wave-uniform) the 25 tiles
        const uint2 lo = nat_u8x4_bf16(*(const uint32_t*)(rp + base1[i]));
        const uint2 hi = nat_u8x4_bf16(*(const uint32_t*)(rp + base1[i] + 4));
        const bf16x8 a = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        acc1[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb[0], acc1[i][0], 0, 0, 0);
        acc1[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb[1], acc1[i][1], 0, 0, 0);
      }
    }
    __syncthreads();   // the planes are no longer read: their LDS takes rn(l1)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n1 = 16 * j + i16;
      const float bn1 = b1[n1];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (w + 4 * i >= NTILES) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = 16 * (w + 4 * i) + 4 * g + r;
          const float v = fmaxf(acc1[i][j][r] * scale + bn1, 0.f);
          l1[(b * NT1_P + m) * NT1_N + n1] = v;
          const int y = m / NT1_O, x = m - y * NT1_O;
          const int slot = (y * 2 + (x & 1)) * (NT1_O / 2) + (x >> 1);
          sm[slot * B1_R1 + n1] = (uint16_t)nat_bf16_rn(v);
        }
      }
    }
  }
  __syncthreads();
  // ---- conv2: 6 m-tiles of 16 pixels (81 valid) x this wave's 16 channels, 16 taps of 32 cin ----
  const int n = 16 * w + i16;
  bf16x8 bq[C23_PD + 1];
  f32x4 acc2[6];
  {
    int base2[6];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
      const int m = min(16 * mt + i16, NT2_P - 1);
      const int oy = m / NT2_O, ox = m - oy * NT2_O;
      base2[mt] = (oy * 2 * 2) * (NT1_O / 2) + ox;           // slot of (y = 2 oy, parity 0, x/2 = ox)
      acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t* wb2 = w2r + (int64_t)n * NT_K2 + 8 * g;
#pragma unroll
    for (int q = 0; q < C23_PD; ++q) bq[q] = *(const bf16x8*)(wb2 + q * 32);
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      if (tap + C23_PD < 16) bq[(tap + C23_PD) % (C23_PD + 1)] = *(const bf16x8*)(wb2 + (tap + C23_PD) * 32);
      const int kh = tap >> 2, kw = tap & 3;
      const int toff = (kh * 2 + (kw & 1)) * (NT1_O / 2) + (kw >> 1);
#pragma unroll
      for (int mt = 0; mt < 6; ++mt) {
        const bf16x8 a = *(const bf16x8*)(sm + (base2[mt] + toff) * B1_R1 + 8 * g);
        acc2[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[tap % (C23_PD + 1)], acc2[mt], 0, 0, 0);
      }
    }
  }
  __syncthreads();   // every wave is done reading rn(l1)
  {
    const float bn = b2[n];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * g + r;
        if (m < NT2_P) {
          const float v = fmaxf(acc2[mt][r] + bn, 0.f);
          l2[(b * NT2_P + m) * NT2_N + n] = v;
          sm[m * B1_R2 + n] = (uint16_t)nat_bf16_rn(v);
        }
      }
  }
  // weight ring of conv3 starts under the barrier
  const uint16_t* wb3 = w3r + (int64_t)n * NT_K3 + 8 * g;
#pragma unroll
  for (int q = 0; q < C23_PD; ++q) bq[q] = *(const bf16x8*)(wb3 + q * 32);
  __syncthreads();
  // ---- conv3: 4 m-tiles of 16 pixels (49 valid), 18 K steps (9 taps x 2 channel halves) ----
  int base3[4];
  f32x4 acc3[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = min(16 * mt + i16, NT3_P - 1);
    const int oy = m / NT3_O, ox = m - oy * NT3_O;
    base3[mt] = oy * NT2_O + ox;
    acc3[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int st = 0; st < 18; ++st) {
    if (st + C23_PD < 18) bq[(st + C23_PD) % (C23_PD + 1)] = *(const bf16x8*)(wb3 + (st + C23_PD) * 32);
    const int tap = st >> 1, kh = tap / 3, kw = tap - kh * 3;
    const int off = (kh * NT2_O + kw) * B1_R2 + 32 * (st & 1) + 8 * g;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const bf16x8 a = *(const bf16x8*)(sm + base3[mt] * B1_R2 + off);
      acc3[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[st % (C23_PD + 1)], acc3[mt], 0, 0, 0);
    }
  }
  const float b3n = b3[n];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * mt + 4 * g + r;
      if (m < NT3_P) l3[(b * NT3_P + m) * NT3_N + n] = fmaxf(acc3[mt][r] + b3n, 0.f);
    }
  span_end(srec);
}

// the policy / value head of B states (one wave each) on the 512-wide fc output, + the action
// draw and fused env act when sel.mode >= 0 (agent.py:59-62, network.py:72)
// (GAME: the device env's game of the fused act, A3C_GAME_*)
template <int GAME = A3C_GAME_SYNTH>
__global__ void __launch_bounds__(256) k_nat_head(const float* __restrict__ l4, int64_t B, const float* __restrict__ Wp,
                                                  const float* __restrict__ bp, const float* __restrict__ Wv,
                                                  const float* __restrict__ bv, int A, int zs, float* __restrict__ z,
                                                  HeadSelect sel) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float myz = head_row<NoMid, NT_FC>(l4, b, Wp, bp, Wv, bv, A, lane);
  if (lane < zs) z[b * zs + lane] = myz;
  if (sel.mode >= 0) (void)head_act<GAME>(myz, lane, A, sel, b);
  // the overlap rollout's bootstrap head (its last kernel) advances tau (no tau read here)
  if (sel.adv_ptr && blockIdx.x == 0 && threadIdx.x == 0) *sel.adv_ptr += sel.adv_n;
}

static int nat_head_catch_launch(const NetLayout& L, const float* P, const float* l4, int64_t B, float* z,
                                 const HeadSelect& sel, hipStream_t s);
// ---------------------------------------------------------------------------------------
// passes (one launch each, timed individually by a3c_engine_time_kernel)
// ---------------------------------------------------------------------------------------
#define NAT_GROUPS 8
struct NatPlan {
  int head_split, ns1, ns2, ns3, kc1, kc2, kc3;
  int64_t dz, dl4, dl3, dl2, dl1, terms, hgrad, hcol, hslab, fccol, s1, s2, s3, c1, c2, c3, g1, g2, g3, wprep, total;
};
// workgroups per dW pass (the reduction's slab count): conv1 / conv2 / conv3 768 / 2048 / 768,
// by whole-bench sweeps (r6dwg2-5, B = 1280): 1.717M against 1.653M for 1536 on all three (the
// choice by times alone, r6dwg: 62 / 89 / 97 -> 51 / 74 / 81 us against 512); conv1's count is
// the sensitive one (832: 1.65M, 1536: 1.65M, 640: 1.68M).  DESIGN §4d,
// profiles/round6/r6dwg_nature_dw_wgs_sweep_ab.txt
#define NAT_DW_WGS1 768
#define NAT_DW_WGS2 2048
#define NAT_DW_WGS3 768
// the reduction split of a weight-gradient pass: ~target workgroups over its m tiles
static void dw_split(int64_t R, int mtiles, int target, int& ns, int& kc) {
  int want = target / mtiles;
  if (want < 1) want = 1;
  int64_t per = (R + want - 1) / want;
  per = (per + 31) / 32 * 32;               // whole K slices
  if (per < 32) per = 32;
  kc = (int)per;
  ns = (int)((R + per - 1) / per);
}
static NatPlan nat_plan(const NetLayout& L, int64_t B) {
  NatPlan p = {};
  int64_t o = 0;
  auto take = [&](int64_t floats) { int64_t r = o; o += (floats + 63) & ~(int64_t)63; return r; };
  p.head_split = a3c_gemm_effective_split((int)B, a3c_gemm_plan_split(NT_FC, L.zs, (int)B, 128));
  dw_split(B * NT1_P, 2, NAT_DW_WGS1, p.ns1, p.kc1);     // M = 256 in 128-row tiles
  dw_split(B * NT2_P, 8, NAT_DW_WGS2, p.ns2, p.kc2);     // M = 512 in 64-row tiles
  dw_split(B * NT3_P, 9, NAT_DW_WGS3, p.ns3, p.kc3);     // M = 576
  p.dz = take(B * L.zs);
  p.dl4 = take(B * NT_FC);
  p.dl3 = take(B * NT_FLAT);
  p.dl2 = take(B * NT_A2);
  p.dl1 = take(B * NT_A1);
  p.terms = take(B * 4);
  p.hgrad = take((int64_t)NT_FC * L.zs);
  p.hcol = take((int64_t)p.head_split * L.zs);
  p.hslab = take(p.head_split > 1 ? (int64_t)p.head_split * NT_FC * L.zs : 0);
  p.fccol = take(NT_FC);
  p.s1 = take((int64_t)p.ns1 * NT_K1 * NT1_N);
  p.s2 = take((int64_t)p.ns2 * NT_K2 * NT2_N);
  p.s3 = take((int64_t)p.ns3 * NT_K3 * NT3_N);
  p.c1 = take((int64_t)p.ns1 * NT1_N);
  p.c2 = take((int64_t)p.ns2 * NT2_N);
  p.c3 = take((int64_t)p.ns3 * NT3_N);
  p.g1 = take((int64_t)NAT_GROUPS * NT_K1 * NT1_N);
  p.g2 = take((int64_t)NAT_GROUPS * NT_K2 * NT2_N);
  p.g3 = take((int64_t)NAT_GROUPS * NT_K3 * NT3_N);
  p.wprep = take(A3C_NAT_PREP_BYTES / 4);   // the per-op path's weight terms (the engine's are in the slot)
  p.total = o;
  return p;
}

// the fc forward's split-K: the plan's (an override of 2 or 8 lost, 1.05M / 1.25M against 1.26M:
// DESIGN §4d, profiles/round6/r6sp1_nature_split_ab.txt)
static int fc_split(int64_t B) {
  return a3c_gemm_effective_split(NT_FLAT, a3c_gemm_plan_split((int)B, NT_FC, NT_FLAT, 512));
}
// the forward's workspace: the fc's split-K slabs, then room for the prepared block of a per-op call
static int64_t nat_fwd_slab_floats(int64_t B) {
  const int sp = fc_split(B);
  const int64_t fc = sp > 1 ? (int64_t)sp * B * NT_FC : 0;
  return (fc + 63) / 64 * 64;
}
int64_t a3c_nat_fwd_ws_floats(int64_t B) { return nat_fwd_slab_floats(B) + A3C_NAT_PREP_BYTES / 4; }
int64_t a3c_nat_bwd_ws_floats(const NetLayout& L, int64_t B) { return nat_plan(L, B).total; }

// one pass of the forward (B states) or of the backward (B samples, buffers of the plan in bws).
// The backward tiles, per pass <MODE, LAYER, BN, TA, TB, NBUF, PF>: three bf16 terms per operand in
// the fp32 mode (conv1 dW's u8 pixels: one), one in the bf16 mode; one LDS buffer
// (NBUF 1: two time faster alone on the dW passes but cost the concurrent rollout its co-residency,
// 1.20M against 1.28M, profiles/round6/r6pf3_nature_variant_bench_ab.txt); conv1 dW alone keeps two
// buffers and two slices in registers (PF 2: 1.33M against 1.28M without,
// r6pf4_nature_knob_bench_ab.txt).  The fc's GEMMs on these tiles lost to gemm.hip (r6fc1_nature_fc_bf_ab.txt: 1.27M / 1.30M
// / 1.32M against 1.33M); conv3 dX + conv2 dX as one per-sample kernel lost too (153 us alone against
// 85 + 107, but 1.51M against 1.60M: its 52 KB workgroups keep the rollout's conv workgroups off
// their CUs, r6fu_nature_fusion_ab.txt, r6dxp_nature_dx_fc_ab.txt).  All in DESIGN §4d.
int a3c_nat_pass_launch(int pass, const NetLayout& L, const float* P, const StateAddr& sa, int64_t B, const float* l1,
                        const float* l2, const float* l3, const float* l4, const uint16_t* w1t, float* fws,
                        float* bws, hipStream_t s, float* grads) {
  const bool b1 = L.prec == A3C_PREC_BF16;
  if (!w1t && pass >= NAT_C1F && pass <= NAT_C3F)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_pass_launch", "the conv forward needs the prepared block");
  switch (pass) {
    case NAT_C1F:
    case NAT_C3F:   // inside NAT_C2F's launch
      return 0;
    case NAT_C2F:   // conv1 + conv2 + conv3, one workgroup per state
      if (b1)
        hipLaunchKernelGGL(k_nat_conv123_b1, dim3((unsigned)B), dim3(256), 0, s, sa, w1t, P + L.off[N_L1B],
                           w1t + A3C_NAT_W2T_OFF / 2, P + L.off[N_L2B], w1t + A3C_NAT_W3T_OFF / 2, P + L.off[N_L3B],
                           (float*)l1, (float*)l2, (float*)l3, 1.0f / 255.0f);
      else
        hipLaunchKernelGGL(k_nat_conv23, dim3((unsigned)B), dim3(256), 0, s, w1t + A3C_NAT_W2T_OFF / 2,
                           P + L.off[N_L2B], w1t + A3C_NAT_W3T_OFF / 2, P + L.off[N_L3B], (float*)l2, (float*)l3, sa,
                           w1t, P + L.off[N_L1B], (float*)l1, 1.0f / 255.0f);
      A3C_CHECK(hipGetLastError());
      return 0;
    case NAT_FCF: {
      if (fws == nullptr) return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_pass_launch", "fc: no slab workspace");
      if (L.fc_prec == A3C_PREC_BF16)   // (its K chunks within the slabs of the fp32 plan)
        return a3c_nat_fc_fwd_launch(l3, P + L.off[N_FCW], P + L.off[N_FCB], (float*)l4, B, fws, fc_split(B), s);
      // l4 = relu(l3 W + b) (network.py:41-42, ops.py:41-44): split-K slabs, the fold applies the epilogue
      GemmArgs gf = {};
      gf.A = l3; gf.lda = NT_FLAT;
      gf.B = P + L.off[N_FCW]; gf.ldb = NT_FC;
      gf.C = (float*)l4; gf.ldc = NT_FC;
      gf.M = (int)B; gf.N = NT_FC; gf.K = NT_FLAT;
      gf.epi = EPI_BIAS_RELU; gf.bias = P + L.off[N_FCB];
      gf.nsplit = fc_split(B); gf.slab = fws;
      return a3c_gemm(true, true, gf, s);
    }
    default:
      break;
  }
  const NatPlan p = nat_plan(L, B);
  NatGemm a = {};
  switch (pass) {
    case NAT_FCW: {   // fc weights: dW[3136][512] = l3^T dl4 straight into grads (split-K inside the workgroups), db = colsum
      if (!grads) return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_pass_launch", "fc dW: no gradient buffer");
      if (L.fc_prec == A3C_PREC_BF16)
        return a3c_nat_fc_dw_launch(l3, bws + p.dl4, B, grads + L.off[N_FCW], bws + p.fccol, s);
      GemmArgs gf = {};
      gf.A = l3; gf.lda = NT_FLAT;
      gf.B = bws + p.dl4; gf.ldb = NT_FC;
      gf.C = grads + L.off[N_FCW]; gf.ldc = NT_FC;
      gf.M = NT_FLAT; gf.N = NT_FC; gf.K = (int)B;
      gf.epi = EPI_STORE; gf.colsum = bws + p.fccol; gf.wg_split = 4; gf.xcd = 1;
      return a3c_gemm(false, true, gf, s);
    }
    case NAT_FCX: {   // dl3 = (dl4 W^T) * (l3 > 0)
      if (L.fc_prec == A3C_PREC_BF16)
        return a3c_nat_fc_dx_launch(bws + p.dl4, P + L.off[N_FCW], l3, B, bws + p.dl3, s);
      GemmArgs gd = {};
      gd.A = bws + p.dl4; gd.lda = NT_FC;
      gd.B = P + L.off[N_FCW]; gd.ldb = NT_FC;
      gd.C = bws + p.dl3; gd.ldc = NT_FLAT;
      gd.M = (int)B; gd.N = NT_FLAT; gd.K = NT_FC;
      gd.epi = EPI_MASK; gd.mask = l3; gd.ldm = NT_FLAT; gd.nsplit = 1;
      return a3c_gemm(true, false, gd, s);
    }
    case NAT_C3W:     // dW3 (+ db3) over the (sample, pixel) rows
      a.X = l2; a.dY = bws + p.dl3; a.slab = bws + p.s3; a.colsum = bws + p.c3;
      a.M = NT_K3; a.N = NT3_N; a.K = (int)(B * NT3_P); a.kchunk = p.kc3;
      return b1 ? nat_go_bf<NG_DW, 3, 64, 1, 1, 1, 1>(a, (unsigned)p.ns3, s)
                : nat_go_bf<NG_DW, 3, 64, 3, 3, 1, 1>(a, (unsigned)p.ns3, s);
    case NAT_C3X:     // dl2 = col2im(dl3 W3^T) * (l2 > 0)
      a.X = l2; a.dY = bws + p.dl3; a.Wt = P + L.off[N_L3W]; a.Y = bws + p.dl2;
      a.M = (int)(B * NT2_P); a.N = NT2_N; a.K = 3 * 3 * NT3_N;
      return b1 ? nat_go_bf<NG_DX, 3, 64, 1, 1, 1, 1>(a, 1, s) : nat_go_bf<NG_DX, 3, 64, 3, 3, 1, 1>(a, 1, s);
    case NAT_C2W:
      a.X = l1; a.dY = bws + p.dl2; a.slab = bws + p.s2; a.colsum = bws + p.c2;
      a.M = NT_K2; a.N = NT2_N; a.K = (int)(B * NT2_P); a.kchunk = p.kc2;
      return b1 ? nat_go_bf<NG_DW, 2, 64, 1, 1, 1, 1>(a, (unsigned)p.ns2, s)
                : nat_go_bf<NG_DW, 2, 64, 3, 3, 1, 1>(a, (unsigned)p.ns2, s);
    case NAT_C2X:     // dl1 = col2im(dl2 W2^T) * (l1 > 0), per stride-2 parity class
      a.X = l1; a.dY = bws + p.dl2; a.Wt = P + L.off[N_L2W]; a.Y = bws + p.dl1;
      a.M = (int)(B * (NT1_O / 2) * (NT1_O / 2)); a.N = NT1_N; a.K = 2 * 2 * NT2_N;
      return b1 ? nat_go_bf<NG_DX, 2, 32, 1, 1, 1, 1>(a, 4, s) : nat_go_bf<NG_DX, 2, 32, 3, 3, 1, 1>(a, 4, s);
    case NAT_C1W:     // dW1 (+ db1) from the u8 planes (the input needs no gradient)
      a.sa = sa; a.dY = bws + p.dl1; a.slab = bws + p.s1; a.colsum = bws + p.c1;
      a.M = NT_K1; a.N = NT1_N; a.K = (int)(B * NT1_P); a.kchunk = p.kc1;
      return b1 ? nat_go_bf<NG_DW1, 1, 32, 1, 1, 2, 2>(a, (unsigned)p.ns1, s)
                : nat_go_bf<NG_DW1, 1, 32, 1, 3, 2, 2>(a, (unsigned)p.ns1, s);
    default:
      return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_pass_launch", "unknown pass");
  }
}

// the rollout's tau snapshot and the backward's go (k_prep_fwd's duties, without the NIPS weight
// preparation)
__global__ void k_nat_prep(const int64_t* __restrict__ tau_src, int64_t* __restrict__ tau_dst, uint32_t* sig) {
  if (tau_dst) *tau_dst = *tau_src;
  if (sig) (void)__hip_atomic_fetch_add(sig, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the three forward forms: three terms each, or rn(W) alone in the bf16 mode (the backward tiles
// split or round W at their LDS store)
static int nat_w1_terms_launch(const NetLayout& L, const float* P, uint16_t* w1t, hipStream_t s) {
  const int n = NT1_N * NT_K1 + NT2_N * NT_K2 + NT3_N * NT_K3;
  const dim3 grid((n + 255) / 256);
  if (L.prec == A3C_PREC_BF16)
    hipLaunchKernelGGL(k_nat_w_terms<1>, grid, dim3(256), 0, s, P + L.off[N_L1W], P + L.off[N_L2W], P + L.off[N_L3W], w1t);
  else
    hipLaunchKernelGGL(k_nat_w_terms<3>, grid, dim3(256), 0, s, P + L.off[N_L1W], P + L.off[N_L2W], P + L.off[N_L3W], w1t);
  A3C_CHECK(hipGetLastError());
  return 0;
}
int a3c_nat_prep_launch(const NetLayout& L, const float* P, uint16_t* w1t, const int64_t* tau_src, int64_t* tau_dst,
                        uint32_t* sig, hipStream_t s) {
  if (int rc = nat_w1_terms_launch(L, P, w1t, s)) return rc;
  hipLaunchKernelGGL(k_nat_prep, dim3(1), dim3(1), 0, s, tau_src, tau_src ? tau_dst : nullptr, sig);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
int a3c_nat_forward_launch(const NetLayout& L, const FwdArgs& a, hipStream_t s, const LaunchMode& m) {
  const float* P = a.params;
  const int64_t B = a.B;
  float *l3 = a.act_l3, *l4 = a.act_l4, *z = a.z, *ws = a.nat_ws;
  const HeadSelect& sel = *a.sel;
  const uint16_t* w1t = (const uint16_t*)a.prep;   // (a3c_nat_prep_launch's block)
  const uint8_t* play_frozen = a.play_frozen;
  if (L.trunk != A3C_TRUNK_NATURE || B <= 0 || B * NT1_P > 0x7fffffffLL)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_forward", "nature trunk, 0 < B, B * 400 < 2^31");
  if (play_frozen && !(sel.mode >= 0 && sel.env_on && sel.pool))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_forward", "the play step runs with the device env and the fused screen");
  if (!w1t) {   // one-off forward: the weight terms into the workspace's tail first
    uint16_t* t = (uint16_t*)(ws + nat_fwd_slab_floats(B));
    if (int rc = nat_w1_terms_launch(L, P, t, s)) return rc;
    w1t = t;
  }
  for (int pass = NAT_C1F; pass <= NAT_FCF; ++pass) {
    const int rc = a3c_nat_pass_launch(pass, L, P, a.sa, B, a.act_l1, a.act_l2, l3, l4, w1t, ws, nullptr, s);
    if (rc) return rc;
  }
  // the step tail; the fc's own fold stays in front of it (folding inside the head + screen kernel
  // lost, 1.29M against 1.33M: DESIGN §4d, profiles/round6/r6fh1_nature_fold_in_head_ab.txt)
  const bool step_tail = sel.mode >= 0 && sel.env_on && sel.pool;   // the engine's rollout step
  if (play_frozen)   // Agent.play's step tail (agent.py:371-377)
    return a3c_head_screen_play_launch(NT_FC, l4, P + L.off[N_HW], P + L.off[N_HB], P + L.off[N_VW], P + L.off[N_VB],
                                       L.A, L.zs, B, z, sel, play_frozen, s, m);
  if (step_tail)   // head + act + Environment.screen
    return a3c_head_screen_wide_launch(l4, P + L.off[N_HW], P + L.off[N_HB], P + L.off[N_VW], P + L.off[N_VB], L.A,
                                       L.zs, B, z, sel, s, m);
  if (sel.mode >= 0 && sel.env_on && sel.envp.game == A3C_GAME_CATCH)   // (the Catch form: end of this file)
    return nat_head_catch_launch(L, P, l4, B, z, sel, s);
  hipLaunchKernelGGL(k_nat_head<>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, l4, B, P + L.off[N_HW],
                     P + L.off[N_HB], P + L.off[N_VW], P + L.off[N_VB], L.A, L.zs, z, sel);
  A3C_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
// every tensor but the fc weights gets its gradient from a k_finalize segment
static bool nat_finalized(int t) { return t != N_FCW; }

int a3c_nat_fused_tab(const NetLayout& L, TensorTab* tt) {
  if (L.nt != N_NT) return -1;
  tt->n = L.nt;
  int nb = 0;
  for (int t = 0; t < L.nt; ++t) {
    tt->off[t] = L.off[t];
    tt->size[t] = L.size[t];
    tt->pb_first[t] = nb;
    tt->pb_count[t] = nat_finalized(t) ? FIN_X : (int)((L.size[t] + SS_CHUNK - 1) / SS_CHUNK);
    nb += tt->pb_count[t];
  }
  if (nb > SS_MAX_BLOCKS) return -1;
  tt->nblocks = nb;
  tt->total = L.total;
  return 0;
}

int a3c_nat_backward_launch(const NetLayout& L, const BwdArgs& args, hipStream_t s) {
  const float* P = args.params;
  const int64_t B = args.B;
  const float *l3 = args.act_l3, *l4 = args.act_l4;
  float *grads = args.grads, *ws = args.ws;
  const SumsqFused* sf = args.sf;
  const uint16_t* wt = args.nat_wt;
  if (L.trunk != A3C_TRUNK_NATURE || B <= 0 || B * NT1_P > 0x7fffffffLL)
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nat_backward", "nature trunk, 0 < B, B * 400 < 2^31");
  ReturnsArgs ra = {};
  if (args.ra) ra = *args.ra;
  const NatPlan p = nat_plan(L, B);
  if (!wt) {   // one-off backward: the weight terms into the workspace first
    uint16_t* t = (uint16_t*)(ws + p.wprep);
    if (int rc = nat_w1_terms_launch(L, P, t, s)) return rc;
    wt = t;
  }
  float* dz = ws + p.dz;
  float* dl4 = ws + p.dl4;
  float* terms = ws + p.terms;
  // returns (fused), losses, dz, dl4 = (dz [W_p W_v]^T) * (l4 > 0)
  int rc = a3c_head_bwd_launch(NT_FC, L, args.z, args.actions, args.target, l4, P + L.off[N_HW], P + L.off[N_VW],
                               args.beta, args.literal, B, dz, dl4, terms, ra, 1, s);
  if (rc) return rc;
  // head weights: dW[512][zs] = l4^T dz (split-K folded by the finalize), db = colsum(dz)
  GemmArgs gh = {};
  gh.A = l4; gh.lda = NT_FC;
  gh.B = dz; gh.ldb = L.zs;
  gh.C = ws + p.hgrad; gh.ldc = L.zs;
  gh.M = NT_FC; gh.N = L.zs; gh.K = (int)B;
  gh.epi = EPI_STORE; gh.slab = ws + p.hslab; gh.nsplit = p.head_split; gh.colsum = ws + p.hcol;
  gh.defer_reduce = 1;
  rc = a3c_gemm(false, true, gh, s);
  if (rc) return rc;
  // the fc's weight and input gradients (passes of their own), then the conv passes
  for (int pass = NAT_FCW; pass <= NAT_FCX; ++pass) {
    rc = a3c_nat_pass_launch(pass, L, P, args.sa, B, args.act_l1, args.act_l2, l3, l4, wt, nullptr, ws, s, grads);
    if (rc) return rc;
  }
  for (int pass = NAT_C3W; pass <= NAT_C1W; ++pass) {
    rc = a3c_nat_pass_launch(pass, L, P, args.sa, B, args.act_l1, args.act_l2, l3, l4, wt, nullptr, ws, s);
    if (rc) return rc;
  }
  // the weight slabs in NAT_GROUPS fixed-order groups, then k_finalize: every segment, the loss
  // terms, the fused per-tensor norms and the lr schedule
  const int g1 = p.ns1 < NAT_GROUPS ? p.ns1 : NAT_GROUPS, g2 = p.ns2 < NAT_GROUPS ? p.ns2 : NAT_GROUPS,
            g3 = p.ns3 < NAT_GROUPS ? p.ns3 : NAT_GROUPS;
  rc = a3c_slab_group_launch(ws + p.s1, p.ns1, g1, (int64_t)NT_K1 * NT1_N, ws + p.g1, s);
  if (!rc) rc = a3c_slab_group_launch(ws + p.s2, p.ns2, g2, (int64_t)NT_K2 * NT2_N, ws + p.g2, s);
  if (!rc) rc = a3c_slab_group_launch(ws + p.s3, p.ns3, g3, (int64_t)NT_K3 * NT3_N, ws + p.g3, s);
  if (rc) return rc;
  FinalizeSegs fs = {};
  fs.dst = grads;
  auto seg = [&](const float* src, int64_t stride, int nsplit, int rows, int src_ld, int col0, int ncols, int tensor,
                 int dst_ld, float scale) {
    FinalizeSeg& q = fs.s[fs.n++];
    q.src = src; q.split_stride = stride; q.nsplit = nsplit; q.rows = rows; q.src_ld = src_ld;
    q.col0 = col0; q.ncols = ncols; q.dst_off = L.off[tensor]; q.dst_ld = dst_ld; q.scale = scale;
    q.slot = sf ? sf->tt->pb_first[tensor] : -1;
  };
  // the patch rows of conv1 are raw u8 pixels: dW1 takes the 1/255 of the input scaling here
  seg(ws + p.g1, (int64_t)NT_K1 * NT1_N, g1, 1, 0, 0, NT_K1 * NT1_N, N_L1W, 0, 1.0f / 255.0f);
  seg(ws + p.c1, NT1_N, p.ns1, 1, 0, 0, NT1_N, N_L1B, 0, 1.0f);
  seg(ws + p.g2, (int64_t)NT_K2 * NT2_N, g2, 1, 0, 0, NT_K2 * NT2_N, N_L2W, 0, 1.0f);
  seg(ws + p.c2, NT2_N, p.ns2, 1, 0, 0, NT2_N, N_L2B, 0, 1.0f);
  seg(ws + p.g3, (int64_t)NT_K3 * NT3_N, g3, 1, 0, 0, NT_K3 * NT3_N, N_L3W, 0, 1.0f);
  seg(ws + p.c3, NT3_N, p.ns3, 1, 0, 0, NT3_N, N_L3B, 0, 1.0f);
  seg(ws + p.fccol, NT_FC, 1, 1, 0, 0, NT_FC, N_FCB, 0, 1.0f);
  const float* hsrc = p.head_split > 1 ? ws + p.hslab : ws + p.hgrad;
  const int64_t hstride = (int64_t)NT_FC * L.zs;
  seg(hsrc, hstride, p.head_split, NT_FC, L.zs, 0, L.A, N_HW, L.A, 1.0f);
  seg(ws + p.hcol, L.zs, p.head_split, 1, 0, 0, L.A, N_HB, 0, 1.0f);
  seg(hsrc, hstride, p.head_split, NT_FC, L.zs, L.A, 1, N_VW, 1, 1.0f);
  seg(ws + p.hcol, L.zs, p.head_split, 1, 0, L.A, 1, N_VB, 0, 1.0f);
  int nsumblk = 0;
  if (sf) {
    fs.part = sf->part;
    fs.tt = *sf->tt;
    fs.op = *sf->op;
    fs.sum_c0[0] = 0;
    fs.sum_t[0] = N_FCW;
    fs.sum_c0[1] = fs.tt.pb_count[N_FCW];
    fs.nsum = 1;
    nsumblk = fs.sum_c0[1];
  }
  return a3c_finalize_launch(fs, nsumblk, terms, B, args.loss_out, s);
}

// ---------------------------------------------------------------------------------------
// C-ABI: the nature trunk as stateless per-op calls (include/a3c_hip.h), for src/network.py
// ---------------------------------------------------------------------------------------
static int nat_layout(const a3c_net_desc* net, NetLayout* L, const char* what) {
  if (a3c_make_layout(net, L) || L->trunk != A3C_TRUNK_NATURE)
    return a3c_set_error(A3C_ERR_INVALID, what, "a nature-trunk net description (a3c, no LSTM)");
  return 0;
}
static StateAddr nat_states(const uint8_t* states, int64_t B) {
  StateAddr sa;
  sa.base = states; sa.env_stride = (int64_t)HIST * PLANE; sa.plane_bytes = PLANE;
  sa.E = (int)B; sa.R = HIST; sa.L = HIST; sa.tau_offset = HIST - 1; sa.tau_ptr = nullptr;
  return sa;
}
static float* nat_align(void* ws) { return (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255); }

extern "C" int a3c_nature_workspace_bytes(const a3c_net_desc* net, int64_t B, int64_t* bytes) {
  NetLayout L;
  if (int rc = nat_layout(net, &L, "a3c_nature_workspace_bytes")) return rc;
  if (B < 1 || !bytes) return a3c_set_error(A3C_ERR_INVALID, "a3c_nature_workspace_bytes", "bad argument");
  const int64_t f = a3c_nat_fwd_ws_floats(B), b = a3c_nat_bwd_ws_floats(L, B);
  *bytes = (f > b ? f : b) * 4 + 256;
  return 0;
}

static int nat_prec_ok(int precision, const char* what) {
  if (precision != A3C_PREC_FP32 && precision != A3C_PREC_BF16)
    return a3c_set_error(A3C_ERR_INVALID, what, "precision: A3C_PREC_FP32 or A3C_PREC_BF16");
  return 0;
}

extern "C" int a3c_nature_forward_prec2(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                                        float* l1, float* l2, float* l3, float* l4, float* z, void* workspace,
                                        void* stream, int precision, int fc_precision) {
  NetLayout L;
  if (int rc = nat_prec_ok(precision, "a3c_nature_forward")) return rc;
  if (int rc = nat_prec_ok(fc_precision, "a3c_nature_forward")) return rc;
  if (int rc = nat_layout(net, &L, "a3c_nature_forward")) return rc;
  L.prec = precision;
  L.fc_prec = fc_precision;
  if (!params || !states || !l1 || !l2 || !l3 || !l4 || !z || !workspace || B < 0 || B * NT1_P > 0x7fffffffLL ||
      (((uintptr_t)params | (uintptr_t)l1 | (uintptr_t)l2 | (uintptr_t)l3 | (uintptr_t)l4) & 15))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nature_forward", "bad argument");
  if (B == 0) return 0;
  HeadSelect sel = {};
  sel.mode = -1;
  sel.E = 1;
  FwdArgs a = {};   // (no prepared block: made in the workspace)
  a.params = params; a.sa = nat_states(states, B); a.B = B; a.z = z; a.sel = &sel;
  a.act_l1 = l1; a.act_l2 = l2; a.act_l3 = l3; a.act_l4 = l4; a.nat_ws = nat_align(workspace);
  return a3c_nat_forward_launch(L, a, (hipStream_t)stream, LAUNCH_ALONE);
}
extern "C" int a3c_nature_forward_prec(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                                       float* l1, float* l2, float* l3, float* l4, float* z, void* workspace,
                                       void* stream, int precision) {
  return a3c_nature_forward_prec2(net, params, states, B, l1, l2, l3, l4, z, workspace, stream, precision,
                                  A3C_PREC_FP32);
}
extern "C" int a3c_nature_forward(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                                  float* l1, float* l2, float* l3, float* l4, float* z, void* workspace,
                                  void* stream) {
  return a3c_nature_forward_prec(net, params, states, B, l1, l2, l3, l4, z, workspace, stream, A3C_PREC_FP32);
}

extern "C" int a3c_nature_loss_backward_prec2(const a3c_net_desc* net, const float* params, const uint8_t* states,
                                              int64_t B, const float* l1, const float* l2, const float* l3,
                                              const float* l4, const float* z, const int32_t* actions,
                                              const float* target, float beta, int literal_adv, float* grads,
                                              float* loss_out, void* workspace, void* stream, int precision,
                                              int fc_precision) {
  NetLayout L;
  if (int rc = nat_prec_ok(precision, "a3c_nature_loss_backward")) return rc;
  if (int rc = nat_prec_ok(fc_precision, "a3c_nature_loss_backward")) return rc;
  if (int rc = nat_layout(net, &L, "a3c_nature_loss_backward")) return rc;
  L.prec = precision;
  L.fc_prec = fc_precision;
  if (!params || !states || !l1 || !l2 || !l3 || !l4 || !z || !actions || !target || !grads || !workspace ||
      B <= 0 || B * NT1_P > 0x7fffffffLL || (((uintptr_t)grads | (uintptr_t)l3 | (uintptr_t)l4) & 15))
    return a3c_set_error(A3C_ERR_INVALID, "a3c_nature_loss_backward", "bad argument");
  BwdArgs a = {};   // (no fused returns or norms, no prepared weight terms)
  a.params = params; a.sa = nat_states(states, B); a.B = B;
  a.act_l1 = l1; a.act_l2 = l2; a.act_l3 = l3; a.act_l4 = l4; a.z = z; a.actions = actions; a.target = target;
  a.beta = beta; a.literal = literal_adv; a.grads = grads; a.loss_out = loss_out; a.ws = nat_align(workspace);
  return a3c_nat_backward_launch(L, a, (hipStream_t)stream);
}
extern "C" int a3c_nature_loss_backward_prec(const a3c_net_desc* net, const float* params, const uint8_t* states,
                                             int64_t B, const float* l1, const float* l2, const float* l3,
                                             const float* l4, const float* z, const int32_t* actions,
                                             const float* target, float beta, int literal_adv, float* grads,
                                             float* loss_out, void* workspace, void* stream, int precision) {
  return a3c_nature_loss_backward_prec2(net, params, states, B, l1, l2, l3, l4, z, actions, target, beta, literal_adv,
                                        grads, loss_out, workspace, stream, precision, A3C_PREC_FP32);
}
extern "C" int a3c_nature_loss_backward(const a3c_net_desc* net, const float* params, const uint8_t* states,
                                        int64_t B, const float* l1, const float* l2, const float* l3, const float* l4,
                                        const float* z, const int32_t* actions, const float* target, float beta,
                                        int literal_adv, float* grads, float* loss_out, void* workspace,
                                        void* stream) {
  return a3c_nature_loss_backward_prec(net, params, states, B, l1, l2, l3, l4, z, actions, target, beta, literal_adv,
                                       grads, loss_out, workspace, stream, A3C_PREC_FP32);
}

// Catch: k_nat_head's A3C_GAME_CATCH instantiation, emitted behind every other kernel
// of this file
static int nat_head_catch_launch(const NetLayout& L, const float* P, const float* l4, int64_t B, float* z,
                                 const HeadSelect& sel, hipStream_t s) {
  hipLaunchKernelGGL(k_nat_head<A3C_GAME_CATCH>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, l4, B, P + L.off[N_HW],
                     P + L.off[N_HB], P + L.off[N_VW], P + L.off[N_VB], L.A, L.zs, z, sel);
  A3C_CHECK(hipGetLastError());
  return 0;
}
