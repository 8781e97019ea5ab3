// C5 LSTM policy head (BASELINE config 5).  Build-defined: the reference has no recurrent code
// (SURVEY §8(f) rank 4).  Cell = TF1 BasicLSTMCell (gate columns i, j, f, o; forget_bias 1.0)
// on the fc ReLU output; the policy / value heads read h.  Oracle: oracle/ref_cpu.py lstm_*.
#pragma once
#include "net.h"

// one step of the cell for B envs.  h_src / c_src: the previous step's raw outputs, zeroed
// where prev_terms[e] (the previous transition was terminal).  hp / cp / gates nullable.
struct LstmStep {
  const float* wt;          // gate matrix transposed, [1024][512] (a3c_lstm_transpose_launch)
  const float* h_src;
  const float* c_src;
  const uint8_t* prev_terms;
  float *hp, *cp, *gates, *h, *c;
  // the cell's input as the fc layer's FC_NS K-slice partials (a3c_fc_part_launch), folded by the
  // cell kernel in slice order + fc bias + ReLU (as the feed-forward head folds them); the folded
  // rows go to l3_out (the backward's act_l3).  nullptr: x is the finished fc output
  const float* fc_part = nullptr;
  const float* fc_bias = nullptr;
  float* l3_out = nullptr;
  // with fc_part set by the caller: the fc launch folds its own partials (k_fc_part_fold, one
  // ticket word per fc tile) and the cell reads the finished rows
  unsigned* fc_tick = nullptr;
};

#define LT 16                    // envs per workgroup tile (both precisions)

__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

int a3c_lstm_fwd_launch(const float* bias, const float* x, const LstmStep& st, int64_t B, hipStream_t s);
// Wt[1024][512] = W[512][1024]^T (once per parameter version: the rollout's forward operand)
int a3c_lstm_transpose_launch(const float* W, float* Wt, hipStream_t s);

// truncated BPTT over n steps of E envs (see include/a3c_hip.h a3c_lstm_bptt)
struct LstmSeq {
  const float *x, *hp, *cp, *gates, *c;   // [n][E][...]
  const uint8_t* terms;                   // [n][E]
};
int64_t a3c_lstm_ws_floats(int n, int64_t E);
// parts: LSTM_BPTT_CHAIN (the cell backwards and the n step launches: da into ws, dx) | LSTM_BPTT_DW (dw, db from
// the da in ws); a3c_engine_time_kernel runs them apart
#define LSTM_BPTT_CHAIN 1
#define LSTM_BPTT_DW 2
int a3c_lstm_bptt_launch(const float* W, int n, int64_t E, const LstmSeq& q, const float* dh, float* dx,
                         float* dw, float* db, float* ws, hipStream_t s, int parts = LSTM_BPTT_CHAIN | LSTM_BPTT_DW);

// cell backward of step t at (e, u) given dh (heads + recurrence) and the carried dc
__device__ inline void lstm_cell_bwd(int64_t e, int u, float dh, float dcn, const float* __restrict__ G,
                                     const float* __restrict__ C, const float* __restrict__ CP,
                                     float* __restrict__ dcp, float* __restrict__ DA) {
  const int64_t i = e * LSTM_U + u;
  const float* gp = G + e * LSTM_G + u;
  const float ig = gp[0], jg = gp[LSTM_U], fg = gp[2 * LSTM_U], og = gp[3 * LSTM_U];
  const float tc = tanhf(C[i]);
  const float dc = dcn + dh * og * (1.f - tc * tc);
  float* da = DA + e * LSTM_G + u;
  da[0] = dc * jg * ig * (1.f - ig);
  da[LSTM_U] = dc * ig * (1.f - jg * jg);
  da[2 * LSTM_U] = dc * CP[i] * fg * (1.f - fg);
  da[3 * LSTM_U] = dh * tc * og * (1.f - og);
  dcp[i] = dc * fg;
}

// one fused BPTT launch (k_lstm_bptt_step, k_lstm_bptt_step_bf)
struct BpttStep {
  const float* DAn;       // da of step t+1 [E][1024]
  const float* xn;        // x of step t+1 [E][256] (fc ReLU output: the dx mask)
  float* dxn;             // dx of step t+1 [E][256]
  int cell;               // 1: run the cell backward of step t in the h-half epilogue
  const float *G, *C, *CP, *dH;   // step t
  const uint8_t* terms;   // terms[t] [E]
  float* dcp;             // [E][U] carried dc (in: step t+1's dc*f, out: step t's)
  float* DA;              // da of step t [E][1024]
};
// the chain both precisions share: the cell backward of step n-1 (k_lstm_cell_bwd_last), then step(t, b) for
// t = n-2 .. -1 with b the launch's arguments; da [n*E][1024] and the carried dc are the first two blocks of ws
int a3c_lstm_bptt_chain(int n, int64_t E, const LstmSeq& q, const float* dh, float* dx, float* ws, hipStream_t s,
                        int (*step)(int t, int64_t E, const BpttStep& b, const void* W, hipStream_t s), const void* W);

// ---- bf16 compute mode (NetLayout::lstm_prec A3C_PREC_BF16; lstm_bf16.hip) ---------------------
// prep [2][512 * 1024] bf16 in the 2 MB of the fp32 transpose: rn(W)^T [1024][512], then rn(W) [512][1024]
int a3c_lstm_prep_bf_launch(const float* W, uint16_t* prep, hipStream_t s);
int a3c_lstm_fwd_bf_launch(const float* bias, const float* x, const LstmStep& st, int64_t B, hipStream_t s);   // st.wt: prep
int a3c_lstm_bptt_bf_launch(const uint16_t* prep, int n, int64_t E, const LstmSeq& q, const float* dh, float* dx,
                            float* dw, float* db, float* ws, hipStream_t s, int parts = LSTM_BPTT_CHAIN | LSTM_BPTT_DW);
