#pragma once
#include "net.h"
#include "lstm.h"
#include "optim.h"

// per-workgroup partial slab of k_conv_bwd: dW1 [256][16] (unscaled by 1/255), dW2 [256][32],
// db1 [16], db2 [32]
#define CB_OFF_W1 0
#define CB_OFF_W2 (KC1 * C1_N)                    // 4096
#define CB_OFF_B1 (CB_OFF_W2 + KC2 * C2_N)         // 12288
#define CB_OFF_B2 (CB_OFF_B1 + C1_N)               // 12304
#define CB_SLAB (CB_OFF_B2 + C2_N)                 // 12336

struct FinalizeSeg {
  const float* src;       // element (r, c) of split s: src[s*split_stride + r*src_ld + col0 + c]
  int64_t split_stride;
  int nsplit, rows, src_ld, col0, ncols;
  int64_t dst_off;        // dst[dst_off + r*dst_ld + c] = scale * sum_s
  int dst_ld;
  float scale;
  int slot;               // >= 0: block x of the segment writes its fp64 sum of squares to part[slot + x]
};
#ifndef FIN_X
#define FIN_X 32          // k_finalize blocks per segment
#endif
struct FinalizeSegs {
  FinalizeSeg s[12];
  int n;
  float* dst;
  // fused per-tensor norms (engine): the segments' partials as above, then one block per
  // SS_CHUNK of the tensors the segments do not write (already final: fc weights, LSTM) and the
  // lr / target-sync schedule -- what k_sumsq would compute, without its launch
  double* part;           // nullptr: none of this
  TensorTab tt;           // partial layout (a3c_fused_tab)
  int nsum;               // tensors summed by chunk blocks
  int sum_t[4];           // their indices
  int sum_c0[5];          // prefix sums of their chunk counts
  OptParams op;
  int no_tail;            // 1: no loss / schedule block (the split backward's second finalize)
};

// engine form of the per-tensor norms: k_finalize produces the partials (layout tt) and the schedule
struct SumsqFused {
  double* part;
  const TensorTab* tt;
  const OptParams* op;
};
// the partial layout SumsqFused expects: FIN_X slots for each tensor a finalize segment writes,
// SS_CHUNK chunks for the others
int a3c_fused_tab(const NetLayout& L, TensorTab* tt);

// Split exchange (multi-GPU): the fc / head gradients -- 99 % of the bytes -- are final
// before the conv backward starts, so the backward finalizes, norms and clips them first, records
// ev_head (the exchange of that range starts on a comm stream under the conv backward), then the
// conv tensors.  Bit-identical to the one-pass clip: the same partials, the same clip math.
struct SplitBwd {
  hipEvent_t ev_head;     // recorded on the backward's stream once grads[cut:] are clipped
  OptParams clip;         // the per-worker clip (mode OPT_CLIP), its range set per pass
  float* sumsq_out;       // per-tensor squared norms (written by the second pass, all tensors)
  int64_t cut;            // float offset of the fc weights: conv tensors [0, cut), the rest [cut, total)
};

struct BwdPlan {
  int nwg, per_wg, head_split, fc_split, groups;
  int64_t dz, dh3, dl2, terms, hgrad, hcol, hslab, fccol, fcslab, cslab, cgroup, total;  // float offsets
};

// optional fused n-step returns in the head backward (engine a3c path)
struct ReturnsArgs {
  const float* rewards;      // [n][E] (nullptr: use the explicit target array)
  const uint8_t* terms;      // [n][E]
  const float* boot;         // V(s_{t+n}) at boot[e * boot_stride]
  int64_t boot_stride;
  int n;
  int64_t E;
  double gamma;
  float* R_out;              // [n*E] the returns (inspection)
  // GAE(lambda) (values != nullptr): the target is the lambda-return A_t + V_t of k_gae
  const float* values;       // V(s_i) of env e at values[(i*E + e) * value_stride]: the rollout's own
  int64_t value_stride;
  double lambda;
};

// C5 LSTM head: the rollout's sequence buffers (engine slot) for the truncated BPTT; the
// terminals come from ReturnsArgs.terms
struct LstmBwd {
  int n;
  int64_t E;
  const float *h, *c, *hp, *cp, *gates;   // [n][E][...]
  float* dh;                              // [n*E][U] scratch: dL/dh_t from the heads
  float* ws;                              // a3c_lstm_ws_floats(n, E) floats
};

BwdPlan a3c_bwd_plan(const NetLayout& L, int64_t B, bool wks = false);
// What a loss + backward over B samples takes, on either trunk (a host-side bundle: no kernel sees
// it).  BwdArgs a = {} asks for no optional feature.  a3c_backward_launch dispatches on L.trunk: the
// NIPS body (net_bwd.hip) or a3c_nat_backward_launch (nature.hip).
struct BwdArgs {
  const float* params;
  StateAddr sa;
  int64_t B;
  const float *act_l1, *act_l2, *act_l3, *act_l4;   // l4: nature trunk only
  const float *z, *target;
  const int32_t* actions;
  float beta;
  int literal;
  float *grads, *loss_out;   // every tensor's gradient in the layout's order; [4] the loss terms, summed
  float* ws;                 // a3c_bwd_plan(L, B).total floats (nature: a3c_nat_bwd_ws_floats(L, B))
  // optional (lb, sp, l2m: NIPS trunk)
  const ReturnsArgs* ra;
  const SumsqFused* sf;
  const LstmBwd* lb;
  const SplitBwd* sp;
  const uint32_t* l2m;       // act_l2's ReLU bits (the dl2 epilogue reads them instead of l2)
  const uint16_t* nat_wt;    // nature: the prepared weight terms of params (null: prepared into ws first)
};
int a3c_backward_launch(const NetLayout& L, const BwdArgs& a, hipStream_t s, const LaunchMode& m);
int a3c_returns_launch(const float* rewards, const uint8_t* terms, const float* boot, int64_t boot_stride,
                       int n, int64_t E, double gamma, float* R, hipStream_t s);
int a3c_gae_launch(const float* rewards, const uint8_t* terms, const float* values, int64_t vstride,
                   const float* boot, int64_t boot_stride, int n, int64_t E, double gamma, double lambda, float* R,
                   float* adv, hipStream_t s);
// qsel != nullptr: double Q-learning -- the value of qn's row at qsel's row argmax (agent.py:176-184)
int a3c_td_target_launch(const float* rewards, const uint8_t* terms, const float* qn, int64_t B, int A,
                         int zs, double discount, float* target, hipStream_t s, const float* qsel = nullptr);
// n-step Q-learning: target [n][E] from the Q rows qb [E][zs] of the bootstrap state s_n (max over
// A, or with qsel the value at qsel's row argmax) and k_returns' recursion with `discount`
int a3c_nstep_q_target_launch(const float* rewards, const uint8_t* terms, const float* qb, const float* qsel, int n,
                              int64_t E, int A, int zs, double discount, float* target, hipStream_t s);
// Sarsa: boot_action [sel.E] <- the draw the rollout's head would make at step *tau0 + n (tau0 null:
// at step n) from the Q rows q [E][zs] (sel: mode 1, key, env ids, eps / the schedule with tau_ptr the counters:
// only tau_ptr[2] is read)
int a3c_boot_action_launch(const HeadSelect& sel, const int64_t* tau0, int64_t n, const float* q, int zs, int A,
                           int32_t* boot_action, hipStream_t s);
// the draw of a_n fused into the target kernel (the engine): a3c_boot_action_launch's arguments
struct BootDraw {
  HeadSelect sel;
  const int64_t* tau0;      // the slot's rollout-start tau (device); the draw's step is *tau0 + n
  const float* q;           // [E][zs] the slot's own parameters' Q rows of s_n
  int32_t* boot_action;     // [E] out
};
// target [n][E] at the taken actions: qt [n*E][zs] of s_1..s_n (nstep 0, k_td_target's form) or [E][zs] of s_n
// (nstep 1, k_nstep_q_target's recursion); a' = actions[i+1][e], boot[e] behind the rollout.  draw != nullptr:
// boot is not read -- the kernel draws a_n itself, as a3c_boot_action_launch would, and writes draw->boot_action
int a3c_sarsa_target_launch(const float* rewards, const uint8_t* terms, const int32_t* actions, const int32_t* boot,
                            const float* qt, int nstep, int n, int64_t E, int A, int zs, double discount,
                            float* target, hipStream_t s, const BootDraw* draw = nullptr);
// lambda-return Q targets: target [n][E] from qt [n*E][zs] of s_1..s_n; the bootstrap value of s_{i+1}
// is the row's max, with qsel [n*E][zs] its value at qsel's row argmax (double Q), with actions and boot (both or
// neither, never with qsel) its value at a' = actions[i+1][e], boot[e] behind the rollout (Sarsa).  draw != nullptr
// (with actions): boot is not read -- the kernel draws a_n itself, as a3c_sarsa_target_launch's does
int a3c_lambda_q_target_launch(const float* rewards, const uint8_t* terms, const int32_t* actions, const int32_t* boot,
                               const float* qt, const float* qsel, int n, int64_t E, int A, int zs, double discount,
                               double lambda, float* target, hipStream_t s, const BootDraw* draw = nullptr);
int a3c_select_launch(const float* z, int64_t B, int zs, int A, const HeadSelect& sel, hipStream_t s);
void a3c_init_once();   // (capi.hip: the two below, once per process)
void a3c_conv12_set_smem();
void a3c_conv_bwd_set_smem();
int a3c_head_screen_fold_launch(const float* part, int nsplit, const float* fbias, float* l4, const float* Wp,
                                const float* bp, const float* Wv, const float* bv, int A, int zs, int64_t B, float* z,
                                const HeadSelect& sel, hipStream_t s, const LaunchMode& m);
int a3c_head_screen_wide_launch(const float* l4, const float* Wp, const float* bp, const float* Wv, const float* bv,
                                int A, int zs, int64_t B, float* z, const HeadSelect& sel, hipStream_t s,
                                const LaunchMode& m);
int a3c_head_screen_launch(const NetLayout& L, const float* P, const float* act_l3, int64_t B, float* z,
                           const HeadSelect& sel, hipStream_t s, const LaunchMode& m);
int a3c_head_screen_conv12_launch(const NetLayout& L, const float* P, const float* act_l3, int64_t B, float* z,
                                  const HeadSelect& sel, const Conv12Next& nx, hipStream_t s);
int a3c_conv12_launch(const NetLayout& L, const float* P, const uint8_t* prep, const StateAddr& sa, int64_t B,
                      float* act_l1, float* act_l2, hipStream_t s, const LaunchMode& m, uint32_t* l2m = nullptr);
int a3c_conv_bwd_launch(const NetLayout& L, const float* P, const StateAddr& sa, int64_t B, const float* act_l1,
                        const float* dl2, float* ws, hipStream_t s, const LaunchMode& m);

// shared with the nature trunk (nature.hip): the head backward at width 256 (FC) or 512, the
// deterministic slab grouping, and k_finalize (segments + loss terms + fused norms / schedule)
int a3c_head_bwd_launch(int width, const NetLayout& L, const float* z, const int32_t* actions, const float* target,
                        const float* h, const float* Wp, const float* Wv, float beta, int literal, int64_t B,
                        float* dz, float* dh, float* terms, const ReturnsArgs& ra, int relu, hipStream_t s);
int a3c_slab_group_launch(const float* src, int nsplit, int groups, int64_t len, float* dst, hipStream_t s);
int a3c_finalize_launch(const FinalizeSegs& fs, int nsumblk, const float* terms, int64_t B, float* loss_out,
                        hipStream_t s);
