/*
 * a3c_hip.h -- C-ABI of liba3c_hip.so, the MI355X (gfx950) rollout + gradient path of
 * datavizweb/async-rl-tensorflow re-built as hand-written HIP kernels.
 *
 * The reference has no FFI: its boundary is the Python object API.
 * Each entry point below names the reference interface (file:line under the reference
 * root) whose arithmetic it replaces; the Python mirror in
 * async-rl-tensorflow_amd/src/ binds them through ctypes.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; every pointer is a CALLER-OWNED device buffer
 *    unless stated.  Nothing here allocates on the hot path; a3c_engine_create is the only
 *    allocating call (one-time workspace).
 *  - every call enqueues on the caller's stream (`stream` is a hipStream_t; NULL = legacy
 *    default stream) and returns an int status: 0 = ok, otherwise a hipError_t value or one
 *    of the A3C_ERR_* codes; a3c_last_error() gives the message.  No C++ exception crosses
 *    the ABI.  The Python side raises ValueError / RuntimeError (network.py:21,28,54).
 *  - no call is re-entrant on the same engine handle.
 */
#ifndef A3C_HIP_H
#define A3C_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A3C_OK 0
#define A3C_ERR_INVALID 10001   /* bad argument / unsupported shape            */
#define A3C_ERR_STATE 10002     /* engine used in the wrong order               */

#define A3C_ALGO_A3C 0          /* policy + value heads (src/network.py:60-94) */
#define A3C_ALGO_Q 1            /* one-step Q-learning head (src/agent.py:251-254) */

#define A3C_TRUNK_NIPS 0        /* 16/32/256 trunk: agent.py:226-251, network.py:43-52 */
#define A3C_TRUNK_NATURE 1      /* 32/64/64/512 trunk: network.py:30-42 (A3C heads only)   */
#define A3C_LSTM_UNITS 256      /* C5 LSTM head width (build-defined: the reference has no
                                   recurrent code)                 */

const char* a3c_version(void);
const char* a3c_last_error(void);
/* 1 when a gfx950 device is visible (no compute). */
int a3c_device_ok(void);

/* ----------------------------------------------------------------------------
 * Network description and flat parameter layout.
 * Flat fp32 vector in TF variable order (ops.py:21,24,36,38; agent.py:226-252 /
 * network.py:47-79); each tensor starts at a 64-float (256 B) aligned offset,
 * padding floats are zero and stay zero.
 *  a3c : l1_w[8,8,4,16] l1_b l2_w[4,4,16,32] l2_b l4_w[2592,256] l4_b p_w[256,A] p_b q_w[256,1] q_b
 *  q   : l1_w l1_b l2_w l2_b l3_w[2592,256] l3_b q_w[256,A] q_b
 *  a3c, nature trunk: l1_w[8,8,4,32] l1_b l2_w[4,4,32,64] l2_b l3_w[3,3,64,64] l3_b
 *        l4_w[3136,512] l4_b p_w[512,A] p_b q_w[512,1] q_b   (network.py:30-42, 62-79)
 *  a3c + LSTM head (lstm_units = 256, BASELINE config 5): the a3c list, then
 *        lstm_w[256+U, 4U] lstm_b[4U]   (TF1 BasicLSTMCell "Matrix"/"Bias", gate columns
 *        i, j, f, o, forget_bias 1.0); the policy / value heads read the LSTM's h.
 * -------------------------------------------------------------------------- */
typedef struct a3c_net_desc {
  int algo;            /* A3C_ALGO_*                                       */
  int trunk;           /* A3C_TRUNK_NIPS, or A3C_TRUNK_NATURE (algo A3C, no LSTM: the
                          engine only; the per-op a3c_forward / a3c_loss_backward are NIPS) */
  int action_size;     /* A (<= 31)                                        */
  int history_length;  /* 4 (config.py:22)                                 */
  int screen_h;        /* 84                                               */
  int screen_w;        /* 84                                               */
  int lstm_units;      /* 0: feed-forward head; A3C_LSTM_UNITS: LSTM head (a3c only).  The
                          batch-independent a3c_forward / a3c_loss_backward reject it (a
                          recurrent head needs the sequence: a3c_lstm_step / a3c_lstm_bptt
                          or the engine). */
} a3c_net_desc;

#define A3C_MAX_TENSORS 16
/* n_tensors, offsets[i], sizes[i] (floats), total padded length. */
int a3c_param_layout(const a3c_net_desc* net, int* n_tensors, int64_t* offsets, int64_t* sizes,
                     int64_t* total);
/* bytes of scratch a3c_forward / a3c_loss_backward need for batch B */
int a3c_workspace_bytes(const a3c_net_desc* net, int64_t B, int64_t* bytes);

/* ----------------------------------------------------------------------------
 * The nature trunk (network.py:30-42, Network(DQN_type='nature')): net->trunk =
 * A3C_TRUNK_NATURE, algo A3C, history_length 4.  Stateless forward / loss + backward over B
 * states (u8 planes [B][4][84][84], 16-B aligned), implicit-GEMM kernels of nature.hip:
 *   l1 [B][20][20][32], l2 [B][9][9][64], l3 [B][3136] (conv3 out, (h,w,c) flatten),
 *   l4 [B][512] (fc out), z [B][zs] (logits, value).  The backward (network.py:81-94 with the
 *   A11 fixes) reads the forward's activations; grads [total] in the flat layout, loss_out[4].
 * Replace network.py:30-42 + 81-94 (the TF graph of the nature trunk, its compute_gradients).
 * -------------------------------------------------------------------------- */
int a3c_nature_workspace_bytes(const a3c_net_desc* net, int64_t B, int64_t* bytes);
int a3c_nature_forward(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                       float* l1, float* l2, float* l3, float* l4, float* z, void* workspace, void* stream);
int a3c_nature_loss_backward(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                             const float* l1, const float* l2, const float* l3, const float* l4, const float* z,
                             const int32_t* actions, const float* target, float beta, int literal_adv,
                             float* grads, float* loss_out, void* workspace, void* stream);

/* ----------------------------------------------------------------------------
 * K1  Environment.screen (environment.py:49-53): fp64 luminance truncated to u8, then
 *     Pillow BILINEAR fixed-point resample (scipy.misc.imresize, environment.py:5-8).
 *     rgb frames [*, in_h, in_w, 3] u8; frame i reads rgb + (frame_idx ? frame_idx[i] : i)
 *     * in_h*in_w*3 and writes out + i*out_stride ([out_h][out_w] u8).  Bit-exact.
 * -------------------------------------------------------------------------- */
int a3c_preprocess_u8(const uint8_t* rgb, const int32_t* frame_idx, int64_t n, int in_h, int in_w,
                      uint8_t* out, int64_t out_stride, int out_h, int out_w, void* stream);

/* luminance step alone (environment.py:51-52): out[i] = uint8(fp64 0.2126R+0.7152G+0.0722B)
 * for npix RGB pixels, in the exact integer form the Atari screen kernel uses. */
int a3c_luminance_u8(const uint8_t* rgb, int64_t npix, uint8_t* out, void* stream);

/* ----------------------------------------------------------------------------
 * K2  History (history.py:3-27).  hist is [n][L][h*w] u8 (oldest plane first);
 *     push: if reset_mask && reset_mask[i]: zero (History.reset, :17-18); then shift one
 *     plane and append screens[i] (History.add, :13-15).
 *     get: float32 copy, NHWC [n][h][w][L] when nhwc else [n][L][h][w] (History.get, :20-24).
 * -------------------------------------------------------------------------- */
int a3c_history_push(uint8_t* hist, const uint8_t* screens, const uint8_t* reset_mask, int64_t n,
                     int L, int64_t hw, void* stream);
int a3c_history_get_f32(const uint8_t* hist, int64_t n, int L, int h, int w, int nhwc, float* out,
                        void* stream);

/* ----------------------------------------------------------------------------
 * Forward (agent.py:217-254 q-net / network.py:43-79 a3c net, ops.py:4-46).
 *  states  [B][L][84][84] u8 (frame values; the /255 of agent.py:226 is applied inside)
 *  act_l1  [B][400][16]  f32 conv1 out (nullable: only needed for a3c_loss_backward)
 *  act_l2  [B][2592]     f32 conv2 out, (h,w,c) flatten order (agent.py:231-232)
 *  act_l3  [B][256]      f32 fc out
 *  z       [B][zs]       f32 head: a3c -> A logits then V at column A; q -> A q-values.
 *                         zs = a3c_z_stride(net).
 * -------------------------------------------------------------------------- */
int a3c_z_stride(const a3c_net_desc* net);
int a3c_forward(const a3c_net_desc* net, const float* params, const uint8_t* states, int64_t B,
                float* act_l1, float* act_l2, float* act_l3, float* z, void* workspace,
                void* stream);

/* ----------------------------------------------------------------------------
 * K6  action selection.
 *  mode 0 (a3c, network.py:65-72 softmax + batch_sample): categorical draw
 *        u = philox(seed; tau, env_ids[i], P_ACTION); first j with fp32 cumsum(pi)[j] > u.
 *  mode 1 (q, agent.py:141-151): if u01(x0) < eps[i]: x1 % A  else argmax_j q[j]
 *        (first maximum, tf.argmax agent.py:254).
 *  env_ids nullable (= i).  eps nullable in mode 0.
 * -------------------------------------------------------------------------- */
int a3c_select_action(int mode, const float* z, int64_t B, int zs, int A, const float* eps,
                      uint64_t seed, int64_t tau, const int32_t* env_ids, int32_t* actions,
                      void* stream);

/* ----------------------------------------------------------------------------
 * K7  n-step returns (assets/a3c.png Algorithm S3) over [n][E] in float64:
 *     R = bootstrap[e] (0 if terminals[n-1]); R <- r_i + gamma*R, reset at terminals.
 *     TD target (agent.py:186-190): (1-term)*discount*max_a q_next[i][a] + reward[i] (fp64).
 * -------------------------------------------------------------------------- */
int a3c_returns(const float* rewards, const uint8_t* terminals, const float* bootstrap, int n,
                int64_t E, double gamma, float* R, void* stream);
int a3c_td_target(const float* rewards, const uint8_t* terminals, const float* q_next, int64_t B,
                  int A, int zs, double discount, float* target, void* stream);

/* ----------------------------------------------------------------------------
 * K7b  GAE(lambda) advantages and lambda-returns (Schulman et al.) over [n][E] in float64, with
 *     V_i = values[(i*E + e) * value_stride] and V_n = bootstrap[e], for i = n-1 .. 0:
 *       nt    = terminals[i][e] ? 0 : 1
 *       delta = r_i + gamma*nt*V_{i+1} - V_i
 *       A_i   = delta + gamma*lambda*nt*A_{i+1}                 (A_n = 0)
 *       R[i][e] = (float)(A_i + V_i)      adv[i][e] = (float)A_i      (adv nullable)
 *     lambda = 1: R is the n-step return of a3c_returns (to 1 ulp of float: V_i is added and
 *     subtracted in float64); lambda = 0: R = r_i + gamma*nt*V_{i+1}.
 *     A3C_ERR_INVALID: lambda outside [0, 1], n < 1, value_stride < 1, a null pointer (but adv).
 * -------------------------------------------------------------------------- */
int a3c_gae_returns(const float* rewards, const uint8_t* terminals, const float* values,
                    int64_t value_stride, const float* bootstrap, int n, int64_t E, double gamma,
                    double lambda, float* R, float* adv, void* stream);

/* ----------------------------------------------------------------------------
 * K7c  n-step Q-learning targets (asynchronous n-step Q-learning, Algorithm S2 of the A3C paper)
 *     over [n][E] in float64, contraction off, from the rollout's clipped rewards and terminals and
 *     the Q rows of the bootstrap state s_n (row e of q_boot / q_sel at + e*zs, A live columns):
 *       B_e = max_a q_boot[e][a]
 *             q_sel != NULL (double Q): q_boot[e][argmax_a q_sel[e][a]]   (the first maximum)
 *       R   = (double)B_e
 *       for i = n-1 .. 0:  if terminals[i][e]: R = 0;  R = rewards[i][e] + discount*R;
 *                          target[i][e] = (float)R
 *     n = 1 is a3c_td_target to the last bit.  The engine (cfg.q_nstep) takes q_boot from the
 *     target network and q_sel from the slot's own parameters.
 *     A3C_ERR_INVALID: a null pointer other than q_sel, n < 1, E < 1, A < 1, zs < A.
 * -------------------------------------------------------------------------- */
int a3c_nstep_q_target(const float* rewards, const uint8_t* terminals, const float* q_boot,
                       const float* q_sel, int n, int64_t E, int A, int zs, double discount,
                       float* target, void* stream);

/* ----------------------------------------------------------------------------
 * K7d  Sarsa: the bootstrap state's action (asynchronous one-step Sarsa, §4 and Algorithm S1 of the
 *     A3C paper with the target r + gamma Q(s', a'; theta^-), a' the action the behaviour policy
 *     takes in s').  The epsilon-greedy draw the rollout's head makes for env e at step tau
 *     (agent.py:141-151), from the Q rows q [E][zs] (A live columns):
 *       x = philox4x32(lo32(tau), hi32(tau), env_id_base + e, P_ACTION = 1; key = seed)
 *       boot_actions[e] = u01(x.x) < eps[e] ? x.y % A : the first argmax_a q[e][a]
 *     The engine (a3c_engine_opts.sarsa) draws it at tau = the slot's rollout-start tau + n with the
 *     slot's own parameters' rows of s_n and the schedule's epsilon of that step: rollout k+1's own
 *     first draw whenever the parameters did not change in between, and wherever u < eps.
 *     A3C_ERR_INVALID: a null pointer, E < 1, A < 1, zs < A.
 * -------------------------------------------------------------------------- */
int a3c_boot_action(const float* q, const float* eps, int64_t E, int A, int zs, int64_t tau,
                    int env_id_base, uint64_t seed, int32_t* boot_actions, void* stream);

/* ----------------------------------------------------------------------------
 * K7e  Sarsa targets (one-step Sarsa, §4 of the A3C paper; nstep: its n-step form, Algorithm S2's
 *     returns bootstrapped at the taken action) over [n][E] in float64, contraction off, from the
 *     rollout's clipped rewards, terminals and actions [n][E], the bootstrap state's action
 *     boot_actions [E] (a3c_boot_action) and the target network's Q rows q_target (A live columns,
 *     row stride zs).  An action word w is used as the column (uint32)w % A, so any word reads
 *     inside its row.
 *       nstep = 0, q_target [n*E][zs] the rows of s_1 .. s_n, b = i*E + e:
 *         a' = i < n-1 ? actions[i+1][e] : boot_actions[e]
 *         target[b] = (float)((1 - terminals[b]) * discount * (double)q_target[b][a'] + rewards[b])
 *       nstep = 1, q_target [E][zs] the rows of s_n:
 *         R = (double)q_target[e][boot_actions[e]]
 *         for i = n-1 .. 0:  if terminals[i][e]: R = 0;  R = rewards[i][e] + discount*R;
 *                            target[i][e] = (float)R
 *     After a terminal, actions[i+1] belongs to the new game and (1 - terminal) removes it.  n = 1:
 *     both forms are the same operations.  With a' the argmax of the same rows the targets are
 *     a3c_td_target's / a3c_nstep_q_target's to the last bit.
 *     A3C_ERR_INVALID: a null pointer, nstep not 0 or 1, n < 1, E < 1, A < 1, zs < A.
 * -------------------------------------------------------------------------- */
int a3c_sarsa_target(const float* rewards, const uint8_t* terminals, const int32_t* actions,
                     const int32_t* boot_actions, const float* q_target, int nstep, int n, int64_t E,
                     int A, int zs, double discount, float* target, void* stream);

/* ----------------------------------------------------------------------------
 * K7f  lambda-return Q targets over the rollout (the forward view: Peng's Q(lambda), its double-Q form
 *     and Sarsa(lambda)) over [n][E] in float64, contraction off, from the rollout's clipped rewards,
 *     terminals and actions [n][E] and the target network's Q rows of s_1 .. s_n, q_target [n*E][zs]
 *     (b = i*E + e, A live columns, columns >= A never read).  The bootstrap value B_i of s_{i+1}:
 *       Q:         max_a q_target[b][a]
 *       double Q   (q_sel != NULL, rows [n*E][zs] of the same states under the learner's own
 *                  parameters): q_target[b][argmax_a q_sel[b][a]]              (the first maximum)
 *       Sarsa      (actions, boot_actions != NULL): q_target[b][a'],
 *                  a' = i < n-1 ? actions[i+1][e] : boot_actions[e]; an action word w is used as the
 *                  column (uint32)w % A, so any word reads inside its row.
 *     and, for env e, with G = (double)B_{n-1} before the loop, for i = n-1 .. 0:
 *       mix = (1 - lambda) * B_i + lambda * G
 *       if terminals[i][e]: mix = 0
 *       G = rewards[i][e] + discount * mix
 *       target[i][e] = (float)G
 *     which is (1 - lambda) sum_k lambda^(k-1) G^(k) + lambda^(N-1) G^(N) over the k-step returns
 *     G^(k) of the rollout's remaining N = n - i steps, cut at the first terminal.  With finite
 *     inputs this operation order makes both ends exact: lambda = 0 gives mix = B_i + 0, that is
 *     a3c_td_target (with q_sel its double-Q form) / a3c_sarsa_target(nstep = 0) to the last bit;
 *     lambda = 1 gives mix = 0 + G, that is a3c_nstep_q_target / a3c_sarsa_target(nstep = 1) on the
 *     rows of s_n to the last bit.  The engine (a3c_engine_set_q_lambda) takes q_target from the
 *     target network, q_sel from the slot's own Q rows and boot_actions from a3c_boot_action's draw.
 *     No trace is cut at a non-greedy action (Watkins's Q(lambda) is not this rule).
 *     A3C_ERR_INVALID: a null rewards, terminals, q_target or target; q_sel together with actions /
 *     boot_actions; only one of actions / boot_actions; lambda outside [0, 1] or NaN; n < 1; E < 1;
 *     A < 1; zs < A.
 * -------------------------------------------------------------------------- */
int a3c_lambda_q_target(const float* rewards, const uint8_t* terminals, const int32_t* actions,
                        const int32_t* boot_actions, const float* q_target, const float* q_sel, int n,
                        int64_t E, int A, int zs, double discount, double lambda, float* target,
                        void* stream);

/* ----------------------------------------------------------------------------
 * K8+K9 loss + backward (network.py:81-94 with the SURVEY §8 A11 fixes / agent.py:306-317).
 *  target: a3c -> R (n-step return); q -> TD target.
 *  a3c loss per sample  -log pi(a)*stopgrad(R-V) - beta*H + (R-V)^2/2, summed over B
 *      (literal_adv != 0: no stop-gradient, network.py:83-84 literal form);
 *  q   loss mean((target - Q[a])^2) over B (agent.py:313-314).
 *  grads: flat fp32 (layout of a3c_param_layout), OVERWRITTEN.
 *  loss_out (device, 4 floats): a3c {policy_sum, value_sum, entropy_sum, total_sum};
 *                               q {loss, mean_q_acted, 0, 0}.
 * -------------------------------------------------------------------------- */
int a3c_loss_backward(const a3c_net_desc* net, const float* params, const uint8_t* states,
                      int64_t B, const float* act_l1, const float* act_l2, const float* act_l3,
                      const float* z, const int32_t* actions, const float* target, float beta,
                      int literal_adv, float* grads, float* loss_out, void* workspace,
                      void* stream);

/* ----------------------------------------------------------------------------
 * K10+K11  per-tensor clip_by_norm (agent.py:316-319) + TF ApplyRMSProp
 *  (main.py:63-65, agent.py:321): ms += (g^2-ms)(1-rho); mom = mom*momentum +
 *  lr*g/sqrt(ms+eps); w -= mom.  ms must be initialised to 1.0, mom to 0 (TF1 slots).
 *  clip <= 0 disables clipping.  sumsq_out (nullable, device, n_tensors floats) receives
 *  the pre-clip squared norms.  workspace >= a3c_optim_workspace_bytes().
 *  a3c_clip_grads only clips in place (multi-GPU: clip per worker, then all-reduce).
 * -------------------------------------------------------------------------- */
int a3c_optim_workspace_bytes(int64_t total, int64_t* bytes);
int a3c_clip_grads(float* grads, int n_tensors, const int64_t* offsets, const int64_t* sizes,
                   float clip, float* sumsq_out, void* workspace, void* stream);
int a3c_clip_rmsprop_apply(float* params, float* ms, float* mom, float* grads, int n_tensors,
                           const int64_t* offsets, const int64_t* sizes, float lr, float rho,
                           float momentum, float eps, float clip, float* sumsq_out,
                           void* workspace, void* stream);
/* The same pass with TF1 ApplyAdam: m += (g-m)(1-beta1); v += (g^2-v)(1-beta2);
 * w -= m*alpha / (sqrt(v) + eps), in fp32.  m and v must be initialised to 0.  The caller forms
 * alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) of the step t = 1, 2, ... it applies. */
int a3c_clip_adam_apply(float* params, float* m, float* v, float* grads, int n_tensors,
                        const int64_t* offsets, const int64_t* sizes, float alpha, float beta1,
                        float beta2, float eps, float clip, float* sumsq_out,
                        void* workspace, void* stream);

/* ----------------------------------------------------------------------------
 * Generic layer ops (ops.py:4-46 drop-ins, any shape; off the hot path).
 *  conv2d VALID, weights [kh,kw,cin,cout] (ops.py:16-21), x NHWC [N,H,W,C] or NCHW [N,C,H,W]
 *  (nhwc flag), y likewise; bias nullable; relu = activation_fn tf.nn.relu (ops.py:27-28).
 *  backward: dx (nullable) / dw, db (nullable) -- OVERWRITTEN.
 *  matmul: C[m][n] (+)= sum_k A[m*sam+k*sak] * B[k*sbk+n*sbn] (+bias[n]) (relu) -- linear
 *  (ops.py:41-46) and its gradients through the strides.
 * -------------------------------------------------------------------------- */
int a3c_conv2d_forward(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int C,
                       int KH, int KW, int SH, int SW, int OC, int nhwc, int relu, void* stream);
int a3c_conv2d_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int N,
                        int H, int W, int C, int KH, int KW, int SH, int SW, int OC, int nhwc, void* stream);
int a3c_matmul(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
               int64_t ldc, int M, int N, int K, const float* bias, int relu, int accumulate, void* stream);

/* ----------------------------------------------------------------------------
 * The fp32 matrix-core GEMM of the fc layers, their gradients and the LSTM gate gradients
 * (csrc/gemm.hip), alone: every tile form, operand layout and epilogue the engine can select,
 * so each can be tested and timed without an engine around it.
 *   C[m*ldc + n] = epi( sum_k A(m,k) * B(k,n) ),   m < M, n < N
 *   A(m,k) = a_kcontig ? A[m*lda + k] : A[k*lda + m];  B(k,n) = b_ncontig ? B[k*ldb + n] : B[n*ldb + k]
 *   epi: A3C_GEMM_STORE v; _BIAS_RELU max(v + bias[n], 0); _BIAS v + bias[n];
 *        _MASK mask[m*ldm + n] > 0 ? v : 0;
 *        _MASKBITS bit (n & 31) of maskbits[m*ldm + (n >> 5)] ? v : 0  (ldm in 32-bit words)
 *   nsplit:   requested split of K into chunks of whole 16-wide k-tiles; the effective split
 *             (a3c_gemm_workspace_bytes) may be smaller.  Effective split > 1: the partial tiles go to
 *             `workspace` [split][M][N] and a fold kernel applies epi.
 *   wg_split: 0, or 4 = K split over 4 wave groups inside each workgroup and folded in LDS (no
 *             workspace, effective split 1; another summation grouping than the slab split).
 *   big:      128x128 tiles; xcd: 0, 1, 2 tile order; max_wgs: 0 or a cap on the workgroups.  big
 *             ignores xcd and max_wgs, wg_split ignores nsplit, big and max_wgs.  Tile size, order
 *             and cap do not change a bit of the result.
 *   colsum:   nullable; row s of [effective split][N] = sum over K-chunk s of B(k, n) (one row
 *             with wg_split); the caller folds the rows.
 * Alignment: A, B and the workspace 16 bytes, the other pointers 4; lda and ldb % 4; K % 4 unless
 * (a k-strided, b n-contiguous); M % 4 when a is k-strided; N % 4 when b is n-contiguous.
 * A3C_ERR_INVALID, nothing launched: a NULL desc, A, B or C; bias / mask / maskbits NULL where epi
 * reads it; an unknown epi; M, N, K or nsplit < 1; a leading dimension shorter than its row; any
 * alignment rule above; effective split > 1 with workspace NULL or workspace_bytes too small;
 * wg_split not 0 or 4; xcd not 0, 1, 2; wg_split with xcd 2; max_wgs < 0.
 *  a3c_gemm_workspace_bytes: *nsplit_eff and *bytes (either nullable) of a launch with `nsplit`
 *             requested (wg_split launches need none).
 *  a3c_gemm_f32: one GEMM; *nsplit_eff (nullable) = the split the launch used.
 *  a3c_gemm3_f32: d[0..2] as ONE launch (the synchronous backward's dW_head, dW_fc, dl2) and then
 *             their split-K folds.  Layouts are fixed: d[0], d[1] (a k-strided, b n-contiguous),
 *             d[2] (a k-contiguous, b k-contiguous); wg_split, big, xcd, max_wgs must be 0.  Bit
 *             for bit the three a3c_gemm_f32 calls.
 * -------------------------------------------------------------------------- */
#define A3C_GEMM_STORE 0
#define A3C_GEMM_BIAS_RELU 1
#define A3C_GEMM_BIAS 2
#define A3C_GEMM_MASK 3
#define A3C_GEMM_MASKBITS 4
typedef struct a3c_gemm_desc {
  const float* A; int64_t lda;
  const float* B; int64_t ldb;
  float* C; int64_t ldc;
  const float* bias;
  const float* mask;
  const uint32_t* maskbits;
  int64_t ldm;
  float* colsum;
  int M, N, K;
  int a_kcontig, b_ncontig;
  int epi;
  int nsplit;
  int wg_split, big, xcd, max_wgs;
} a3c_gemm_desc;
int a3c_gemm_workspace_bytes(int M, int N, int K, int nsplit, int* nsplit_eff, int64_t* bytes);
int a3c_gemm_f32(const a3c_gemm_desc* d, void* workspace, int64_t workspace_bytes, int* nsplit_eff,
                 void* stream);
int a3c_gemm3_f32(const a3c_gemm_desc* d, void* const* workspaces, const int64_t* workspace_bytes,
                  int* nsplit_eff, void* stream);

/* ----------------------------------------------------------------------------
 * C5  LSTM head (BASELINE config 5; no reference code -- build-defined after TF1
 *     BasicLSTMCell, forget_bias 1.0, and the A3C-LSTM of assets/a3c.png's paper).
 *  a3c_lstm_transpose: w_t [4U][256+U] = w^T, the forward's operand layout (once per
 *    parameter version).
 *  a3c_lstm_step: one cell step for B envs on w_t.  x [B][256] (fc ReLU output), h_src/c_src [B][U]
 *    the previous step's outputs; prev_terms [B] (nullable): state zeroed where the previous
 *    transition was terminal.  Writes h/c [B][U]; hp/cp (the masked inputs it used) and gates
 *    ([B][4U], activated i, j, f, o) are nullable (only the backward needs them).
 *  a3c_lstm_bptt: truncated BPTT over n steps of E envs (b = t*E + e), given dh [n*E][U] =
 *    dL/dh_t from the heads.  dx [n*E][256] = dL/dx_t masked by x > 0 (the fc ReLU: ready for
 *    the fc backward); dw [256+U][4U], db [4U] OVERWRITTEN.  terms [n][E] (transition t
 *    terminal -> no gradient flows from step t+1 into step t's state).
 * -------------------------------------------------------------------------- */
int a3c_lstm_transpose(const float* w, float* w_t, void* stream);
int a3c_lstm_step(const float* w_t, const float* b, const float* x, const float* h_src, const float* c_src,
                  const uint8_t* prev_terms, int64_t B, float* hp, float* cp, float* gates, float* h,
                  float* c, void* stream);
int a3c_lstm_workspace_bytes(int n, int64_t E, int64_t* bytes);
int a3c_lstm_bptt(const float* w, int n, int64_t E, const float* x, const float* hp, const float* cp,
                  const float* gates, const float* c, const uint8_t* terms, const float* dh, float* dx,
                  float* dw, float* db, void* workspace, void* stream);

/* K12  target sync (agent.py:342-344) / theta' <- theta (network.py:96-107). */
int a3c_copy_params(float* dst, const float* src, int64_t n, void* stream);

/* ----------------------------------------------------------------------------
 * Hogwild parameter server across GPUs (main.py:58-66 ps with unlocked RMSProp,
 * SURVEY §8(e) "async"): every GPU owns a byte-range shard of params / ms / mom in
 * its HBM, exported over IPC; workers push clipped gradients straight into every
 * shard with an unlocked elementwise RMSProp over xGMI and pull the parameters back
 * at rollout start (theta' <- theta, network.py:96-107).
 *  a3c_dev_alloc/free: plain hipMalloc'd device memory (IPC-exportable base pointer).
 *  a3c_dev_alloc_kind: the same with kind 0 coarse-grained (= a3c_dev_alloc), 1 fine-grained
 *                      (hipDeviceMallocFinegrained: peer writes coherent at instruction
 *                      granularity, the Hogwild shards' default), 2 uncached; free with a3c_dev_free.
 *  a3c_ipc_handle:     64-byte hipIpcMemHandle of such a base pointer.
 *  a3c_ipc_open/close: map a peer's handle (lazy peer access) into this process.
 *  a3c_rmsprop_range:  TF ApplyRMSProp on n elements (w, ms, mom may live on a peer
 *                      GPU); lr read from lr_dev[0] when lr_dev != NULL.
 * -------------------------------------------------------------------------- */
int a3c_dev_alloc(int64_t bytes, void** out);
int a3c_dev_alloc_kind(int64_t bytes, int kind, void** out);
int a3c_dev_free(void* p);
int a3c_ipc_handle(void* base, void* handle64);
int a3c_ipc_open(const void* handle64, void** out);
int a3c_ipc_close(void* p);
int a3c_rmsprop_range(float* w, float* ms, float* mom, const float* grads, int64_t n, const float* lr_dev,
                      float lr, float rho, float momentum, float eps, void* stream);

/* ----------------------------------------------------------------------------
 * Batched synthetic Atari env (gym/ALE is absent): the Environment / GymEnvironment interface
 * of environment.py:14-106 for E envs on device (dynamics: oracle/synthetic_env.py).
 *  new_game(random=0): environment.py:28-33; random=1: new_random_game :35-40 (mask nullable)
 *  act: GymEnvironment.act :78-96 (simple=1: SimpleGymEnvironment.act :102-106); outputs
 *       reward / terminal / frame index per env (each nullable), state updated in place
 *  screen: Environment.screen :49-53 of every env's current frame -> out + e*out_stride
 * -------------------------------------------------------------------------- */
typedef struct a3c_env a3c_env;
int a3c_env_create(int num_envs, int action_size, int start_lives, int random_start, int action_repeat,
                   int num_frames, uint64_t seed, int env_id_base, a3c_env** out);
/* The game the device envs play (a3c_engine_create_ex, a3c_env_create_ex).
 *  A3C_GAME_SYNTH: the synthetic Atari stand-in above -- rewards, lives and episode ends are
 *    Philox draws that do not depend on the action, which only picks a hashed noise frame.
 *  A3C_GAME_CATCH ("Catch-v0"): a game that can be learned.  A ball falls down an 8-column,
 *    10-row board, one row per step, onto a paddle in the bottom row: actions 0 stay, 1 left,
 *    2 right (any other value: stay), the paddle clamped to the board.  At the landing (row 9)
 *    the reward is +1 with the paddle in the ball's column, else -1, and the episode ends:
 *    every episode lasts 9 steps, the optimal return is +1.  The state is the pool frame index
 *    f = (c*10 + r)*8 + p < 640 (ball column c, ball row r, paddle column p); ep_step = r,
 *    ep_len = 9, lives = 0.  reset: episode += 1, (x0, x1, ..) = philox(episode, id, P_RESET, 0),
 *    c = x0 % 8, p = x1 % 8, r = 0; new_game and new_random_game are the reset (random_start is
 *    ignored: the reset is the random start); a step draws nothing; a step on a landed state
 *    changes nothing and returns reward 0, terminal 1.  Frame f of the pool is rendered, not
 *    hashed: black, the ball's 21 x 20 px cell (rows 21r.., cols 20c..) in (236,236,236), then
 *    the paddle, rows 200..209 x cols 20p..20p+19, in (92,186,92).
 *    Needs num_frames >= 640, action_size 3, start_lives 0; not with frame84 or external_env
 *    (A3C_ERR_INVALID).  a3c_hostenv_* stays the synthetic game. */
#define A3C_GAME_SYNTH 0
#define A3C_GAME_CATCH 1
/* a3c_env_create with the game as an argument; a3c_env_create is game = A3C_GAME_SYNTH. */
int a3c_env_create_ex(int num_envs, int action_size, int start_lives, int random_start, int action_repeat,
                      int num_frames, uint64_t seed, int env_id_base, int game, a3c_env** out);
/* Catch's two rule parameters, visible_rows V in 1..10 and frozen_rows F in 0..8; V = 10,
 * F = 0 is the game above, bit for bit, and "CatchMemory-v0" is V = 1, F = 4.
 *  render: the ball's cell is drawn only in the frames of ball rows r < V; the paddle always is.
 *  step:   in one elementary step the paddle moves only if the row before the step is >= F; the
 *          row always advances.  Landing, reward and terminal are unchanged.
 *  reset:  the same Philox draw; p = x1 % 8, M = 9 - F, lo = max(0, p - M), hi = min(7, p + M),
 *          c = lo + x0 % (hi - lo + 1): the ball falls where the paddle can still reach it
 *          (F <= 2: c = x0 % 8).
 * With F >= V + 3 and action_repeat 1 no 4-frame state in which an action moves the paddle shows
 * the ball: a policy without memory cannot do better than chance, one with memory reaches +1.
 * a3c_env_set_catch_rules records the rules and renders the pool again on `stream`; the envs' states
 * stay as they are, the caller starts new games afterwards.  A3C_ERR_INVALID, before anything
 * touches the device and in this order: V outside 1..10, F outside 0..8, env NULL, an env whose
 * game is not Catch.  An env that never calls it is V = 10, F = 0. */
int a3c_env_set_catch_rules(a3c_env* env, int visible_rows, int frozen_rows, void* stream);
int a3c_env_destroy(a3c_env* env);
int a3c_env_new_game(a3c_env* env, const uint8_t* mask, int random, void* stream);
int a3c_env_act(a3c_env* env, const int32_t* actions, int is_training, int simple, float* rewards,
                uint8_t* terminals, int32_t* frames, void* stream);
int a3c_env_screen(a3c_env* env, uint8_t* out, int64_t out_stride, void* stream);
int a3c_env_buffers(a3c_env* env, uint8_t** pool, int32_t** frame, int32_t** lives, uint32_t** episode,
                    uint32_t** ep_step, float** reward, uint8_t** terminal);

/* ----------------------------------------------------------------------------
 * Batched actor-learner engine: E envs per GPU stepped in lock-step on device
 * (synthetic ALE stand-in, oracle/synthetic_env.py semantics), n-step rollout,
 * backward, per-tensor clip, RMSProp.  One process per GPU; the multi-GPU gradient
 * exchange happens between a3c_engine_rollout_grad and a3c_engine_apply (RCCL from the
 * host, on the same stream).
 * -------------------------------------------------------------------------- */
typedef struct a3c_engine a3c_engine;

typedef struct a3c_engine_config {
  a3c_net_desc net;
  int num_envs;          /* E per GPU                                              */
  int n_step;            /* rollout length n (a3c 5; q: train_frequency 32)          */
  int env_id_base;       /* global id of this GPU's env 0 (rank * E)                 */
  int world_size;        /* GPUs taking part (lr schedule counts their env-steps)    */
  int start_lives;       /* 0 Pong, 5 Breakout, 3 SpaceInvaders                      */
  int random_start;      /* config.py:7 (30)                                          */
  int action_repeat;     /* config.py:50 (1)                                          */
  int num_frames;        /* synthetic frame pool size (HBM resident RGB frames)       */
  int use_graph;         /* 1: capture the rollout / backward into hipGraphs; default 0
                            (eager launches: faster on MI355X)          */
  uint64_t seed;         /* main.py:35 random_seed (123)                             */
  double gamma;          /* config.py:9 discount 0.99                                 */
  float beta;            /* config.py:16 entropy weight 0.01                          */
  float learning_rate;   /* config.py:11 7e-4                                          */
  int64_t max_step;      /* config.py:5 8e7                                           */
  float decay, momentum, epsilon;   /* main.py:64-65: 0.99, 0, 0.1                    */
  float clip_norm;       /* agent.py:319: 40                                          */
  int literal_adv;       /* 1: network.py literal un-stopped advantage gradient       */
  /* q-learning only */
  float ep_start, ep_end;   /* config.py:18-19                                          */
  int q_nstep;        /* q only: 1 = asynchronous n-step Q-learning (Algorithm S2; a3c_nstep_q_target): the
                        target of step i of the rollout is its n-step return, bootstrapped from the target
                        net on s_n alone (double_q: at the slot's own argmax), instead of the one-step TD
                        target of every transition.  0 (default): one-step.  Other values, and 1 with
                        algo a3c, are rejected.  A hyperparameter (not in the checkpoint's state; play does
                        not read it).  python async-rl-tensorflow_amd/main.py --mode engine --algo q
                        --q_nstep true --n_step 5 --env_name Catch-v0.  It takes the 4 bytes that aligned ep_end_t: the size
                        and every other offset of this struct are what they were without it.     */
  int64_t ep_end_t, learn_start;  /* config.py:20-25                                    */
  int64_t target_q_update_step;   /* config.py:10 (4e4)                               */
  double discount;                /* config.py:9                                      */
  int overlap;        /* 1 (a3c, q; not with host envs): rollout k runs on an engine stream while the backward +
                        apply of rollout k-1 run on the caller's stream; rollout k uses the
                        parameters after update k-2 (A3C stale-parameter asynchrony, fixed
                        staleness 1).  0: synchronous rollout -> grad -> apply.          */
  int external_env;   /* 1: the envs are stepped by the host (real ALE / gym workers,
                        SURVEY §8(f)1): a3c_engine_ext_* below feed their RGB frames,
                        rewards and terminals each step; no synthetic env, no frame pool
                        (num_frames ignored).  Synchronous engines only.                 */
  int frame84;        /* 1: measurement mode M2: the pool holds pre-sized 84x84
                        grey frames (the north star's synthetic 84x84x4 states), so the env
                        step's Environment.screen becomes a 7 KB copy into the history ring.
                        0 (default, M1): raw 210x160x3 RGB frames, screen computed on device. */
  int split_exchange; /* 1 (world_size > 1, eager launches): the backward clips the fc / head
                        gradients (99 % of the bytes) before the conv backward and records an
                        event there, so the partitioned-PS exchange of that range runs on a comm
                        stream under the conv backward (a3c_engine_wait_grad_head); only the
                        conv tensors' exchange waits for the whole backward.  Gradients are
                        bit-identical either way.  Default 1.                                 */
  int double_q;       /* q only: double Q-learning (agent.py:176-184) -- the TD target of transition
                        t takes the target net's q of s_{t+1} at the online net's argmax action
                        (the rollout's own q rows, plus one online forward of the bootstrap state
                        s_n) instead of the target net's max.  Default 0.                     */
  float gae_lambda;   /* a3c only: GAE(lambda) (a3c_gae_returns).  The target of the head backward --
                        the policy advantage's minuend and the value target -- is the lambda-return
                        A_t + V(s_t), with the rollout's own V rows.  1 (default): the n-step return
                        of Algorithm S3, the kernels without GAE.  In [0, 1]; != 1 is rejected with
                        algo q and with literal_adv.                                          */
} a3c_engine_config;

void a3c_engine_config_default(a3c_engine_config* cfg);
int a3c_engine_create(const a3c_engine_config* cfg, a3c_engine** out);
/* a3c_engine_create with the game of the device envs, `game` = A3C_GAME_SYNTH or A3C_GAME_CATCH: the
 * same fused rollout / play kernels step it (their Catch instantiations).  a3c_engine_create is
 * game = A3C_GAME_SYNTH.  (An argument and not a field of a3c_engine_config, so that callers built
 * against the struct as it stands stay valid -- as a3c_engine_play_ex's refill.)  A3C_ERR_INVALID
 * for an unknown game, and for Catch with num_frames < 640, action_size != 3, start_lives != 0,
 * frame84 or external_env; nothing is allocated or launched then. */
int a3c_engine_create_ex(const a3c_engine_config* cfg, int game, a3c_engine** out);
/* Options that a3c_engine_config, whose size and layout callers hold, has no room for: a struct that
 * starts with its own size, so later options append and a caller built against a shorter one stays
 * valid (fields past `size` take their defaults).
 *  game:  A3C_GAME_*, as a3c_engine_create_ex's argument.
 *  sarsa: q only.  1 = asynchronous Sarsa (§4 of the A3C paper, beside Algorithm S1): the target of a
 *         transition is r + discount * Q(s', a'; theta^-) at the action a' the behaviour policy takes
 *         in s' -- the rollout's next action, and for the last step the draw the rollout's head would
 *         make in s_n (a3c_boot_action, with the slot's own parameters) -- instead of the maximum
 *         (a3c_sarsa_target).  With cfg.q_nstep = 1: n-step Sarsa, the n-step returns bootstrapped
 *         from Q(s_n, a_n; theta^-).  0 (default): Q-learning, the launches without it.  A
 *         hyperparameter (not in the checkpoint's state; play does not read it).
 *         python async-rl-tensorflow_amd/main.py --mode engine --algo q --sarsa true.
 * a3c_engine_create and a3c_engine_create_ex are a3c_engine_create_opts with the defaults (and the
 * game).  A3C_ERR_INVALID, beside a3c_engine_create_ex's cases: opts NULL or opts->size smaller than
 * the fields read here, sarsa not 0 or 1, sarsa with algo a3c, sarsa with double_q (double Q picks
 * the argmax, Sarsa the taken action); nothing is allocated or launched then. */
typedef struct a3c_engine_opts { int size; int game; int sarsa; } a3c_engine_opts;
void a3c_engine_opts_default(a3c_engine_opts* opts);   /* size = sizeof, game = A3C_GAME_SYNTH, sarsa = 0 */
int a3c_engine_create_opts(const a3c_engine_config* cfg, const a3c_engine_opts* opts, a3c_engine** out);
int a3c_engine_destroy(a3c_engine* eng);
/* The engine's optimizer.  A3C_OPT_RMSPROP (the default: cfg.decay / momentum / epsilon;
 * beta1, beta2 and eps are then checked and otherwise unused) or A3C_OPT_ADAM, TF1 ApplyAdam with the
 * lr of the same schedule: the `mom` buffer holds m, the `ms` buffer v, and the engine keeps the fp64
 * running products beta1^t, beta2^t of its t applied steps on the device -- the schedule forms alpha
 * from them, the apply (a3c_engine_apply_commit: by the nranks of its a3c_engine_apply_shard calls)
 * advances them.  A setter, not an option of a struct: neither a3c_engine_config nor a3c_engine_opts
 * can grow.  Legal whenever no gradient is pending (before or after a3c_engine_reset, between
 * iterations): it re-initialises the two slots (RMSProp: ms = 1, mom = 0; Adam: both 0) and the
 * products (1, 1) on the null stream and waits for them; a3c_engine_reset does the same for the
 * optimizer set.  A3C_ERR_INVALID, before anything touches the device: kind unknown, a beta outside
 * [0, 1), eps <= 0, eng NULL (checked in that order).  A3C_ERR_STATE: a computed gradient not yet applied.
 * Engines that never call it launch what they launched without it.
 * a3c_engine_adam_powers: the two products (1, 1 for RMSProp), after the work on `stream`;
 * a3c_engine_set_adam_powers writes them (resume from a checkpoint; Adam engines only). */
#define A3C_OPT_RMSPROP 0
#define A3C_OPT_ADAM 1
int a3c_engine_set_optimizer(a3c_engine* eng, int kind, double beta1, double beta2, double eps);
int a3c_engine_adam_powers(a3c_engine* eng, double* beta1_power, double* beta2_power, void* stream);
int a3c_engine_set_adam_powers(a3c_engine* eng, double beta1_power, double beta2_power, void* stream);
/* Catch's rule parameters for the engine's device envs (a3c_env_set_catch_rules has the rules; DESIGN
 * 4k).  A setter as the optimizer's, for the same reason.  It only records the rules: until the next
 * a3c_engine_reset -- which renders the pool with them, resets the envs and zeroes the play context --
 * rollout, iterate, play and every other entry that needs a reset return A3C_ERR_STATE.
 * A3C_ERR_INVALID, before anything touches the device and in this order: visible_rows outside 1..10,
 * frozen_rows outside 0..8, eng NULL, an engine whose game is not Catch.  A3C_ERR_STATE: a computed
 * gradient not yet applied.  A hyperparameter: not in the checkpoint's state.  An engine that never
 * calls it launches what it launched without it, and its state blob is byte for byte the same.
 * python async-rl-tensorflow_amd/main.py --mode engine --lstm true --env_name CatchMemory-v0 */
int a3c_engine_set_catch_rules(a3c_engine* eng, int visible_rows, int frozen_rows);
/* first_screen: what a Catch engine's training rollouts write into the history at a
 * terminal.  on = 0, the default, is the reference worker loop (agent.py:59-67): the landing's screen
 * is added and the new game started at agent.py:66-67 shows nothing until its first act, so the first
 * frame of an episode that training sees is its row 1.  on = 1: at a terminal of env e in rollout step
 * t the screen written to ring slot (tau + t + 1) % R is that of the new game's first state -- the rule
 * Agent.play follows at agent.py:366-367 -- and the landing's screen, whose only reader is a next state
 * that every target multiplies by (1 - terminal), is not written.  One slot, not four: the three older
 * planes belong to the states before.  Reward, terminal, env state, action draw, the LSTM carry and
 * the target cadence are unchanged; the per-step frame indices the engine records are those of the
 * screens written.  Play is not affected.  A setter, as the two above: it needs no reset and takes
 * effect at the next terminal; it drops captured graphs.  A3C_ERR_INVALID, before anything touches the
 * device and in this order: on not 0 or 1, eng NULL, an engine whose game is not Catch (the external-
 * env engine included).  A3C_ERR_STATE: a computed gradient not yet applied.  A hyperparameter: not in
 * the checkpoint's state.  An engine that never calls it launches what it launched without it.
 * python async-rl-tensorflow_amd/main.py --mode engine --lstm true --env_name CatchMemory-v0 --first_screen true */
int a3c_engine_set_first_screen(a3c_engine* eng, int on);
/* q_lambda: lambda-return targets for a Q engine (a3c_lambda_q_target), the knob between
 * its one-step targets (lambda = 0) and the n-step returns of cfg.q_nstep (lambda = 1).  on = 0, the
 * default: every launch is what it is without this call.  on = 1: the gradient's launches are those
 * of the one-step rule -- the target network on the n*E rows of s_1 .. s_n, and for double Q and Sarsa
 * the slot's own forward of s_n -- with a3c_lambda_q_target in the target kernel's place: cfg.double_q
 * passes the rollout's own rows of s_1 .. s_n as q_sel, a Sarsa engine (a3c_engine_opts.sarsa) draws
 * a_n as it does without lambda (a3c_boot_action's rule, inside the target kernel;
 * a3c_engine_slot_boot_actions reads it) and passes the rollout's actions.  Sync, overlap,
 * graph, host-env and Hogwild iterations share that block.  A setter, as the three above: no reset,
 * the next gradient follows it; it drops captured graphs.  A3C_ERR_INVALID, before anything touches the
 * device and in this order: on not 0 or 1, lambda outside [0, 1] or NaN, eng NULL, an engine of algo
 * a3c (it has cfg.gae_lambda), an engine with cfg.q_nstep = 1 (that engine is lambda = 1 with the
 * target forward of s_n alone).  A3C_ERR_STATE: a computed gradient not yet applied.  A hyperparameter:
 * not in the checkpoint's state (a resumed run gives it again), and play does not read it.
 * python async-rl-tensorflow_amd/main.py --mode engine --algo q --q_lambda 0.8 --env_name Catch-v0 */
int a3c_engine_set_q_lambda(a3c_engine* eng, int on, double lambda);
/* fill the frame pool, reset the envs (new_random_game, environment.py:35-40), fill each
 * history with 4 copies of the first screen (agent.py:37-38) and initialise params
 * from host memory (nullable -> keep), rms slot = 1, mom = 0 (Adam: m = v = 0, products = 1). */
int a3c_engine_reset(a3c_engine* eng, const float* host_params, void* stream);
/* n rollout steps + bootstrap + loss + backward + per-tensor clip -> grads */
int a3c_engine_rollout_grad(a3c_engine* eng, void* stream);
/* RMSProp apply of grads (lr from the device worker step, agent.py:393-395) and advance counters.
 * overlap: a no-op until the pipeline holds a gradient (first call after reset). */
int a3c_engine_apply(a3c_engine* eng, void* stream);
/* a3c_engine_rollout_grad + a3c_engine_apply as one enqueue (single GPU, device envs only: no
 * gradient exchange between them), the apply captured into the same hipGraphs.  Same results
 * bit for bit; a3c_engine_grad_ready reports as after a3c_engine_rollout_grad, and a following
 * a3c_engine_apply is a no-op (the gradient is applied already). */
int a3c_engine_iterate(a3c_engine* eng, void* stream);
/* 1 if the last a3c_engine_rollout_grad produced a gradient (always, unless overlap and it
 * was the first call after reset) -- exchange / apply only then. */
int a3c_engine_grad_ready(a3c_engine* eng);
/* advance tau / global step as a3c_engine_apply does, without touching the parameters
 * (Hogwild: the gradient went to the shared shards instead) */
int a3c_engine_advance(a3c_engine* eng, void* stream);

/* Partitioned parameter server: the multi-GPU form of the reference's PS (main.py:58-66), where
 * every worker's per-worker-clipped gradient (agent.py:316-319) is its own RMSProp step on the
 * shared variables (agent.py:321), applied in arrival order.  Rank r of W owns the flat range
 * [lo, lo + n) of params / ms / mom.  Per iteration, after a3c_engine_rollout_grad (world_size > 1:
 * grads hold this worker's clipped gradient):
 *   host: all-to-all of grads -> grads_by_rank [W][n] (rank q's gradient of this range);
 *   a3c_engine_apply_shard: the W RMSProp steps of the range, in rank order q = 0..W-1 (lr from the
 *     device schedule), new weights -> w_out [n];
 *   host: all-gather of every rank's w_out -> the full parameter vector;
 *   a3c_engine_apply_commit: params <- params_src (nullable: already there), overlap snapshot,
 *     target sync (q), counters -- the rest of a3c_engine_apply.
 * Both are no-ops when no gradient is pending (overlap pipeline filling).  With A3C_OPT_ADAM the W
 * steps are Adam steps, step q with the alpha of the step count advanced q + 1 times (at most 64
 * ranks per call), and the commit advances the count by W; a commit of a pending gradient
 * with no a3c_engine_apply_shard before it -- the Hogwild push, which applies RMSProp in its shards --
 * returns A3C_ERR_STATE on an Adam engine. */
int a3c_engine_apply_shard(a3c_engine* eng, const float* grads_by_rank, int nranks, int64_t lo, int64_t n,
                           float* w_out, void* stream);
int a3c_engine_apply_commit(a3c_engine* eng, const float* params_src, void* stream);
/* Split exchange (cfg.split_exchange, world_size > 1): the backward clips grads[cut:] (fc + heads,
 * 99 % of the bytes) before the conv backward and marks it; the exchange of that range (all-to-all,
 * a3c_engine_apply_shard of its part of each owned range, all-gather) then runs on a comm stream
 * under the conv backward, and only grads[:cut] (the conv tensors, ~50 KB) wait for the whole
 * backward (src/distributed.py PartitionedPS).  The same apply_shard / apply_commit calls, on the
 * sub-ranges; results bit-identical to the one-phase exchange.
 *   a3c_engine_exchange_split: *cut (0: the engine does not split);
 *   a3c_engine_wait_grad_head: `stream` waits for grads[cut:] of the last rollout_grad. */
int a3c_engine_exchange_split(a3c_engine* eng, int64_t* cut);
int a3c_engine_wait_grad_head(a3c_engine* eng, void* stream);

/* ----------------------------------------------------------------------------
 * Summaries: the aggregates train_with_summary logs every test_step
 * (agent.py:69-139), kept on device over every env of this GPU.
 *  stats_accumulate: adds the rollout whose gradient the last rollout_grad / iterate computed
 *                    (enqueue after it on the same stream; a no-op while no gradient is ready).
 *  stats_read:       waits for `stream`, copies the A3C_STATS_N doubles; reset = 1 starts a new
 *                    interval (each env's running episode reward carries on).
 * out: [0] sum of act() rewards (unclipped, every env-step; agent.py:101), [1] sum, [2] max,
 *      [3] min of finished episodes' rewards (the terminal step's reward excluded, agent.py:91-98;
 *      max -inf / min +inf when none), [4] games, [5] sum over updates of the per-sample loss
 *      (q: the MSE, agent.py:196; a3c: total / (n*E)), [6] sum over updates of the batch mean
 *      Q(s) (q: over actions, agent.py:200; a3c: V(s)), [7] updates, [8] env-steps, [9..11] sums
 *      of per-sample policy loss, value loss, entropy (a3c). */
#define A3C_STATS_N 16
int a3c_engine_stats_accumulate(a3c_engine* eng, void* stream);
int a3c_engine_stats_read(a3c_engine* eng, double* out, int reset, void* stream);

/* ----------------------------------------------------------------------------
 * Checkpoint / resume.  Replaces the Supervisor's Saver (main.py:74-90, which saves
 * the prediction weights + `step` every 600 s, agent.py:29) and its restore at managed_session.
 *  set_step:    resume from parameters + step only (what the reference's Saver keeps; the caller
 *               writes params / target / RMSProp slots through a3c_engine_get_buffers): the global
 *               step T (agent.py:165) and the workers' loop counter (agent.py:34,46,55: the lr and
 *               epsilon schedules run on it) restart at the given values.  After a3c_engine_reset.
 *  state_*:     the whole engine state -- parameters, target, RMSProp slots, counters, env state,
 *               frame ring, LSTM carry and, in overlap mode, the rollout in flight -- so a restored
 *               engine of the same configuration continues the run bit for bit.  state_save / load
 *               wait for the engine's streams; load needs a3c_engine_reset first (frame pool).
 *               Engines with host-stepped envs (external_env) refuse: the host envs cannot be
 *               snapshotted, they resume with set_step. */
int a3c_engine_set_step(a3c_engine* eng, int64_t global_step, int64_t worker_step, void* stream);
int a3c_engine_state_bytes(a3c_engine* eng, int64_t* bytes);
int a3c_engine_state_save(a3c_engine* eng, void* host, int64_t bytes, void* stream);
int a3c_engine_state_load(a3c_engine* eng, const void* host, int64_t bytes, void* stream);

/* ----------------------------------------------------------------------------
 * External (host-stepped) environments, cfg.external_env = 1.  Per rollout:
 *   for t in 0..n-1:  a3c_engine_ext_act -> sync -> host steps every env with its action
 *                     (GymEnvironment.act, environment.py:78-96; new_random_game on a
 *                     terminal, agent.py:66-67) -> a3c_engine_ext_observe
 *   a3c_engine_rollout_grad (bootstrap + loss + backward) -> [exchange] -> a3c_engine_apply.
 * Host pointers should be pinned (hipHostMalloc / torch pin_memory) for async copies; device
 * pointers work too (hipMemcpyDefault).
 *  ext_begin:   rgb [E][210][160][3] u8 first frames of each env (after new_random_game):
 *               every history slot <- its screen (agent.py:33-38), tau / step counters reset.
 *  ext_act:     predict of step t (agent.py:141-151 / network.py:65-72 draw); actions [E] i32.
 *  ext_observe: post-act frames rgb, rewards [E] f32 (clipped here, agent.py:154), terminals
 *               [E] u8 -> Environment.screen (environment.py:49-53) + History.add.
 * -------------------------------------------------------------------------- */
int a3c_engine_ext_begin(a3c_engine* eng, const uint8_t* rgb, void* stream);
int a3c_engine_ext_act(a3c_engine* eng, int32_t* actions, void* stream);
int a3c_engine_ext_observe(a3c_engine* eng, const uint8_t* rgb, const float* rewards, const uint8_t* terminals,
                           void* stream);
/* part of observe (same step, before it): frames of envs [env_lo, env_hi) only, so the copy of
 * one range overlaps the host stepping of the next; observe is then called with rgb = NULL, which
 * fails with A3C_ERR_STATE unless the step's ranges covered every env in [0, E) */
int a3c_engine_ext_upload(a3c_engine* eng, const uint8_t* rgb, int env_lo, int env_hi, void* stream);

/* Host-side batched synthetic env (the device env's emulator, bit-identical dynamics, stepped by
 * `threads` CPU threads): raw RGB frames into caller host buffers -- a stand-in for real ALE
 * worker processes when driving / measuring the external-env path.  No GPU work.
 *  begin: new_random_game of every env; first frames -> rgb [E][210][160][3] u8
 *  step:  GymEnvironment.act (environment.py:78-96) of every env, post-act frames -> rgb,
 *         rewards [E] f32 (unclipped), terminals [E] u8; new_random_game where terminal
 *         (agent.py:66-67). */
typedef struct a3c_hostenv a3c_hostenv;
int a3c_hostenv_create(int num_envs, int action_size, int start_lives, int random_start, int action_repeat,
                       int num_frames, uint64_t seed, int env_id_base, int threads, a3c_hostenv** out);
int a3c_hostenv_destroy(a3c_hostenv* env);
int a3c_hostenv_begin(a3c_hostenv* env, uint8_t* rgb);
int a3c_hostenv_step(a3c_hostenv* env, const int32_t* actions, int is_training, uint8_t* rgb, float* rewards,
                     uint8_t* terminals);
/* step of envs [env_lo, env_hi) only (buffers stay full-size, indexed by env) */
int a3c_hostenv_step_range(a3c_hostenv* env, const int32_t* actions, int is_training, uint8_t* rgb,
                           float* rewards, uint8_t* terminals, int env_lo, int env_hi);

/* device pointers owned by the engine (valid until destroy) */
typedef struct a3c_engine_buffers {
  float* params; float* target_params; float* ms; float* mom; float* grads;
  int64_t n_params;
  uint8_t* frame_ring;     /* [E][R][84*84] u8                                */
  int ring_slots;
  int64_t* tau;            /* device: current frame index tau; tau[2] = the workers' base step
                              (worker step of rollout step t = tau[2] + tau - 3 + t)  */
  int64_t* global_step;    /* device: env-steps taken by all GPUs (= tau + 1)  */
  int32_t* actions;        /* [n][E]                                           */
  float* rewards;          /* [n][E]                                           */
  uint8_t* terminals;      /* [n][E]                                           */
  float* z;                /* [(n+1)][E][zs] (row n = bootstrap forward)       */
  float* returns;          /* [n][E] R or TD target                            */
  float* loss;             /* [4]                                              */
  float* sumsq;            /* [n_tensors] pre-clip squared norms               */
  float* act_l1; float* act_l2; float* act_l3;  /* [n*E][...]                  */
  uint8_t* frame_pool;     /* [num_frames][210][160][3]                        */
  int32_t* env_frame; int32_t* env_lives; uint32_t* env_episode; uint32_t* env_step;
  uint32_t* env_len;
  int zs; int n_tensors; int64_t offsets[A3C_MAX_TENSORS]; int64_t sizes[A3C_MAX_TENSORS];
  float* sched;            /* device: [0] learning rate of the last gradient (agent.py:393-395) */
  /* LSTM head (net.lstm_units > 0), per rollout step t: h_t, c_t [n][E][U]; the masked state
   * inputs hp, cp [n][E][U]; activated gates [n][E][4U].  NULL without the LSTM head. */
  float* lstm_h; float* lstm_c; float* lstm_hp; float* lstm_cp; float* lstm_gates;
  int lstm_units;
  /* nature trunk (net.trunk = A3C_TRUNK_NATURE): act_l1 [n*E][20][20][32], act_l2 [n*E][9][9][64],
   * act_l3 [n*E][3136] (the conv3 output, (h,w,c)-flattened), act_l4 [n*E][512] (fc out);
   * NIPS: act_l4 NULL */
  float* act_l4;
  int trunk;
} a3c_engine_buffers;
int a3c_engine_get_buffers(a3c_engine* eng, a3c_engine_buffers* out);
/* same, with the rollout buffers (actions .. act_l3) of slot 0 or 1 (overlap: rollout k
 * writes slot k & 1); get_buffers == slot 0 */
int a3c_engine_slot_buffers(a3c_engine* eng, int slot, a3c_engine_buffers* out);
/* Sarsa engines (a3c_engine_opts.sarsa): *out = the slot's boot_actions [E] i32, the action drawn for
 * the bootstrap state s_n by the slot's last gradient (a3c_boot_action's rule; transient: written and
 * read inside one gradient, not part of the saved state).  A3C_ERR_INVALID without sarsa. */
int a3c_engine_slot_boot_actions(a3c_engine* eng, int slot, int32_t** out);

/* ----------------------------------------------------------------------------
 * Evaluation: Agent.play (agent.py:351-391) on the engine, without learning.  The engine's E envs
 * play n_episode episodes in waves of E: episode idx = w * E + e is played by env e in wave w
 * (ceil(n_episode / E) waves, the last one possibly partial).  A forward-only rollout with a
 * context of its own (env state, a frame ring of HIST + 1 slots, one step's activations, LSTM
 * state): no training buffer, counter or env is written, in overlap mode too, and the frame pool
 * is only read.  The context is allocated and zeroed by the first call, persists across calls and
 * is zeroed again by a3c_engine_reset.
 *  parameters: the live ones as they stand on `stream` at the call (agent.py:351: the network
 *              being trained), prepared once per call.
 *  wave start: new_random_game of the wave's envs (agent.py:363; the emulator goes on where the
 *              env's last episode stopped, it resets only at lives == 0), the first screen into
 *              the HIST newest ring slots (agent.py:366-367), LSTM state zeroed, and the play tau
 *              of wave w set to (HIST-1) + w * (n_step + HIST) on every call.
 *  step:       forward, action draw on the (tau, env id) Philox counter the rollout uses
 *              (agent.py:371), act with is_training = false (agent.py:373: a lost life is no
 *              terminal and costs no -1), the new screen into the ring (agent.py:375), return +=
 *              the raw reward, the terminal step's included (agent.py:377), length += 1.  A
 *              terminal ends the env's episode (agent.py:378-379); no new game follows.
 *  frozen:     an env that is done, or has no episode in the wave, is frozen: nothing of it
 *              advances (emulator, ring, LSTM state, trace entries).  A wave ends after n_step
 *              steps, or once the host -- reading the active count every poll_every steps -- sees
 *              none active; results do not depend on poll_every.
 *  draw:       q engines: epsilon-greedy with eps = test_ep for every env, or with the engine's
 *              per-env final epsilon (main.py:68, the reference's test_ep = self.ep_end) when
 *              test_ep < 0.  a3c engines: the categorical draw (network.py:72) with greedy = 0;
 *              with greedy = 1 epsilon-greedy on the logits with eps = max(test_ep, 0).
 *              test_ep = 0 means greedy.  (The reference's `test_ep or schedule`, agent.py:371 ->
 *              :142-144, falls back to the training schedule for test_ep = 0; here 0 is honoured.)
 *  outputs:    host arrays returns / lengths / terminated [n_episode] (terminated: the episode hit
 *              a terminal before the n_step cap).  The reference's best episode (agent.py:381-383)
 *              is the first idx, in idx order, whose return is > the best so far, from (0, 0).
 *              trace_actions [waves][n_step][E] i32 and trace_z [waves][n_step][E][zs] f32:
 *              optional device buffers written by the steps' own kernels; entries of frozen envs
 *              and of steps a wave did not run are left untouched.
 * Synchronous: `stream` is idle when the call returns.  A3C_ERR_INVALID for engines with
 * host-stepped envs and for n_episode, n_step or poll_every < 1; A3C_ERR_STATE before
 * a3c_engine_reset. */
typedef struct a3c_play_config {
  int n_episode;     /* agent.py:351 n_episode (100)                                     */
  int n_step;        /* agent.py:351 n_step (10000): the cap on an episode's env steps    */
  int greedy;        /* a3c engines: 1 = argmax / epsilon-greedy on the logits (0)         */
  float test_ep;     /* agent.py:351 test_ep; < 0: the per-env final epsilon (-1)          */
  int poll_every;    /* steps between the host's reads of the active count (64)            */
} a3c_play_config;
void a3c_play_config_default(a3c_play_config* cfg);
int a3c_engine_play(a3c_engine* eng, const a3c_play_config* cfg, float* returns, int32_t* lengths,
                    uint8_t* terminated, int32_t* trace_actions, float* trace_z, void* stream);
/* Play with refill (continuous batched evaluation): a3c_engine_play_ex(.., refill = 1, ..).  refill
 * = 0 is a3c_engine_play, bit for bit; other values give A3C_ERR_INVALID.  (The mode is an argument
 * and not a field of a3c_play_config, so that callers built against the five-field struct stay
 * valid.)  In a wave an env whose episode ended idles until the wave's slowest env is done; here
 * it takes the next episode at once, as the reference's one emulator plays its episodes back to
 * back.  Everything not stated below (parameters, step, draw rules, frozen envs, rejections) is as
 * in waves mode.
 *  start:   one run per call, no waves.  tau = HIST-1; episodes idx = 0 .. min(E, n_episode)-1 start
 *           on envs e = idx exactly as a wave does; the other envs are idle (frozen).
 *  end of an episode on env e: at a terminal, or when the episode's own length reaches n_step --
 *           then terminated = 0 and lives > 0, so the emulator goes on, as after a capped wave
 *           episode.  Its return, length and terminated flag go to per-episode device arrays.
 *  refill:  in the same step, behind the bookkeeping.  The envs that ended in this step take the
 *           next unassigned episode indices in env-id order (each env counts the envs in front of
 *           it that ended: exact whatever the order, no atomics).  An
 *           env that gets idx < n_episode: new_random_game (agent.py:363), the new game's first
 *           screen into the HIST newest ring slots of the next step, (tau+1-3 .. tau+1) mod R, over
 *           the post-terminal screen the step has just written (agent.py:366-367), return and length
 *           zeroed, LSTM h / c zeroed in the copy the next step reads, frozen flag of the next step
 *           cleared.  An env that gets none is frozen for good.  Both parity copies of the env state
 *           stay equal.
 *  draw:    the (tau, env id) Philox counter; tau advances by 1 per run step without gaps, so no two
 *           (step, env) share a counter.
 *  end:     once the host -- reading the device count of unfinished episodes every poll_every
 *           steps -- sees 0, and after ceil(n_episode / E) * n_step steps at the latest (under
 *           in-order list scheduling episode k has started by floor(k / E) * n_step).  Results do
 *           not depend on poll_every.  A3C_ERR_INVALID if that bound exceeds 2^31 - 1.
 *  traces:  the buffers keep the waves-mode size, read as [waves * n_step][E] (x zs) indexed by run
 *           step; entries of idle envs and of steps not run are left untouched.
 * a3c_engine_play_schedule: the last play call's schedule -- for episode idx < n (n <= its
 * n_episode) the env that played it and the tau of its first step (lengths[idx] gives the rest);
 * waves mode reports idx % E and the wave's start tau.  *steps: the run steps in which any env was
 * live (waves mode: summed over the waves).  Any output pointer may be NULL. */
int a3c_engine_play_ex(a3c_engine* eng, const a3c_play_config* cfg, int refill, float* returns, int32_t* lengths,
                       uint8_t* terminated, int32_t* trace_actions, float* trace_z, void* stream);
int a3c_engine_play_schedule(a3c_engine* eng, int32_t* episode_env, int64_t* episode_tau0, int n, int64_t* steps);
/* device pointers of the play context (tests; allocates it like the first a3c_engine_play).  The
 * env fields are [2][E] with both parity copies equal; lstm_h / lstm_c [2][E][U], NULL without the
 * LSTM head: the current state is copy (steps the last wave ran) & 1.  episode_idx [E] and sched
 * (the next unassigned idx in two copies by step parity, episodes not finished, steps with a live
 * env) belong to refill runs. */
typedef struct a3c_play_buffers {
  uint8_t* frame_ring;     /* [E][ring_slots][84*84] u8                        */
  int ring_slots;
  int64_t* tau;            /* device: the play tau                             */
  int32_t* env_frame; int32_t* env_lives; uint32_t* env_episode; uint32_t* env_step; uint32_t* env_len;
  float* returns; int32_t* lengths; uint8_t* terminated;   /* [E]: the last wave's bookkeeping */
  uint8_t* frozen;         /* [2][E]                                           */
  float* lstm_h; float* lstm_c;
  int32_t* episode_idx;    /* [E] refill runs: the episode env e plays / played last */
  int32_t* sched;          /* [4] refill runs: next idx x 2, unfinished, live steps  */
} a3c_play_buffers;
int a3c_engine_play_buffers(a3c_engine* eng, a3c_play_buffers* out);

/* profiling hook: average device time (ms) of `iters` back-to-back launches of one engine
 * kernel on its live buffers, bracketed by HIP events on `stream` (idempotent: each
 * relaunch recomputes the same outputs). */
#define A3C_KER_CONV12_FWD 0   /* conv1+conv2 forward, B = E (saves conv1 out)          */
#define A3C_KER_FC_FWD 1       /* fc 2592->256 forward GEMM (+split-K reduce), B = E     */
#define A3C_KER_ENV_STEP 2     /* Environment.screen of the post-act frames into the ring */
#define A3C_KER_CONV_BWD 3     /* fused conv backward over B = n*E                       */
#define A3C_KER_HEAD_SCREEN 4  /* fused head + action draw + Environment.screen, B = E    */
#define A3C_KER_HEAD_SCREEN_CONV12 5  /* ... + conv1+conv2 of the next states (overlap mode) */
#define A3C_KER_FC_PART 6      /* fc as K-slice partials (overlap mode; the head folds them)  */
/* nature trunk engines (nature.hip k_nat_gemm passes): forward over E states of the live
 * parameters, backward passes over the n*E samples of the last back-propagated rollout */
/* The release build runs the three forward convolutions of a state as ONE launch (the per-state
 * kernel k_nat_conv23, nature.hip) under A3C_KER_NAT_C2F; A3C_KER_NAT_C1F and _C3F then have no
 * launch of their own and a3c_engine_time_kernel returns A3C_ERR_INVALID for them (likewise
 * _C2X in builds that fuse the two dX passes under _C3X). */
#define A3C_KER_NAT_C1F 7      /* conv1 8x8/4 4->32 forward (u8 ring -> l1), B = E         */
#define A3C_KER_NAT_C2F 8      /* conv2 4x4/2 32->64 forward (release: conv1+conv2+conv3)  */
#define A3C_KER_NAT_C3F 9      /* conv3 3x3/1 64->64 forward                               */
#define A3C_KER_NAT_FCF 10     /* fc 3136->512 forward (split-K GEMM + bias/ReLU fold)      */
#define A3C_KER_NAT_C3W 11     /* conv3 weight gradient (slabs), B = n*E                  */
#define A3C_KER_NAT_C3X 12     /* conv3 input gradient dl2                                 */
#define A3C_KER_NAT_C2W 13     /* conv2 weight gradient                                    */
#define A3C_KER_NAT_C2X 14     /* conv2 input gradient dl1 (4 stride-parity classes)       */
#define A3C_KER_NAT_C1W 15     /* conv1 weight gradient from the u8 planes                 */
/* Live launch spans, recorded by the kernels themselves inside the engine's graphs (which 0:
 * k_conv_bwd, 1: k_head_screen_conv12): per launch, last workgroup end - first workgroup start
 * (s_memrealtime).  reset = 1 clears the records (before a timed region); otherwise returns the
 * average and max span in microseconds and the number of launches recorded (at most 1024). */
int a3c_engine_span_stats(a3c_engine* eng, int which, int reset, double* avg_us, double* max_us,
                          int64_t* launches);
/* The same records of k_head_screen_conv12 (which = 1) split by rollout step: avg_us[t] is the
 * average live span of the launch that runs step t's head (t = 0..n-1; the last one also runs the
 * bootstrap state's conv1+conv2), launches[t] how many were recorded.  Call synchronised, after a
 * timed region with no a3c_engine_set_step/reset since the records were cleared. */
int a3c_engine_span_steps(a3c_engine* eng, double* avg_us, int64_t* launches);
/* The raw records behind both (measurement): out[2 r], out[2 r + 1] = first workgroup start and
 * last workgroup end (s_memrealtime ticks, 100 MHz; 0 = not recorded) of record r < 1024 of
 * `which`, and the live tau counter (records are keyed by tau, see a3c_engine_span_steps). */
int a3c_engine_span_raw(a3c_engine* eng, int which, unsigned long long* out, int64_t* tau_now);
int a3c_engine_time_kernel(a3c_engine* eng, int kernel, int iters, void* stream, float* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* A3C_HIP_H */
