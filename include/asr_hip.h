/*
 * libasr_hip.so -- C ABI of the MI355X (gfx950) hot path of the hybrid
 * CTC/attention ASR training step.
 *
 * Plain pointers and sizes only: no torch / C++ types cross this boundary.
 * All device pointers are HIP device memory owned by the caller; the library
 * never allocates, frees or synchronises inside an entry point (graph-capture
 * safe).  Every entry point is stream-ordered on `stream` (a hipStream_t
 * passed as void*), re-entrant, and returns ASR_OK (0) or a negative error
 * code; asr_last_error() gives the text (thread-local).
 *
 * Reference interfaces replaced (paths into carolinebear/pytorch_end2end_speech_recognition):
 *   CTC           warpctc_pytorch.gpu_ctc / cpu_ctc as bound by
 *                 models/pytorch_v3/ctc/ctc.py:30-66 (my_warpctc)
 *   LSTM layer    torch.nn.LSTM(bidirectional) + pack/pad in
 *                 models/pytorch_v3/encoders/rnn.py:166-172,218-224,343-390
 *   LinearND      models/pytorch_v3/linear.py:15-47 (and every nn.Linear GEMM)
 *   attention     AttentionMechanism.forward (location) in
 *                 models/pytorch_v3/attention/attention_layer.py:123-251
 *   LSTMCell      models/pytorch_v3/attention/rnn_decoder.py:63-113
 *   optimizer     torch.optim.Adam / SGD + clip_grad_norm in
 *                 models/pytorch_v3/base.py:141-213, utils/training/training_loop.py:42-51
 *   best path     GreedyDecoder in models/pytorch_v3/ctc/decoders/greedy_decoder.py:19-47
 */
#ifndef ASR_HIP_H_
#define ASR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_OK 0
#define ASR_ERR_ARG (-1)      /* bad pointer / size / shape argument */
#define ASR_ERR_WORKSPACE (-2) /* workspace too small */
#define ASR_ERR_HIP (-3)      /* HIP runtime error (launch / memset) */
#define ASR_ERR_UNSUPPORTED (-4)

#define ASR_DT_F32 0
#define ASR_DT_BF16 1

/* ---------------------------------------------------------------- info */
const char* asr_version(void);
const char* asr_last_error(void);
/* 1 when the current device is a gfx950 (the only code-object target of the
 * library), 0 for another device, -1 when no device can be queried. */
int asr_arch_is_gfx950(void);

/* A HIP stream restricted to CUs [cu_begin, cu_begin + cu_count) of the
 * current device (hipExtStreamCreateWithCUMask).  The weight-gradient GEMMs
 * of encoder layer l run on it beside the persistent backward recurrence of
 * layer l-1, which keeps the remaining CUs to itself. */
int asr_stream_create_cu_masked(int cu_begin, int cu_count, void** stream_out);
int asr_stream_destroy(void* stream);

/* ----------------------------------------------------------------- CTC
 * Replaces warpctc_pytorch.gpu_ctc(acts, grads, labels, label_lens,
 * act_lens, minibatch, costs) (models/pytorch_v3/ctc/ctc.py:35-45).
 *
 * acts: unnormalised f32 activations, element (t, b, v) at
 *   acts[t*stride_t + b*stride_b + v]  -- time-major [T,B,V] as warp-ctc
 *   (stride_t = B*V, stride_b = V) or batch-major [B,T,V] (stride_t = V,
 *   stride_b = T*V) without a transpose copy.
 * labels_flat: int32 [sum(label_lens)], device, values in [0,V) != blank.
 * label_lens, act_lens: int32 [B], device.  max_label_len >= max(label_lens).
 * Softmax is applied inside; blank index `blank` (reference: 0).
 * costs: f32 [B] = -log P(y_b|x_b) (0 if infeasible and zero_infinity, +inf
 *   otherwise).  loss_out (nullable): f32 [1] = loss_scale * sum_b costs[b].
 * Gradient (w.r.t. the unnormalised activations, zero for t >= act_lens[b],
 *   zero for infeasible utterances) is produced by asr_ctc_backward from the
 *   state kept in `workspace` (so it is written exactly once, already scaled),
 *   scaled by scale * (*grad_scale) (grad_scale: device f32 scalar, e.g. the
 *   upstream dLoss; NULL means 1.0).
 */
size_t asr_ctc_workspace_bytes(int T, int B, int V, int max_label_len);
int asr_ctc_forward(const float* acts, long long stride_t, long long stride_b, int T, int B,
                    int V, const int32_t* labels_flat, const int32_t* label_lens,
                    const int32_t* act_lens, int max_label_len, int blank, int zero_infinity,
                    float* costs, float* loss_out, float loss_scale, void* workspace,
                    size_t ws_bytes, void* stream);
/* asr_ctc_forward with the per-frame log-sum-exp already formed by the output
 * layer's GEMM (asr_gemm_lse_ws): lse_part holds, for every frame row b*T + t
 * and 64-class slab q < nslab = ceil(V / 64), the pair (max, sum exp(x - max))
 * at lse_part[2 (q B T + b T + t)].  The activations are then read only at
 * the label columns; costs, loss and the workspace state for asr_ctc_backward
 * are those of asr_ctc_forward. */
int asr_ctc_forward_lse(const float* acts, long long stride_t, long long stride_b, int T, int B,
                        int V, const float* lse_part, int nslab, const int32_t* labels_flat,
                        const int32_t* label_lens, const int32_t* act_lens, int max_label_len,
                        int blank, int zero_infinity, float* costs, float* loss_out,
                        float loss_scale, void* workspace, size_t ws_bytes, void* stream);
int asr_ctc_backward(const float* acts, long long stride_t, long long stride_b, int T, int B,
                     int V, const int32_t* labels_flat, const int32_t* label_lens,
                     const int32_t* act_lens, int max_label_len, int blank,
                     const float* grad_scale, float scale, float* grads, long long gstride_t,
                     long long gstride_b, const void* workspace, size_t ws_bytes, void* stream);
/* asr_ctc_backward writing the gradient as bf16 rows of gld columns (gld >= V,
 * gld % 8 == 0, 16-B aligned rows, strides in elements), columns [V, gld)
 * zero: the zero-padded dY operand of the output layer's staged bf16 GEMMs
 * (the fused CTC head, native_ops.LinearCTCFn; no f32 gradient pass). */
int asr_ctc_backward_bf16(const float* acts, long long stride_t, long long stride_b, int T, int B,
                          int V, const int32_t* labels_flat, const int32_t* label_lens,
                          const int32_t* act_lens, int max_label_len, int blank,
                          const float* grad_scale, float scale, uint16_t* grads,
                          long long gstride_t, long long gstride_b, int gld,
                          const void* workspace, size_t ws_bytes, void* stream);
/* asr_ctc_backward_bf16 that also ADDS the f32 column sums of the gradient,
 * formed before the bf16 rounding, into dbias [V] (the output layer's bias
 * gradient of the fused CTC head: the reference's LinearND bias gradient,
 * linear.py:32-47, summed from dY = ctc.py:30-52's gradient).  Deterministic
 * (fixed-order per-block partials); bias_ws holds
 * asr_ctc_bias_workspace_bytes(T, B, V, gld) bytes.  Supported where
 * asr_ctc_bias_supported(V, gld, max_label_len) returns 1 (gld <= 16384, and
 * for V > 256 the class table beside the lattice-state arrays within a
 * work-group's 64 KiB of LDS: V <= 16256 for labels up to 31, V <= 14336 for
 * labels up to 511); ASR_ERR_UNSUPPORTED otherwise, with nothing written --
 * the caller then runs asr_ctc_backward_bf16 and sums the bias gradient from
 * dY. */
int asr_ctc_bias_supported(int V, int gld, int max_label_len);
size_t asr_ctc_bias_workspace_bytes(int T, int B, int V, int gld);
int asr_ctc_backward_bf16_db(const float* acts, long long stride_t, long long stride_b, int T,
                             int B, int V, const int32_t* labels_flat, const int32_t* label_lens,
                             const int32_t* act_lens, int max_label_len, int blank,
                             const float* grad_scale, float scale, uint16_t* grads,
                             long long gstride_t, long long gstride_b, int gld,
                             const void* workspace, size_t ws_bytes, float* dbias, void* bias_ws,
                             size_t bias_ws_bytes, void* stream);
/* warp-ctc drop-in: forward + backward with scale 1 in one call. */
int asr_ctc_fwd_bwd(const float* acts, long long stride_t, long long stride_b, int T, int B,
                    int V, const int32_t* labels_flat, const int32_t* label_lens,
                    const int32_t* act_lens, int max_label_len, int blank, int zero_infinity,
                    float* costs, float* grads, void* workspace, size_t ws_bytes, void* stream);

/* Which kernels the last CTC forward / gradient ran (host-side record), out2 =
 * {normaliser: 0 the emission pass over the logits, 1 the head GEMM
 * epilogue's partials; gradient: 0 f32 ctc_grad, 1 ctc_grad_bf16, 2 narrow
 * (V <= 256), 3 pipelined, 4 streamed}. */
int asr_ctc_last_path(int* out2);
/* Which kernel asr_ctc_backward_bf16 (with_bias 0) or asr_ctc_backward_bf16_db
 * (with_bias 1) would run for these shapes, and on which grid, under the
 * current ASR_CTC_* environment switches: the library's own plan, answered on
 * the host with nothing launched.  acts is looked at for its 16-B alignment
 * only, never dereferenced.  cus: the CU count to plan for, 0 = the current
 * device's (only then is a GPU needed).  path is numbered as
 * asr_ctc_last_path's gradient entry (1 .. 4); nch and aligned are the
 * kernel's chunks-per-thread and aligned-rows template arguments (nch 0:
 * the form without bias sums); threads, rpb, nblk: work-group size, rows per
 * work-group, work-groups; lds_bytes: dynamic LDS per work-group; rev: rows
 * descending (ASR_CTC_ORDER bit 1); acts_bytes: the activations' extent for
 * buffer loads (0: plain loads); part_bytes: the nblk column partials at the
 * head of bias_ws (0 without bias sums).  ASR_ERR_UNSUPPORTED, with the reason
 * in the error text, where the gradient entry point would refuse. */
typedef struct {
  int path, nch, aligned, threads, rpb, nblk, rev, acts_bytes;
  size_t lds_bytes, part_bytes;
} asr_ctc_grad_plan_t;
int asr_ctc_grad_plan(int T, int B, int V, int gld, int max_label_len, const void* acts,
                      long long stride_t, long long stride_b, int with_bias, int cus,
                      asr_ctc_grad_plan_t* out);
/* Waves per direction of the last CTC forward's lattice (round 6): 1 = the
 * one-wave ctc_lattice, 2 / 4 = ctc_lattice_w (ASR_CTC_LATTICE_W=1 forces 1). */
int asr_ctc_last_lattice_waves(void);
/* Tag of the last GEMM launch (4 x kernel family + operand mode, the
 * ASR_PTAG_GEMM_* families of csrc/prof.h): diagnostics, tools/gemm_log.py. */
int asr_gemm_last_family(void);

/* ---------------------------------------------------------------- GEMM
 * C(m,n) = alpha * sum_k A(m,k) B(n,k) + beta * C(m,n) + bias[n] + bias2[n]  (f32 C)
 * Replaces every nn.Linear / LinearND GEMM (linear.py:15-47) and the LSTM
 * input-projection and weight-gradient GEMMs inside nn.LSTM.
 *
 * A row map turns a logical row index r into memory:
 *   g = r / rows_per_b, t = r % rows_per_b, tp = t*t_mul + t_add,
 *   row(r) = base + perm[g]*stride_b + tp*stride_t   (perm NULL = identity)
 *   rows with tp outside [0, t_limit) read as zeros (A/B) / are not stored (C).
 * This fuses the length-sort gather (rnn.py:319-326), the pyramidal drop
 * subsampling xs[:,1::2] (rnn.py:415-419) and the h_{t-1} shift of dW_hh
 * into the operand loads.  Operand element (i,k) is at row(i)+k (trans=0) or
 * row(k)+i (trans=1); operands are f32 or bf16 in memory.
 * compute_dtype ASR_DT_F32: exact-f32 MFMA (v_mfma_f32_16x16x4_f32);
 * ASR_DT_BF16: bf16 MFMA with f32 accumulation.  Up to 2 independent
 * problems per launch (e.g. the two LSTM directions).
 */
typedef struct {
  long long stride_b;
  long long stride_t;
  int rows_per_b; /* <= 0: a single group */
  int t_mul;      /* 0 means 1 */
  int t_add;
  int t_limit;    /* <= 0: unlimited */
  const int32_t* perm;
} asr_rowmap_t;

typedef struct {
  const void* ptr;
  int dtype;
  int trans;
  asr_rowmap_t map;
  /* bytes readable from ptr (the rest of its allocation), 0 = unknown.  Known
   * extents < 2 GiB let bf16 operands use the range-checked buffer-load path
   * (out-of-range and masked rows read as zeros straight into LDS). */
  long long bytes;
  /* 3x3 "tap" addressing (implicit-GEMM convolution over a zero-haloed
   * [rows = padded pixels][channels] layout), 0 = off.  The contiguous index x
   * (k for trans=0, the output index for trans=1) splits into tap = x /
   * tap_group and x' = x % tap_group; the element is read at column x' of row
   * r + tap_sign * ((tap / 3 - 1) * tap_pitch + tap % 3 - 1).  Needs
   * tap_group % 16 == 0 (trans=0) or % 8 == 0 (trans=1). */
  int tap_group;
  int tap_pitch;
  int tap_sign;
} asr_operand_t;

typedef struct {
  asr_operand_t a;
  asr_operand_t b;
  float* c;
  asr_rowmap_t c_map;
  const float* bias;  /* nullable, f32 [N] */
  const float* bias2; /* nullable, f32 [N], added too (nn.LSTM b_ih + b_hh) */
  int M, N, K;
  float alpha, beta;
  int batch;          /* <= 1: single; else `batch` independent products */
  long long batch_stride_a, batch_stride_b, batch_stride_c; /* elements */
  /* drop_p > 0: the written value is multiplied by asr_dropout's mask for the
   * element's offset i from c (kept iff u01(drop_seed, i) >= drop_p, scale
   * 1 / (1 - drop_p)): dropout's backward fused into the producing GEMM. */
  float drop_p;
  unsigned long long drop_seed;
  /* ASR_DT_F32 (0, the default of a zeroed struct) or ASR_DT_BF16: C is
   * written as bf16 (bf16 compute, beta 0; the product is not split over K;
   * the 128 x 128 / 256 x 64 / generic kernels). */
  int c_dtype;
} asr_gemm_t;

/* One call's settings (NULL = all zero = the defaults); a value other than 0 or
 * 1 is ASR_ERR_ARG before any launch.
 *   small_tiles: the call uses only the 128 x 128 kernel (64 KB of LDS per
 *     work-group), so that its work-groups fit beside a persistent recurrence
 *     work-group on every CU (weight gradients co-resident with the backward
 *     recurrence).
 *   nosplit: the call takes no split-K slabs, and asr_gemm_workspace_bytes
 *     counts none (rows of one product computed by several launches then sum
 *     every output element in the order one launch would: bitwise the same dX
 *     either way).
 *   n64_kmode: products with N <= 64 (M >= 4096) whose B is K-major also take
 *     the 256 x 64 kernel. */
typedef struct { int small_tiles, nosplit, n64_kmode; } asr_gemm_opts_t;

int asr_gemm(const asr_gemm_t* problems, int nprob, int compute_dtype, void* stream,
             const asr_gemm_opts_t* opts);

/* Same product with a workspace for deterministic split-K: weight-gradient
 * GEMMs (dW = dgates^T x over B*T rows, K ~ 32000) have few output tiles and
 * a long K; they are split along K into fixed f32 slabs and summed in a fixed
 * order by a second kernel (bit-reproducible run to run).  The split is a pure
 * function of the shapes and opts; asr_gemm_workspace_bytes returns 0 when no
 * problem splits (then workspace may be NULL and this equals asr_gemm). */
size_t asr_gemm_workspace_bytes(const asr_gemm_t* problems, int nprob,
                                const asr_gemm_opts_t* opts);
int asr_gemm_ws(const asr_gemm_t* problems, int nprob, int compute_dtype, void* workspace,
                size_t ws_bytes, void* stream, const asr_gemm_opts_t* opts);
/* asr_gemm_ws of ONE product (beta 0, no dropout, f32 C, batch 1) whose
 * epilogue also writes, for every row m < M and 64-column slab q < ceil(N/64),
 * the online log-sum-exp pair of the values written to C: lse[2 (q M + m)] =
 * max, lse[2 (q M + m) + 1] = sum exp(c - max) (the CTC normaliser of an
 * output layer, formed where the logits are produced; asr_ctc_forward_lse). */
int asr_gemm_lse_ws(const asr_gemm_t* problem, int compute_dtype, float* lse, void* workspace,
                    size_t ws_bytes, void* stream, const asr_gemm_opts_t* opts);

/* Enqueue on `stream` a one-wave gate that releases once the NEXT persistent
 * backward recurrence (asr_lstm_backward*, any stream) has all its work-groups
 * resident, or after ~5 ms.  Work queued behind it on `stream` (the small-tile
 * weight-gradient GEMMs) then runs beside that recurrence.  Timing only. */
int asr_lstm_wgrad_gate(void* stream);

/* out0[n] (+ out1[n] if non-NULL) += alpha * sum_m g[m*ld + n]  (bias grads of
 * nn.Linear / nn.LSTM bias_ih and bias_hh); fixed-order, deterministic. */
size_t asr_colsum_workspace_bytes(int M, int N);
int asr_colsum_accumulate(const float* g, long long ld, int M, int N, float alpha, float* out0,
                          float* out1, void* workspace, size_t ws_bytes, void* stream);
/* asr_colsum_accumulate over a bf16 matrix (f32 sums). */
int asr_colsum_accumulate_bf16(const uint16_t* g, long long ld, int M, int N, float alpha,
                               float* out0, float* out1, void* workspace, size_t ws_bytes,
                               void* stream);

/* ---------------------------------------------------------- LSTM layer
 * Bidirectional recurrence of one encoder layer (nn.LSTM bidirectional with
 * pack/pad semantics, rnn.py:166-172,218-224,343-390).  Gate order i,f,g,o.
 * gx_act: f32 [B][T][8H]; on entry x@W_ih^T + b_ih + b_hh (forward dir in
 *   columns [0,4H), reverse in [4H,8H)); on exit the post-activation gates
 *   (i,f,g,o) needed by backward.  whh: [2][4H][H] (forward then reverse),
 *   f32 or bf16 (w_dtype).  lens: int32 [B] device (frames >= lens[b] give
 *   zero state / output).  y: f32 [B][T][2H] = [h_fwd ; h_bwd]; cst: f32
 *   [B][T][2H] cell states.  compute_dtype selects bf16 or exact-f32 MFMA for
 *   h @ W_hh^T (state and accumulation always f32).
 * Backward: dy f32 [B][T][2H] (nullable = 0); act_dg holds the saved gates on
 *   entry and the pre-activation gate gradients dG on exit (feeds the weight
 *   gradient GEMMs: dW_ih = dG^T x, dW_hh = dG^T h_prev, db = colsum dG).
 * ybf / dgbf (nullable): bf16 copies of y [B][T][2H] / dG [B][T][8H], written by
 *   the persistent kernels as they go, for the bf16 weight-gradient GEMMs.
 * bf16 mode runs each pass as ONE persistent launch when the grid is
 *   co-resident (see lstm_persist.hip), else one launch per time step.
 * opts: the tagged-granule recurrence's settings for that call alone (NULL =
 * all zero = the defaults).  Every call reads ws_prezeroed, the bf16 backward
 * calls the pin and the units, asr_lstm_backward_dgbf_h alone the dy flags and
 * the progress report; a value out of range is ASR_ERR_ARG before any launch.
 *   ws_prezeroed: the workspace's leading asr_lstm_ws_zero_bytes(B, H) bytes
 *     are already zero (native_ops.rec_arena_begin: one fill per training
 *     step), so a tagged-granule launch skips its own memset.
 *   bwd_pin_kb: the backward's dynamic-LDS pin, 0 (ASR_XG_PIN_BWD_KB, else
 *     140) or KB in (80, 160].  At the default no kernel with more than 9 KB
 *     of LDS -- every GEMM and convolution kernel -- can be co-resident with it.
 *   bwd_units: hidden units per backward work-group, 0 (ASR_XG_BWD_XU, else
 *     16), 16, or 32 -- half the work-groups, which leaves CUs to the layer
 *     above's weight-gradient GEMMs (native_ops' ASR_OVERLAP_WGRAD mode 3).  32
 *     only where H % 32 == 0, H <= 512 and 8 rows per group fit; else 16.
 *   dy_flags, dy_c0 > 0, dy_epoch != 0 (flags NULL: off): dy is written
 *     concurrently by the layer above's dX GEMMs (rnn.py:343-390's stacked
 *     layers), in chunks of processing steps q in [c0 k, c0 (k + 1)) -- rows
 *     t = q and t = T - 1 - q -- complete once flags[k] == epoch (up to the
 *     middle step (T + 1) / 2 - 1); the recurrence waits for each chunk's flag.
 *   progress, progress_q1 >= 0, progress_q2 (NULL: off): the launch adds 1 to
 *     *progress per cell wave once the gate gradients of processing steps
 *     <= q1 are stored and released at agent scope, and again at q2 > q1
 *     (q2 < 0: one step).  Step q covers t = T-1-q (forward direction) and
 *     t = q (reverse): rows t in [T-1-q, q] of dG are final once q >= T/2. */
typedef struct {
  int ws_prezeroed, bwd_pin_kb, bwd_units;
  const int* dy_flags;
  int dy_c0, dy_epoch;
  unsigned long long* progress;
  int progress_q1, progress_q2;
} asr_lstm_opts_t;
size_t asr_lstm_workspace_bytes(int B, int H, int compute_dtype, int backward);
int asr_lstm_forward(float* gx_act, const void* whh_f, const void* whh_r, int w_dtype,
                     const int32_t* lens, int B, int T, int H, int compute_dtype, float* y,
                     float* cst, uint16_t* ybf, void* workspace, size_t ws_bytes, void* stream,
                     const asr_lstm_opts_t* opts);
int asr_lstm_backward(const float* dy, const void* whh_f, const void* whh_r, int w_dtype,
                      const int32_t* lens, int B, int T, int H, int compute_dtype, float* act_dg,
                      const float* cst, uint16_t* dgbf, void* workspace, size_t ws_bytes,
                      void* stream, const asr_lstm_opts_t* opts);
/* asr_lstm_backward plus the bias gradients of nn.LSTM's bias_ih / bias_hh
 * (both [2 dirs x 4H], accumulated +=, identical values: both biases feed the
 * same gate pre-activation, rnn.py:166-172).  The tagged-granule recurrence
 * sums them inside the pass; other paths reduce dG afterwards.  workspace:
 * asr_lstm_workspace_bytes(B, H, compute_dtype, 2). */
int asr_lstm_backward_db(const float* dy, const void* whh_f, const void* whh_r, int w_dtype,
                         const int32_t* lens, int B, int T, int H, int compute_dtype,
                         float* act_dg, const float* cst, uint16_t* dgbf, float* db_ih,
                         float* db_hh, void* workspace, size_t ws_bytes, void* stream,
                         const asr_lstm_opts_t* opts);
/* asr_lstm_backward_db for a caller that feeds only the bf16 gate gradients
 * (dgbf, required) to its weight / input gradient GEMMs: the tagged-granule
 * recurrence skips the f32 dG stores and act_dg's contents are unspecified on
 * exit.  Same workspace as asr_lstm_backward_db. */
int asr_lstm_backward_dgbf(const float* dy, const void* whh_f, const void* whh_r, int w_dtype,
                           const int32_t* lens, int B, int T, int H, int compute_dtype,
                           float* act_dg, const float* cst, uint16_t* dgbf, float* db_ih,
                           float* db_hh, void* workspace, size_t ws_bytes, void* stream,
                           const asr_lstm_opts_t* opts);

/* Forward layer pass with the input projection fused into the persistent
 * recurrence (bf16 mode; replaces asr_gemm(gx = x W_ih^T + b_ih + b_hh) +
 * asr_lstm_forward): x [B*T][Din] bf16 rows (b, t) of the layer input, wih
 * [8H][Din] bf16 = [W_ih fwd; W_ih rev], b_ih / b_hh f32 [8H], whh f32 [4H][H]
 * per direction.  act [B][T][8H] f32 receives the post-activation gates (the
 * backward's input, as gx_act after asr_lstm_forward); y, cst, ybf as there.
 * ASR_ERR_UNSUPPORTED: this shape / device does not take the path
 * (asr_lstm_forward_x_ok tells beforehand). */
int asr_lstm_forward_x(const uint16_t* x, int Din, const uint16_t* wih, const float* b_ih,
                       const float* b_hh, const float* whh_f, const float* whh_r,
                       const int32_t* lens, int B, int T, int H, float* act, float* y, float* cst,
                       uint16_t* ybf, void* workspace, size_t ws_bytes, void* stream,
                       const asr_lstm_opts_t* opts);
int asr_lstm_forward_x_ok(int B, int H, int Din);
/* asr_lstm_forward_x with the gate activations stored packed as fp16:
 * act_h [B][T][2][H][4] (i, f, g, o of one (utterance, frame, direction,
 * unit) in one 8-B word; 8 B per cell instead of 16, one store instead of
 * four).  Read back by asr_lstm_backward_dgbf_h (or unpacked to the f32
 * [B][T][8H] layout by asr_lstm_unpack_act_h).  Replaces the same nn.LSTM
 * forward as asr_lstm_forward_x (models/pytorch_v3/encoders/rnn.py:166-172). */
int asr_lstm_forward_xh(const uint16_t* x, int Din, const uint16_t* wih, const float* b_ih,
                        const float* b_hh, const float* whh_f, const float* whh_r,
                        const int32_t* lens, int B, int T, int H, uint16_t* act_h, float* y,
                        float* cst, uint16_t* ybf, void* workspace, size_t ws_bytes,
                        void* stream, const asr_lstm_opts_t* opts);
/* asr_lstm_forward_xh for a layer whose output feeds only the next BLSTM
 * layer's staged bf16 input (the stacked nn.LSTM layers of
 * models/pytorch_v3/encoders/rnn.py:343-390 with dropout between them,
 * rnn.py:398): y may be NULL (the f32 output is then not written); ydrop,
 * when non-NULL, receives bf16(dropout(y)) [B][T][2H] with asr_dropout's mask
 * for (drop_p, drop_seed) -- what asr_convert_rows_bf16_dropout would stage
 * from y; ybf (bf16 y) is required. */
int asr_lstm_forward_xh_drop(const uint16_t* x, int Din, const uint16_t* wih, const float* b_ih,
                             const float* b_hh, const float* whh_f, const float* whh_r,
                             const int32_t* lens, int B, int T, int H, uint16_t* act_h,
                             float* y, float* cst, uint16_t* ybf, uint16_t* ydrop, float drop_p,
                             unsigned long long drop_seed, void* workspace, size_t ws_bytes,
                             void* stream, const asr_lstm_opts_t* opts);
/* asr_lstm_backward_dgbf reading act_h of asr_lstm_forward_xh (tagged-granule
 * recurrence only; ASR_ERR_UNSUPPORTED otherwise).  Same workspace. */
int asr_lstm_backward_dgbf_h(const float* dy, const void* whh_f, const void* whh_r, int w_dtype,
                             const int32_t* lens, int B, int T, int H, int compute_dtype,
                             const uint16_t* act_h, const float* cst, uint16_t* dgbf,
                             float* db_ih, float* db_hh, void* workspace, size_t ws_bytes,
                             void* stream, const asr_lstm_opts_t* opts);
int asr_lstm_unpack_act_h(const uint16_t* act_h, int B, int T, int H, float* act, void* stream);
/* Diagnostics only (tools/buckets_diag.py, ASR_DIAG_SPIN): nwg work-groups of
 * 256 threads that fill 64 KB of LDS with a pattern and check it `iters`
 * times; mismatches are added to *bad (device int). */
int asr_diag_lds_spin(int nwg, int iters, int* bad, void* stream);

/* Diagnostics only (tests/test_coresidency_gpu.py): nwg work-groups of 256
 * threads holding lds_bytes of LDS each stay resident for usec microseconds
 * (a long-lived kernel beside the next persistent recurrence launch). */
int asr_diag_hold_cus(int nwg, int lds_bytes, int usec, void* stream);

/* ------------------------------------------------------------ GRU layer
 * Replaces the packed nn.GRU(bidirectional=True) of
 * models/pytorch_v3/encoders/rnn.py:173-191 (fast path) / :226-233 (per layer).
 * Gate order r, z, n; h0 = 0; outputs and state are 0 for t >= lens[b].
 *   gx_act [B][T][6H] f32: in  x W_ih^T + b_ih (forward cols [0,3H), reverse [3H,6H))
 *                          out r, z, n (post-activation), then dgx after backward
 *   whh    [2][3H][H] f32 (forward then reverse), bhh [2][3H] f32
 *   y      [B][T][2H] f32 out = [h_fwd ; h_rev];  ghn [B][T][2H] f32 out = W_hn h + b_hn
 * Backward: dy [B][T][2H] (nullable = 0); writes dgx over gx_act and
 * dgh [B][T][6H] = the gate gradients of W_hh h + b_hh; the weight / bias /
 * input gradients are GEMMs and column sums of dgx and dgh.  One launch per
 * time step (both directions), exact-f32 MFMA. */
size_t asr_gru_workspace_bytes(int B, int H);
int asr_gru_forward(float* gx_act, const float* whh, const float* bhh, const int32_t* lens, int B,
                    int T, int H, float* y, float* ghn, void* stream);
int asr_gru_backward(const float* dy, const float* whh, const int32_t* lens, int B, int T, int H,
                     float* act_dgx, const float* ghn, const float* y, float* dgh,
                     void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------ unidirectional LSTM layer
 * Replaces the packed nn.LSTM(bidirectional=False) of
 * models/pytorch_v3/encoders/rnn.py:166-172 (fast path) / :218-224 (per layer),
 * the encoder_bidirectional=False form.  Gate order i, f, g, o; h0 = c0 = 0;
 * outputs and state are 0 for t >= lens[b] (pad_packed's zeros).
 *   gx_act [B][T][4H] f32: in  x W_ih^T + b_ih + b_hh
 *                          out i, f, g, o (post-activation, 0 at padded frames),
 *                          then the pre-activation gate gradients dG after backward
 *   whh    [4H][H], w_dtype f32 or bf16 (f32 compute needs f32)
 *   lens   int32 [B];  y, cst [B][T][H] f32 out (h_t, c_t)
 *   ybf    optional bf16 copy of y;  dgbf optional bf16 copy of dG
 * Backward: dy [B][T][H] (NULL = 0; values at t >= lens[b] are ignored);
 * db_ih (required) and db_hh (optional), [4H], are accumulated (+=) with the
 * column sums of dG, identical values, by a fixed-order reduction: results
 * are bitwise reproducible.  The weight and input gradients are GEMMs of dG
 * by the caller.
 * compute_dtype f32: f32 state, exact-f32 MFMA.  bf16: h (forward) and dG
 * (backward) rounded to bf16 as MFMA operands beside a bf16 W_hh, f32
 * accumulation and f32 state.
 * One launch per time step and pass (product and cell math in one kernel;
 * only the stream orders the steps), plus one weight conversion / transpose
 * launch and, in the backward, the two column-sum launches.
 * Accepted shapes: 1 <= B <= 8192, 1 <= T <= 65536, 1 <= H <= 1024 (H % 8 == 0
 * takes vector fragment loads, any other H guarded scalar ones).  Any other
 * positive shape is ASR_ERR_UNSUPPORTED before any launch, nothing written.  workspace: asr_lstm_uni_workspace_bytes(B, H,
 * compute_dtype, backward != 0); it need not be zero.
 * asr_lstm_uni_shape_ok: 1 for an accepted shape, else 0 (host only). */
int asr_lstm_uni_shape_ok(int B, int T, int H);
size_t asr_lstm_uni_workspace_bytes(int B, int H, int compute_dtype, int backward);
int asr_lstm_uni_forward(float* gx_act, const void* whh, int w_dtype, const int32_t* lens, int B,
                         int T, int H, int compute_dtype, float* y, float* cst, uint16_t* ybf,
                         void* workspace, size_t ws_bytes, void* stream);
int asr_lstm_uni_backward(const float* dy, const void* whh, int w_dtype, const int32_t* lens, int B,
                          int T, int H, int compute_dtype, float* act_dg, const float* cst,
                          uint16_t* dgbf, float* db_ih, float* db_hh, void* workspace,
                          size_t ws_bytes, void* stream);

/* ------------------------------------ stateful recurrence (streaming inference)
 * One chunk of Tc frames of a unidirectional LSTM layer with the state carried
 * in and out (csrc/lstm_stream.hip): asr_lstm_uni_forward's cell and roundings,
 * no saved activations.
 *   gx     [B][Tc][4H] f32, read only: x W_ih^T + b_ih + b_hh, gates i, f, g, o
 *   whh    [4H][H], w_dtype f32 or bf16 (f32 compute needs f32; a caller that
 *          feeds many chunks converts W_hh once and passes the bf16 copy)
 *   lens   int32 [B]: valid frames of row b in this chunk, 0 <= lens[b] <= Tc
 *          (values outside are clipped to that range)
 *   h_in, c_in [B][H] f32: the state before the chunk's first frame
 *   h_out, c_out [B][H] f32: the state after frame lens[b] - 1; h_in[b], c_in[b]
 *          unchanged where lens[b] == 0
 *   y      [B][Tc][H] f32: h_t for t < lens[b], 0 for t >= lens[b]
 * For t >= lens[b] the state is frozen, not zeroed -- the one difference from
 * asr_lstm_uni_forward -- so a row that ended early, or has no frame in this
 * chunk, continues from its state in the next one.  The state is always f32.
 * compute_dtype f32: exact-f32 MFMA.  bf16: h and W_hh rounded to bf16 as MFMA
 * operands, f32 sums, state and cell math.  Feeding an utterance in chunks
 * gives, bit for bit, what one call over the whole utterance gives.
 * Aliasing: h_out must not overlap h_in (step 0 reads all of h_in[b] in every
 * work-group of row b while h_out[b] is being written): ASR_ERR_ARG.  c_out
 * may be c_in itself (each c[b][j] has one reader and writer), any other
 * overlap of the two is ASR_ERR_ARG.  So is every other overlap of an output
 * (y, h_out, c_out) with another output or with gx, h_in or c_in, and in bf16
 * mode with H % 8 == 0 an h_in, y or bf16 whh that is not 16-byte aligned.
 * whh, lens and the workspace must not overlap an output either; that is not
 * checked.  The step launches are not recorded by the launch profiler.
 * Accepted shapes: asr_lstm_uni_shape_ok(B, Tc, H); anything else is
 * ASR_ERR_UNSUPPORTED before any launch, nothing written.  One launch per
 * frame, ordered by the stream.  workspace: asr_lstm_stream_workspace_bytes(B,
 * H, compute_dtype); read only in bf16 mode with an f32 whh (the converted
 * copy), may be NULL otherwise; it need not be zero. */
size_t asr_lstm_stream_workspace_bytes(int B, int H, int compute_dtype);
int asr_lstm_stream_forward(const float* gx, const void* whh, int w_dtype, const int32_t* lens,
                            int B, int Tc, int H, int compute_dtype, const float* h_in,
                            const float* c_in, float* h_out, float* c_out, float* y,
                            void* workspace, size_t ws_bytes, void* stream);

/* nn.GRUCell nonlinearity (decoder cells, rnn_decoder.py:91-95): gi = x W_ih^T +
 * b_ih, gh = h W_hh^T + b_hh [B][3D] (GEMMs by the caller); act [B][3D] out =
 * r, z, n; hout = (1 - z) n + z h.  Backward: dgi, dgh [B][3D] (the gate
 * gradients of the two GEMMs' outputs) and dh_prev = dh z (the direct term;
 * the caller adds dgh W_hh). */
int asr_gru_cell_forward(const float* gi, const float* gh, const float* h, int B, int D,
                         float* act, float* hout, void* stream);
int asr_gru_cell_backward(const float* act, const float* gh, const float* h, const float* dh,
                          int B, int D, float* dgi, float* dgh, float* dh_prev, void* stream);

/* ------------------------------------------------------------ optimizer
 * Replaces torch.nn.utils.clip_grad_norm(params, max_norm)
 * (utils/training/training_loop.py:46-50) + torch.optim Adam / SGD /
 * momentum / nesterov (models/pytorch_v3/base.py:141-194) over the model's
 * flat f32 parameter and gradient buffers.
 * asr_grad_sqnorm: out[0] = sum g^2 (deterministic; g 16-B aligned).
 * asr_optim_step: kind 0 adam (m, v), 1 sgd, 2 momentum (m), 3 nesterov (m);
 *   the clip coefficient min(1, max_norm / (sqrt(*grad_sqnorm) + 1e-6)) is
 *   computed on device (grad_sqnorm NULL or max_norm <= 0: no clipping);
 *   weight decay is L2 added to the gradient (torch semantics); step is the
 *   1-based step count for Adam bias correction; bf16_shadow (nullable)
 *   receives a bf16 copy of the updated parameters.
 */
size_t asr_grad_sqnorm_workspace_bytes(void);
int asr_grad_sqnorm(const float* g, long long n, float* out, void* workspace, size_t ws_bytes,
                    void* stream);
/* asr_optim_step_guarded: the same with guard (device int32[2], nullable):
 * when guard[0] | guard[1] != 0 (asr_lstm_status_gather's words) the kernel
 * leaves params and state untouched. */
int asr_optim_step_guarded(int kind, float* params, const float* grads, float* m, float* v,
                           long long n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, long long step, float momentum, float dampening,
                           const float* grad_sqnorm, float max_norm, uint16_t* bf16_shadow,
                           const int* guard, void* stream);
int asr_optim_step(int kind, float* params, const float* grads, float* m, float* v, long long n,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   long long step, float momentum, float dampening, const float* grad_sqnorm,
                   float max_norm, uint16_t* bf16_shadow, void* stream);

/* ------------------------------------------------------- elementwise
 * asr_dropout: y = x * (u(seed, i) >= p) / (1 - p), u a counter hash (the
 *   mask is recomputed from (seed, i) in backward: call again on dy).  u(seed,
 *   i) is 16-bit field i % 2 of lowbias32(((i / 2) * 0x9E3779B9) ^ key), key =
 *   lowbias32((uint32)seed ^ (uint32)(seed >> 32) * 0x85EBCA6B), divided by
 *   65536 (two elements per 32-bit hash; one stream covers 2^33 elements;
 *   oracle/rng.py restates it).
 *   Replaces nn.Dropout on the encoder / decoder activations.
 * asr_embedding_*: nn.Embedding(padding_idx) lookup / gradient (linear.py:50-77;
 *   trans=1: weight stored [E][V], the one-hot @ W^T of Embedding_LS,
 *   linear.py:80-116).  idx int64 [n]; an index outside [0, V) reads row
 *   clamp(idx, 0, V-1), and both backward forms send its gradient to that
 *   same row.  Backward is deterministic and skips padding_idx (pass -1 for
 *   none).
 * asr_tanh_*: F.tanh of the encoder projection / attention bottleneck.
 */
int asr_dropout(const float* x, float* y, long long n, float p, unsigned long long seed,
                void* stream);
int asr_embedding_forward(const long long* idx, const float* weight, int n, int V, int E,
                          int trans, float* out, void* stream);
int asr_embedding_backward(const long long* idx, const float* dout, int n, int V, int E,
                           int trans, int padding_idx, float* grad_weight, void* stream);
/* The embedding gradient with the rows grouped by token (CSR built on the host
 * from the label array the caller already holds: rows order[starts[v] ..
 * starts[v+1]) carry token v in ascending order).  Same sums, O(n E). */
int asr_embedding_backward_csr(const int32_t* order, const int32_t* starts, const float* dout,
                               int V, int E, int trans, int padding_idx, float* grad_weight,
                               void* stream);
/* nn.LSTMCell nonlinearity (RNNDecoder.forward, rnn_decoder.py:80-86): pre
 * [B][4D] gate pre-activations (i, f, g, o) -> h, c [B][D]; act [B][4D] the
 * activated gates kept for the backward.  c_prev nullable (zero state).
 * Backward: dh / dc nullable cotangents -> dpre [B][4D], dc_prev [B][D]
 * (nullable). */
int asr_lstm_cell_forward(const float* pre, const float* c_prev, int B, int D, float* act,
                          float* h, float* c, void* stream);
int asr_lstm_cell_backward(const float* act, const float* c_prev, const float* c,
                           const float* dh, const float* dc, int B, int D, float* dpre,
                           float* dc_prev, void* stream);
int asr_tanh_forward(const float* x, float* y, long long n, void* stream);
int asr_tanh_backward(const float* y, const float* dy, float* dx, long long n, void* stream);
/* y = tanh(a + b) (attention bottleneck with per-branch dropout,
 * attention_seq2seq.py:788-790); its backward is asr_tanh_backward for both. */
int asr_add_tanh_forward(const float* a, const float* b, float* y, long long n, void* stream);
/* y = a + b: the encoder's residual / dense-residual sums (rnn.py:456-462);
 * the backward is the identity to both inputs. */
int asr_add_forward(const float* a, const float* b, float* y, long long n, void* stream);

/* dst[r][0:ncols] = bf16(src[row(r) + 0:ncols]) (round to nearest even) for r <
 * nrows, rows through an asr_rowmap_t (perm / subsample gathers; rows outside
 * [0, t_limit) become zeros).  Builds the dense bf16 GEMM operands of the
 * encoder layer (its input X, W_ih) in bf16 mode.  Any alignment of src and
 * dst is accepted: rows that are not 16-B aligned take a scalar kernel (the
 * same bits, and for the dropout form below the same mask). */
int asr_convert_rows_bf16(const float* src, asr_rowmap_t map, int nrows, int ncols,
                          uint16_t* dst, void* stream);
/* Same with an output row pitch ld >= ncols; columns [ncols, ld) are zeros (a
 * bf16 operand whose leading dimension is padded to a multiple of 8). */
int asr_convert_rows_bf16_ld(const float* src, asr_rowmap_t map, int nrows, int ncols, int ld,
                             uint16_t* dst, void* stream);
/* Up to four asr_convert_rows_bf16 conversions in one launch (round 6: a
 * staged linear layer's input, weight and zero pad rows).  Each needs ncols % 8
 * == 0, 16-B aligned rows (src, dst, map strides); returns 1 when launched, 0
 * when a job does not qualify (nothing launched: convert one by one), < 0 on
 * a launch error.  The same bits as the one-by-one conversions. */
int asr_convert_rows_bf16_multi(int n, const float* const* src, const asr_rowmap_t* maps,
                                const int* nrows, const int* ncols, uint16_t* const* dst,
                                void* stream);
/* asr_convert_rows_bf16 of dropout(src): element at linear offset i of src is
 * kept iff u(seed, i) >= p and scaled by 1/(1-p) -- the mask asr_dropout(src,
 * ., n, p, seed) applies -- so a layer's dropped output is staged as the next
 * layer's bf16 GEMM operand in one pass (nn.Dropout after each BLSTM layer,
 * models/pytorch_v3/encoders/rnn.py:392-393, fused with the input staging). */
int asr_convert_rows_bf16_dropout(const float* src, asr_rowmap_t map, int nrows, int ncols,
                                  uint16_t* dst, float p, unsigned long long seed, void* stream);

/* ------------------------------------------------------------ decoding
 * asr_ctc_best_path: CTC greedy best path (greedy_decoder.py:19-47): per
 *   utterance argmax over V for t < lens[b] (first maximum wins ties, as
 *   np.argmax), collapse repeats, drop `blank`.  hyps int32 [B][T] (first
 *   hyp_lens[b] valid), hyp_lens int32 [B].  Bit-exact with the reference.
 * asr_row_argmax: out[r] = argmax_v x[r*V + v] (int64; first max on ties).
 * In both, a NaN never wins and the result is always in [0, V): a row / frame
 * of all NaN (or all -inf) gives 0.
 * asr_ctc_best_path_stream: asr_ctc_best_path on one chunk [B][T] of longer
 *   utterances.  prev int32 [B], read and written: the label of row b's last
 *   valid frame so far, -1 before its first frame; a repeat run collapses
 *   across the chunk boundary through it; left unchanged where lens[b] == 0.
 *   hyps / hyp_lens hold only the labels this chunk newly emits, so the
 *   chunks' outputs concatenated are asr_ctc_best_path's on the whole logits.
 */
int asr_ctc_best_path(const float* logits, long long stride_t, long long stride_b, int T, int B,
                      int V, const int32_t* lens, int blank, int32_t* hyps, int32_t* hyp_lens,
                      void* stream);
int asr_ctc_best_path_stream(const float* logits, long long stride_t, long long stride_b, int T,
                             int B, int V, const int32_t* lens, int blank, int32_t* prev,
                             int32_t* hyps, int32_t* hyp_lens, void* stream);
int asr_row_argmax(const float* x, int rows, int V, long long* out, void* stream);
/* asr_ctc_beam_search: CTC prefix beam search (beam_search_decoder.py:22-124
 *   with alpha = beta = 0): per utterance the most probable prefix among the
 *   beam_width kept per frame, prefixes ranked by logaddexp(p_blank,
 *   p_nonblank), candidates that denote the same prefix summed before ranking.
 *   logits / strides / lens as asr_ctc_best_path (lens[b] is clipped to T;
 *   frames at t >= lens[b] are never read).  normalize != 0: logits are raw
 *   and the log-softmax is fused; normalize == 0: logits are log-probabilities.
 *   hyps int32 [B][T] (first hyp_lens[b] valid), hyp_lens int32 [B], scores
 *   float32 [B] = log-probability of the returned prefix (lens[b] == 0: empty
 *   hypothesis, score 0).  float32 arithmetic throughout.  On exactly equal
 *   scores: entries already in the beam before extensions, by their previous
 *   rank; extensions by parent rank, then by (logit descending, class
 *   ascending).  A NaN logit never enters the per-frame class ranking.
 *   Refused with ASR_ERR_ARG (nothing launched): beam_width outside [1, 64],
 *   V < 2, blank outside [0, V), a workspace that is not 16-B aligned; with
 *   ASR_ERR_WORKSPACE: one smaller than asr_ctc_beam_ws_bytes(T, B, V,
 *   beam_width) (which is 0 for refused shapes).  The workspace needs no
 *   initialisation.
 */
size_t asr_ctc_beam_ws_bytes(int T, int B, int V, int beam_width);
int asr_ctc_beam_search(const float* logits, long long stride_t, long long stride_b, int T, int B,
                        int V, const int32_t* lens, int blank, int beam_width, int normalize,
                        void* ws, size_t ws_bytes, int32_t* hyps, int32_t* hyp_lens, float* scores,
                        void* stream);
/* The search's first pass alone (per frame: log-sum-exp and the beam_width + 1
 * best non-blank classes, into the workspace); for timing it
 * (tools/ctc_beam_bench.py).  Same checks as asr_ctc_beam_search. */
int asr_ctc_beam_rows(const float* logits, long long stride_t, long long stride_b, int T, int B,
                      int V, const int32_t* lens, int blank, int beam_width, int normalize,
                      void* ws, size_t ws_bytes, void* stream);
/* asr_ctc_beam_search_lm: the prefix search with shallow fusion of an RNN
 * language model and an insertion bonus (csrc/ctc_beam.hip states the contract
 * in full).  lm (asr_att_beam_lm_t, declared with asr_att_beam_decode below;
 * alpha = lm->weight >= 0) has exactly V classes: CTC class c != blank is LM
 * class c - (c > blank), and LM class V - 1 is <eos>, also the LM's start
 * token.  The score of a prefix l after t frames is
 *   log P_ctc,t(l) + alpha sum_i log p_lm(l_i | <eos>, l_<i) + beta |l|,
 * the beam holds the beam_width best distinct prefixes by it, and after the
 * last frame the entries are re-ranked with alpha log p_lm(<eos> | l) added;
 * scores[b] is that value (f32; the LM and every log-softmax run in f32).
 * lm null or lm->weight == 0: the LM term is absent (beta still applies); with
 * beta == 0 too the hypotheses are asr_ctc_beam_search's, by other launches.
 * Launches: 2 + (lm ? 1 : 0) up front, then per frame 2 + (lm ? 1 : 0), then 1;
 * no host read or synchronisation.  Workspace: asr_ctc_beam_lm_ws_bytes
 * (lm_layers == 0: no LM), which needs no initialisation.
 * ASR_ERR_ARG before any launch: asr_ctc_beam_search's refusals, lm->V != V,
 * weight < 0, beta not finite, a null pointer.  ASR_ERR_UNSUPPORTED (nothing
 * launched; the workspace query is 0 for the first two): layers >
 * ASR_ATT_BEAM_LM_MAX_LAYERS, the LM cell's LDS need (2 max(Y, H) + H floats)
 * above 64 KiB, lm->cell != ASR_ATT_BEAM_CELL_LSTM (a GRU LM). */
struct asr_att_beam_lm_s;
size_t asr_ctc_beam_lm_ws_bytes(int T, int B, int V, int beam_width, int lm_layers, int lm_H,
                                int lm_Y);
int asr_ctc_beam_search_lm(const float* logits, long long stride_t, long long stride_b, int T,
                           int B, int V, const int32_t* lens, int blank, int beam_width,
                           int normalize, const struct asr_att_beam_lm_s* lm, double beta, void* ws,
                           size_t ws_bytes, int32_t* hyps, int32_t* hyp_lens, float* scores,
                           void* stream);
/* asr_ctc_beam_stream_*: the two searches above chunk by chunk, their state
 * kept on the device between calls (csrc/ctc_beam.hip, "chunk by chunk").  A
 * session is (max_frames, B, V, beam_width, blank, normalize, lm, beta): every
 * call on one state passes the same values.  lm null or lm->weight == 0: the LM
 * term is absent; with beta == 0 too the plain search runs.
 * Bitwise contract: for any split of a row's frames into feeds -- one-frame
 * chunks, feeds in which lens[b] == 0, ragged rows -- the hyps, hyp_lens and
 * scores of the feed that carries the row's `final` flag are bit for bit those
 * of asr_ctc_beam_search (asr_ctc_beam_search_lm with an LM or beta != 0) on
 * the concatenated logits.
 * asr_ctc_beam_stream_state_bytes: the persistent state.  Per row the beam in
 *   rank order (n, the next node id, and per entry node, parent, last label,
 *   depth, LM slot, p_b, p_nb, hash, parent hash), a pool of max_frames *
 *   beam_width + 1 nodes, the frames consumed and a status word; with an LM
 *   (lm_layers > 0) the 2 beam_width slots of h, c and the cached log-softmax
 *   rows.  0 for refused shapes (max_frames outside [1, (2^31 - 2) / 64], the
 *   refusals of asr_ctc_beam_ws_bytes and asr_ctc_beam_lm_ws_bytes).
 * asr_ctc_beam_stream_ws_bytes: one feed's scratch (the chunk's log-sum-exps
 *   and class lists).  It needs no initialisation and keeps no meaning between
 *   calls.
 * asr_ctc_beam_stream_reset: the rows whose rows[b] != 0 (rows: device int32
 *   [B]; null: every row) at the empty prefix -- p_b = 0, p_nb = -inf, pool
 *   node 0, no frames, status 0 -- and with an LM the root's LM state made from
 *   the zero state and <eos>.  Other rows keep their search state.  A state
 *   must be reset before its first feed.  1 + (lm ? 1 : 0) launches.
 * asr_ctc_beam_stream_feed: advances row b by its lens[b] (clipped to [0, Tc])
 *   frames of logits [B][Tc] (strides as asr_ctc_beam_search); lens[b] == 0
 *   leaves the row's state untouched.  Then per row: the best prefix (rank 0)
 *   in hyps[b * ld_hyp ...], its length in hyp_lens[b], its score S_t (no
 *   <eos> term) in scores[b], and in stable_lens[b] (nullable: not computed)
 *   the length of the longest common prefix of the label sequences of all
 *   beam entries: every later hypothesis descends from a beam entry, so these
 *   first labels never change again.  final: device int32 [B], nullable; for a
 *   row whose flag is set the output is the whole-utterance search's -- with
 *   an LM the entries re-ranked with alpha log p_lm(<eos> | l) added, that
 *   value as the score -- and stable_lens[b] = hyp_lens[b]; the re-ranking is
 *   for the output only, the state is not altered.
 *   Capacity: a row never consumes more than max_frames frames; the frames
 *   past it are dropped and bit 0 of the row's status word is set (bit 1: the
 *   row's counters are not ones a reset or a feed left -- the state was never
 *   reset; the row consumes nothing and reports an empty hypothesis, score
 *   -inf).  The pool is never written past its end.
 *   Launches: 1 (the rows' frame counts), then without LM and bonus the
 *   chunk's pass 1 and one search launch (one wave per utterance: the beam
 *   from the state into LDS, lens[b] frames, back), else the chunk's
 *   log-sum-exps and per chunk frame 2 + (lm ? 1 : 0); then 1 (the output).
 *   No host read, synchronisation or allocation; graph-capture safe.
 *   Refused before any launch: the refusals of asr_ctc_beam_search /
 *   asr_ctc_beam_search_lm (ASR_ERR_UNSUPPORTED: a GRU LM, layers >
 *   ASR_ATT_BEAM_LM_MAX_LAYERS, the LM cell's LDS need above 64 KiB), ld_hyp <
 *   max_frames, a state or workspace that is misaligned (ASR_ERR_ARG) or too
 *   small (ASR_ERR_WORKSPACE).
 * asr_ctc_beam_stream_nbest: every beam entry in rank order: hyps int32
 *   [B][beam_width][ld_hyp], lens and scores [B][beam_width] (S_t,
 *   non-increasing; unused entries: length 0, -inf), counts [B].  lm_layers /
 *   lm_H: those of the state's layout (0, 0 without an LM).  One launch.
 * asr_ctc_beam_stream_status: the rows' status words into status (device int32
 *   [B]); one device-to-device copy on the stream. */
size_t asr_ctc_beam_stream_state_bytes(int max_frames, int B, int V, int beam_width, int lm_layers,
                                       int lm_H, int lm_Y);
size_t asr_ctc_beam_stream_ws_bytes(int Tc, int B, int V, int beam_width);
int asr_ctc_beam_stream_reset(void* state, size_t state_bytes, int max_frames, int B, int V,
                              int beam_width, const struct asr_att_beam_lm_s* lm,
                              const int32_t* rows, void* stream);
int asr_ctc_beam_stream_feed(const float* logits, long long stride_t, long long stride_b, int Tc,
                             int B, int V, const int32_t* lens, int blank, int beam_width,
                             int normalize, const struct asr_att_beam_lm_s* lm, double beta,
                             const int32_t* final, void* state, size_t state_bytes, int max_frames,
                             void* ws, size_t ws_bytes, int32_t* hyps, int ld_hyp,
                             int32_t* hyp_lens, float* scores, int32_t* stable_lens, void* stream);
int asr_ctc_beam_stream_nbest(const void* state, size_t state_bytes, int max_frames, int B, int V,
                              int beam_width, int lm_layers, int lm_H, int32_t* hyps, int ld_hyp,
                              int32_t* lens, float* scores, int32_t* counts, void* stream);
int asr_ctc_beam_stream_status(const void* state, int B, int32_t* status, void* stream);

/* asr_ctc_align: CTC forced alignment (csrc/ctc_align.hip): for each utterance
 *   the best (Viterbi) path of its KNOWN labels through the blank-interleaved
 *   lattice.  Tb = min(act_lens[b], T); labels l_0..l_{L-1} in [0, V), none
 *   equal to `blank` (labels_flat / label_lens as for asr_ctc_forward);
 *   S = 2 L + 1 states, state s of class c(s) = blank (s even) or l_{(s-1)/2}.
 *   The path is chosen on the RAW logits x (a per-frame normaliser moves no
 *   argmax), in float32 adds and compares only:
 *     v_0(0) = x_0[blank], v_0(1) = x_0[l_0], -inf elsewhere;
 *     v_t(s) = fl32(m + x_t[c(s)]), m = the max over the predecessors in the
 *       order s, s-1, s-2 (s-2 only for odd s >= 3 with c(s) != c(s-2)); the
 *       backpointer is the FIRST predecessor in that order that attains m;
 *     end state S-1 if v_{Tb-1}(S-1) >= v_{Tb-1}(S-2), else S-2 (L = 0: 0).
 *   A row is feasible iff the end value is > -inf (not so: Tb = 0 with L > 0,
 *   L + repeats > Tb, a -inf logit on a needed column); a label outside
 *   [0, V), one equal to blank, or a label_len outside [0, max_label_len]
 *   also leaves the row infeasible.
 *   ali int32 [B][T]: c(s_t) for t < Tb, -1 for t >= Tb and for every frame of
 *     an infeasible row.  starts / ends int32 [B][max_label_len] (both may be
 *     NULL): first / last frame (inclusive) in label j's state; -1 for
 *     j >= L and for infeasible rows.  scores f32 [B]: normalize != 0: the
 *     path's log-probability sum_t (x_t[c(s_t)] - lse_t), lse_t over all V
 *     classes (-inf classes add 0), summed per 64-frame chunk by a fixed
 *     lane tree and over the chunks from the last to the first;
 *     normalize == 0: the end value v, bitwise; -inf for an infeasible row;
 *     0 for Tb = 0 with L = 0.
 *   Frames t >= act_lens[b] are never read.  NaN at a blank or label column
 *   is outside the contract (memory-safe, ASR_OK, values unspecified).
 *   Stream work only: no host read, no allocation, no synchronisation; the
 *   workspace need not be zero.  Strides as for asr_ctc_forward (time-major
 *   or batch-major).  max_label_len > 511 (more than 1024 lattice states) or
 *   an operand of 2 GiB or more: ASR_ERR_UNSUPPORTED before any launch, with
 *   nothing written (asr_ctc_align_ws_bytes is then 0).
 * asr_ctc_align_limits: frames per backtrace chunk, and the frames whose
 *   backpointer words stay in LDS (later frames' words pass through the
 *   workspace). */
size_t asr_ctc_align_ws_bytes(int T, int B, int V, int max_label_len);
int asr_ctc_align(const float* logits, long long stride_t, long long stride_b, int T, int B, int V,
                  const int32_t* labels_flat, const int32_t* label_lens, const int32_t* act_lens,
                  int max_label_len, int blank, int normalize,
                  int32_t* ali, int32_t* starts, int32_t* ends, float* scores,
                  void* workspace, size_t ws_bytes, void* stream);
int asr_ctc_align_limits(int* chunk_frames, int* lds_frames);

/* ------------------------------------------------------ hypothesis scoring
 * asr_edit_distance: per utterance pair the edit distance between a decoded
 *   hypothesis and its transcript with the substitution / insertion / deletion
 *   counts of the reference's backtrace (utils/evaluation/edit_distance.py:
 *   53-126), after the token-level form of the recipes' text clean-up.  One
 *   launch on `stream`, integers only (bitwise reproducible), no allocation,
 *   no host synchronisation, no library state.
 *   hyp: int32 (int64 with opts->hyp_i64) [B][ld_hyp], ref: int32 [B][ld_ref];
 *   hyp_lens / ref_lens int32 [B] are clipped to [0, max_hyp] / [0, max_ref],
 *   and max_hyp <= ld_hyp, max_ref <= ld_ref.  out int32 [B][5] = {distance,
 *   sub, ins, del, ref_units}; totals (nullable) int64 [5] += the column sums
 *   (64-bit atomics: zero it once, read it once per evaluation).
 *   Clean-up, in this order, of both sequences:
 *     1. hypothesis only: cut before the first opts->eos (-1: no cut); entries
 *        at or past the length and negative entries are not part of a sequence;
 *     2. opts->map (nullable, int32 [map_len] on the device): token -> token,
 *        a negative value deletes the token; tokens >= map_len pass unchanged;
 *     3. opts->space >= 0: runs of the separator collapse to one, a leading
 *        and a trailing separator go;
 *     4. ASR_ED_WORD: the units are the maximal runs of non-separator tokens,
 *        equal iff their token sequences are (a hash match is confirmed token
 *        by token).  An empty sequence has ZERO units (Python's ''.split('_')
 *        gives one empty word; deliberate);
 *     5. ASR_ED_TOKEN: the units are the tokens left, separators included.
 *   Table: d[i][0] = i, d[0][j] = j, d[i][j] = d[i-1][j-1] on a match, else
 *   1 + min(diagonal, left, up).  Counts: the walk from (ref, hyp) to (0, 0)
 *   that at each cell prefers correct (units match), then insertion (d[x][y]
 *   == d[x][y-1] + 1), then substitution (d[x][y] == d[x-1][y-1] + 1), then
 *   deletion; at x == 0 only insertions, at y == 0 only deletions.
 *   ASR_ERR_UNSUPPORTED (nothing launched, asr_last_error says why): max_ref or
 *   max_hyp above 4095, or an operand of 2 GiB or more.  ASR_ERR_ARG:
 *   ASR_ED_WORD without a separator, a null pointer, a bad shape.
 *   ASR_ERR_WORKSPACE: less than asr_edit_distance_ws_bytes(B, max_ref,
 *   max_hyp), which is 0 for a refused shape; the workspace (the backtrace's
 *   2-bit move codes when max_ref * ceil(max_hyp / 16) words exceed the 16 KB
 *   kept in LDS) needs no initialisation.
 */
#define ASR_ED_TOKEN 0
#define ASR_ED_WORD 1
typedef struct {
  int unit;            /* ASR_ED_TOKEN | ASR_ED_WORD */
  int eos;             /* hypothesis is cut before its first eos; -1: no cut */
  int space;           /* separator token; -1: none (required >= 0 for ASR_ED_WORD) */
  const int32_t* map;  /* nullable LUT [map_len]: token -> token, or -1 = delete the token */
  int map_len;         /* tokens outside [0, map_len) pass unchanged */
  int hyp_i64;         /* hyp tokens are int64 (attention decoders) instead of int32 */
} asr_edit_opts_t;
size_t asr_edit_distance_ws_bytes(int B, int max_ref, int max_hyp);
int asr_edit_distance(const void* hyp, long long ld_hyp, const int32_t* hyp_lens,
                      const int32_t* ref, long long ld_ref, const int32_t* ref_lens, int B,
                      int max_ref, int max_hyp, const asr_edit_opts_t* opts,
                      int32_t* out /* [B][5] */, long long* totals /* [5], += , nullable */,
                      void* workspace, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------- losses
 * Fused softmax cross-entropy + uniform label smoothing over rows of V logits
 * (attention_seq2seq.py:588-601, criterion.py:51-80, ctc.py:329-337):
 *   loss = ce_scale * sum_{r: tgt[r]>=0} (lse_r - x[r,tgt[r]])
 *        + ls_scale * sum_{r in LS rows} -(1/V) sum_v (x[r,v] - lse_r)
 * LS rows: r = b*T + t with t < lens[b] if lens != NULL, else tgt[r] >= 0.
 * targets int64 (nullable), -1 = ignore (any negative value is); a target
 * >= V is NOT an error: it is clamped to V - 1, in forward and backward alike
 * (tests/test_aux_kernels_gpu.py pins this).  workspace keeps the row lse for
 * backward (asr_xent_workspace_bytes(R)).  Backward writes
 * dlogits = scale * (*grad_scale) * dloss/dlogits.
 */
size_t asr_xent_workspace_bytes(int R);
int asr_xent_forward(const float* logits, int R, int V, int T, const long long* targets,
                     const int32_t* lens, float ce_scale, float ls_scale, float* loss_out,
                     void* workspace, size_t ws_bytes, void* stream);
int asr_xent_backward(const float* logits, int R, int V, int T, const long long* targets,
                      const int32_t* lens, float ce_scale, float ls_scale,
                      const float* grad_scale, float scale, float* dlogits,
                      const void* workspace, size_t ws_bytes, void* stream);
int asr_softmax(const float* x, int R, int V, float* y, void* stream);

/* ---------------------------------------------------- attention decoder
 * Teacher-forced decoder loop of AttentionSeq2seq._decode_train
 * (attention_seq2seq.py:704-799; bahdanau order, 1-layer LSTMCell decoder
 * rnn_decoder.py:63-113, location attention attention_layer.py:74-251, 1 head).
 * Dims: B utterances, T encoder frames, E encoder width, A attention dim,
 * C conv channels, K conv width (odd), D decoder units, S decoder steps (L+1).
 * Inputs: enc [B][T][E], enc_a [B][T][A] (= W_enc enc + b), lens [B] (the
 *   multiplicative energy mask, :216-225), w_ih_ctx = &W_ih[0][emb] with row
 *   stride ld_ih (the context columns of the decoder LSTMCell W_ih), w_hh
 *   [4D][D], w_dec [A][D], w_conv [A][C], conv_w [C][K], v [A],
 *   pre_emb [B][S][4D] (= emb(y_in) W_ih_emb^T + b_ih + b_hh, one GEMM for all
 *   steps), h0 [B][D] (nullable = zeros; init_dec_state).
 * Forward outputs (all saved for backward): dec [B][S][D] (dec_out_t; t=0:
 *   h0), c [B][S][D], gates [B][S][4D], x [B][S][E+D] (= [ctx_{t-1}; h_{t-1}]),
 *   ctx [B][S][E], aw [B][S][T].
 * Backward inputs: d_dec_in [B][S][D], d_ctx_in [B][S][E] (from the hoisted
 *   W_d / W_c GEMMs).  Outputs: gates_dg (dgates over the saved gates; feeds
 *   dW_ih, dW_hh, db and the embedding gradient), dctx_tot [B][S][E] (feeds
 *   d enc = aw^T dctx_tot), d_enc_a [B][T][A], d_h0 [B][D] (nullable),
 *   dwd_all [B][S][A] (dW_dec = dwd^T dec), per-(utterance, frame chunk)
 *   partials summed over the steps dv_part [B][NC][A], dwc_part [B][NC][A*C],
 *   dcw_part [B][NC][C*K] with NC = asr_attdec_chunks(dims) (column sums give
 *   dV, dW_conv, d conv kernel; fixed summation order, deterministic).
 */
typedef struct {
  int B, T, E, A, C, K, D, S;
  float sharpening;
  int sigmoid_smoothing;
} asr_attdec_dims_t;

/* Training-mode options of the decoder loop (NULL = none of them).
 * dropout_hidden: RNNDecoder dropout on h after the LSTMCell
 *   (rnn_decoder.py:97-98); the dropped h is both dec_out and the recurrent
 *   state.  Mask of element (b, t, j): asr dropout RNG, seed_hidden, index
 *   (b*S + t)*D + j (regenerated in backward).
 * Scheduled sampling (attention_seq2seq.py:744-748): ss_steps_host[t] != 0
 *   (host memory, [S], t >= 1) feeds step t with embed(argmax logits_{t-1})
 *   instead of the teacher token, where logits_{t-1} = fc(tanh(drop_d(W_d
 *   dec_{t-1} + b_d) + drop_c(W_c ctx_{t-1} + b_c))) -- the same logits the loss
 *   sees when the caller applies its post-loop dropouts with seed_d / seed_c
 *   over [B][S][Dz] (index (b*S + t)*Dz + k).  The sampled embedding (row of
 *   emb_w [V][Y], or column of emb_w [Y][V] when emb_trans) is dropped with
 *   drop_emb / seed_emb (index (b*S + t)*Y + y), written to emb_ss [B][S][Y]
 *   (caller zeroes it; teacher steps stay 0) and projected:
 *   pre_ss[b,t] = W_ih[:, :Y] e + b_ih + b_hh (w_ih_emb row stride ld_ih).
 *   tok_ss [B][S] (nullable) receives the sampled tokens.  In backward,
 *   d_pre [B][S][4D] = dG with sampled steps zeroed (the gradient of pre_emb)
 *   and dg_ss [B][S][4D] = dG at sampled steps only (for W_ih[:, :Y] and the
 *   biases through emb_ss); both NULL when no step is sampled.
 * conv_feat (NULL = off): a persistent forward pass keeps the conv features of
 *   every decoder step here and a persistent backward pass reads them back
 *   instead of recomputing them from aw; the buffer holds
 *   asr_attdec_conv_feat_bytes(dims) bytes.  A backward may only be given the
 *   buffer of a forward that ran persistent (asr_attdec_persist_last). */
typedef struct {
  float dropout_hidden;
  unsigned long long seed_hidden;
  const int32_t* ss_steps_host;
  int Y, Dz, V;
  const float* w_d;
  const float* b_d;
  float drop_d;
  unsigned long long seed_d;
  const float* w_c;
  const float* b_c;
  float drop_c;
  unsigned long long seed_c;
  const float* w_fc;
  const float* b_fc;
  const float* emb_w;
  int emb_trans;
  float drop_emb;
  unsigned long long seed_emb;
  const float* w_ih_emb;
  long long ld_ih;
  const float* b_ih;
  const float* b_hh;
  float* pre_ss;
  float* emb_ss;
  long long* tok_ss;
  float* d_pre;
  float* dg_ss;
  float* conv_feat;
} asr_attdec_opts_t;

/* Diagnostics: phase stamps (s_memrealtime ticks, 100 MHz) of the per-step
 * attention kernels' work-group (0, 0) at decoder step 10 of the last pass;
 * host must hold 64 values. */
int asr_att_trace_read(unsigned long long* host);
size_t asr_attdec_workspace_bytes(const asr_attdec_dims_t* dims, int compute_dtype,
                                  int backward);
int asr_attdec_chunks(const asr_attdec_dims_t* dims);
int asr_attdec_forward(const asr_attdec_dims_t* dims, int compute_dtype, const float* enc,
                       const float* enc_a, const int32_t* lens, const float* w_ih_ctx,
                       long long ld_ih, const float* w_hh, const float* w_dec,
                       const float* w_conv, const float* conv_w, const float* v,
                       const float* pre_emb, const float* h0, float* dec, float* c, float* gates,
                       float* x, float* ctx, float* aw, void* workspace, size_t ws_bytes,
                       void* stream);
int asr_attdec_backward(const asr_attdec_dims_t* dims, int compute_dtype, const float* enc,
                        const float* enc_a, const int32_t* lens, const float* w_ih_ctx,
                        long long ld_ih, const float* w_hh, const float* w_dec,
                        const float* w_conv, const float* conv_w, const float* v,
                        const float* dec, const float* c, const float* aw,
                        const float* d_dec_in, const float* d_ctx_in, float* gates_dg,
                        float* dctx_tot, float* d_enc_a, float* d_h0, float* dwd_all,
                        float* dv_part, float* dwc_part, float* dcw_part, void* workspace,
                        size_t ws_bytes, void* stream);
/* The same two calls with training-mode options (asr_attdec_opts_t above). */
int asr_attdec_forward_ex(const asr_attdec_dims_t* dims, const asr_attdec_opts_t* opts,
                          int compute_dtype, const float* enc, const float* enc_a,
                          const int32_t* lens, const float* w_ih_ctx, long long ld_ih,
                          const float* w_hh, const float* w_dec, const float* w_conv,
                          const float* conv_w, const float* v, const float* pre_emb,
                          const float* h0, float* dec, float* c, float* gates, float* x,
                          float* ctx, float* aw, void* workspace, size_t ws_bytes, void* stream);
/* One location-attention step as a standalone op (AttentionMechanism.forward,
 * attention_layer.py:123-251; the layer boundary of SURVEY §8(b)); the same
 * kernels as the decoder loop.  dims->S is ignored.  Forward: conv of aw_prev
 * [B][T], energies from enc_a [B][T][A] + W_dec dec_out [B][D] + W_conv f,
 * multiplicative length mask, sharpening, softmax / sigmoid -> aw_out [B][T],
 * ctx_out [B][E] = aw_out . enc.  Backward (cotangents d_ctx [B][E],
 * d_aw_out [B][T] nullable): d_enc_a, d_dec, d_aw_prev, dctx_tot, dwd (d of
 * W_dec dec_out) written; dv_part / dwc_part / dcw_part hold
 * B * asr_attdec_chunks rows whose column sums are dV, dW_conv and the
 * conv-kernel gradient.  The caller forms dW_dec = dwd^T dec_out and
 * d enc = aw_out^T dctx_tot. */
size_t asr_att_step_workspace_bytes(const asr_attdec_dims_t* dims);
int asr_att_step_forward(const asr_attdec_dims_t* dims, const float* enc, const float* enc_a,
                         const int32_t* lens, const float* w_dec, const float* w_conv,
                         const float* conv_w, const float* v, const float* dec_out,
                         const float* aw_prev, float* ctx_out, float* aw_out, void* workspace,
                         size_t ws_bytes, void* stream);
int asr_att_step_backward(const asr_attdec_dims_t* dims, const float* enc, const float* enc_a,
                          const int32_t* lens, const float* w_dec, const float* w_conv,
                          const float* conv_w, const float* v, const float* dec_out,
                          const float* aw_prev, const float* aw_out, const float* d_ctx,
                          const float* d_aw_out, float* d_enc_a, float* d_dec, float* d_aw_prev,
                          float* dctx_tot, float* dwd, float* dv_part, float* dwc_part,
                          float* dcw_part, void* workspace, size_t ws_bytes, void* stream);

/* Multi-head attention step (csrc/att_heads.hip): AttentionMechanism.forward
 * (attention_layer.py:141-251) for H >= 1 heads of additive (location, or
 * content with C = 0) or dot-product energies, all heads in one launch.  f32
 * arithmetic whatever the compute mode.
 * Dims as above; A is the width of enc_a (dot: A = D, C = 0; K is ignored when
 * C = 0).  Layouts: enc [B][T][E]; enc_a HEAD-MAJOR [H][B][T][A] (each head's
 * W_enc GEMM writes its own slice); dec_out [B][D]; aw_prev / aw_out / d_aw_out
 * / d_aw_prev [B][H][T]; ctx_out / d_ctx / dctx_tot [B][H][E] (= [B][H*E], the
 * head-major concatenation torch.cat(..., -1) gives).  Per-head weights by
 * pointer: w_dec[h] [A][D], w_conv[h] [A][C], conv_w[h] [C][K], v[h] [A]
 * (all unused for dot).
 * Forward: per head conv of aw_prev, energies V.tanh(enc_a + W_dec dec_out +
 * W_conv f) or enc_a . dec_out, multiplicative length mask, sharpening,
 * softmax over all T frames / sigmoid, context.
 * Backward (cotangents d_ctx, d_aw_out nullable), all written, none
 * accumulated: d_enc_a [H][B][T][A]; d_dec [B][D], summed over the heads in
 * the order h = 0 .. H-1 by one owner thread per element (no atomics: run to
 * run bitwise); d_aw_prev (zero for C = 0 and dot); dctx_tot (= d_ctx; the
 * caller forms d enc[b] = aw_out[b]^T dctx_tot[b], one product with K = H);
 * additive only: dwd [H][B][A] (dW_dec_h = dwd_h^T dec_out) and the partial
 * rows dv_part [H][B][A], dwc_part [H][B][A*C], dcw_part [H][B][C*K] whose
 * column sums over B are dV_h, dW_conv_h and head h's conv-kernel gradient.
 * asr_att_heads_workspace_bytes(p, backward): bytes the call needs (the
 * backward's conv features; 0 for the forward, and 0 for a refused shape).
 * ASR_ERR_UNSUPPORTED (nothing launched, asr_last_error says why): H >
 * ASR_ATT_HEADS_MAX, C > ASR_ATT_HEADS_MAX_C, an even K, B > 65535, any
 * operand or output of 2 GiB or more, or an LDS need over 64 KiB (forward
 * about 4 (2 T + 2 A + A C + C K + K + 64 C) bytes, backward about
 * 4 (2 T + E + D + 3 A + A C + C K + K)); forward and backward refuse the
 * same shapes. */
#define ASR_ATT_HEADS_MAX 8
#define ASR_ATT_HEADS_MAX_C 16
#define ASR_ATT_HEADS_ADDITIVE 0
#define ASR_ATT_HEADS_DOT 1
typedef struct {
  int B, T, E, A, C, K, D, H;
  int kind;
  float sharpening;
  int sigmoid_smoothing;
  const float* w_dec[ASR_ATT_HEADS_MAX];
  const float* w_conv[ASR_ATT_HEADS_MAX];
  const float* conv_w[ASR_ATT_HEADS_MAX];
  const float* v[ASR_ATT_HEADS_MAX];
} asr_att_heads_t;
size_t asr_att_heads_workspace_bytes(const asr_att_heads_t* p, int backward);
int asr_att_heads_forward(const asr_att_heads_t* p, const float* enc, const float* enc_a,
                          const int32_t* lens, const float* dec_out, const float* aw_prev,
                          float* ctx_out, float* aw_out, void* workspace, size_t ws_bytes,
                          void* stream);
int asr_att_heads_backward(const asr_att_heads_t* p, const float* enc, const float* enc_a,
                           const int32_t* lens, const float* dec_out, const float* aw_prev,
                           const float* aw_out, const float* d_ctx, const float* d_aw_out,
                           float* d_enc_a, float* d_dec, float* d_aw_prev, float* dctx_tot,
                           float* dwd, float* dv_part, float* dwc_part, float* dcw_part,
                           void* workspace, size_t ws_bytes, void* stream);

/* Attention beam search on the device (AttentionSeq2seq._decode_infer_beam,
 * attention_seq2seq.py:1038-1237; csrc/att_beam.hip states the semantics) for
 * bahdanau order, a one-layer LSTMCell or GRUCell decoder without residual,
 * location or content attention.  f32 arithmetic whatever the compute mode.
 * dims as above (T = the padded frame count, S ignored); every utterance
 * decodes over its own lens[b] frames (clipped to [0, T]; 0 frames: empty
 * hypothesis).
 * opts: W beam width, V classes, Y embedding width, Dz bottleneck width,
 *   max_len / min_len (min_decode_len counts <sos>), eos, length_penalty
 *   (added in double), the decoder weights: w_ih [4D][ld_ih] (columns [0, Y)
 *   embedding, [Y, Y + E) context), w_hh [4D][D], b_ih / b_hh [4D], w_dec
 *   [A][D], w_conv [A][C], conv_w [C][K], v [A], w_d [Dz][D], w_c [Dz][E],
 *   w_fc [V][Dz] (b_d, b_c, b_fc nullable), emb_w [V][Y] ([Y][V] if emb_trans).
 * enc [B][T][E], enc_a [B][T][A] (= W_enc enc + b), h0 [B][D] (nullable).
 * Outputs: tokens int64 [B][max_len] (hyp_lens[b] valid, -1 after; the final
 *   <eos> included when the hypothesis completed), hyp_lens int32 [B], scores
 *   double [B], aw float [B][max_len][T] (row s = the weights of step s along
 *   the hypothesis' parent rows; zero past hyp_lens[b] rows and lens[b] frames).
 * Plain launches on `stream` in a fixed order, 4 per step; no allocation, no
 * host synchronisation.  The workspace (asr_att_beam_ws_bytes; 256-B aligned,
 * no initialisation) holds the per-step attention record [max_len][B*W][T]
 * and the logits [B*W][V]; utterances read enc in place.
 * ASR_ERR_ARG before any launch: a null pointer, eos outside [0, V), ld_ih <
 *   Y + E, max_len <= 0, an even conv width, and the optional parts' below.
 * ASR_ERR_UNSUPPORTED (nothing launched, asr_last_error says why): W outside
 *   [2, 32], C > 16, or a kernel's LDS need above 64 KiB (attention: D + 2A +
 *   C K + A C + 2T + K + 63 floats); asr_att_beam_ws_bytes is 0 then.
 *
 * ex (nullable: an LSTM cell and neither optional part) chooses the cell and
 * adds the optional parts; whatever is absent costs no launch.
 *   cell: ASR_ATT_BEAM_CELL_LSTM, or ASR_ATT_BEAM_CELL_GRU for a GRUCell
 *     decoder (torch's gate rows r, z, n; r scales the hidden part of n, bias
 *     included): opts' w_ih [3D][ld_ih], w_hh [3D][D], b_ih / b_hh [3D] then
 *     hold the 3-gate tensors.  Only the cell kernel differs; launch counts,
 *     limits, workspace and output layout are the same.  Any other cell is
 *     ASR_ERR_ARG.
 *   ctc (null or weight 0: absent): the joint CTC/attention search, score =
 *     (parent + (1 - weight) lp_att(c) + weight delta_ctc(g, c)) +
 *     length_penalty.  ctc_logits f32 [B][T][Vc]: the raw logits of the CTC head
 *     over the same frames (read in place, frames t < lens[b] only); attention
 *     class c != eos is CTC class c + label_offset, which must lie in [0, Vc)
 *     and differ from blank, and weight must lie in (0, 1] (else ASR_ERR_ARG,
 *     as a null ctc_logits).  Launches: 2 once, then 7 per step (6 at step 0).
 *     Workspace: the plain one plus 2 B T floats and (4 B W T + 2 B W + 2 B W
 *     W) doubles.  The added kernels use a fixed 2 KiB of LDS and add no limit.
 *   lm (null or weight 0: absent): shallow fusion with an RNN language model,
 *     score = (parent + (1 - lambda) lp_att(c) + lambda delta_ctc + weight
 *     lp_lm(c | g)) + length_penalty, lp_lm the f32 log-softmax of the LM's
 *     output logits after the row's prefix g.  The candidates stay the min(W,
 *     V) best attention classes of each row; LM class c is attention class c,
 *     <eos> included, and <sos> is the eos index.  The LM is `layers` stacked
 *     LSTM layers (torch's gate rows i, f, g, o) over an embedding: emb [V][Y],
 *     w_ih[0] [4H][Y], w_ih[l] [4H][H] (l > 0), w_hh[l] [4H][H], b_ih[l] /
 *     b_hh[l] [4H], w_out [V][H] (tied weights: the emb pointer, H == Y), b_out
 *     [V]; its state starts at zero and steps at every t >= 0, whatever the
 *     decoder's cell.  2 more launches per step (beam_lm_cell, beam_lm_score)
 *     and a select variant in the plain one's place.  Workspace: the joint
 *     search's (whatever lambda) plus 4 B W layers H floats of LM state, B W V
 *     logits and B W W candidate terms.  ASR_ERR_ARG: lm->V != opts->V, weight
 *     < 0, a null pointer.  ASR_ERR_UNSUPPORTED (the query is 0 for the first
 *     two): layers > ASR_ATT_BEAM_LM_MAX_LAYERS, beam_lm_cell's LDS need (2
 *     max(Y, H) + H floats) above 64 KiB, lm->cell != ASR_ATT_BEAM_CELL_LSTM (a
 *     GRU LM).
 * asr_att_beam_ws_bytes reads of ex only whether ctc and lm are null and
 * lm->layers / H / Y. */
typedef struct {
  int W, V, Y, Dz, max_len, min_len, eos, emb_trans;
  double length_penalty;
  long long ld_ih;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* w_dec;
  const float* w_conv;
  const float* conv_w;
  const float* v;
  const float* w_d;
  const float* b_d;
  const float* w_c;
  const float* b_c;
  const float* w_fc;
  const float* b_fc;
  const float* emb_w;
} asr_att_beam_opts_t;
typedef struct {
  const float* ctc_logits;
  int Vc, blank, label_offset;
  double weight;
} asr_att_beam_ctc_t;
#define ASR_ATT_BEAM_CELL_LSTM 0
#define ASR_ATT_BEAM_CELL_GRU 1
#define ASR_ATT_BEAM_LM_MAX_LAYERS 4
typedef struct asr_att_beam_lm_s {
  int layers, H, Y, V;
  int cell; /* the LM's cell type: ASR_ATT_BEAM_CELL_LSTM */
  const float* emb;
  const float* w_ih[ASR_ATT_BEAM_LM_MAX_LAYERS];
  const float* w_hh[ASR_ATT_BEAM_LM_MAX_LAYERS];
  const float* b_ih[ASR_ATT_BEAM_LM_MAX_LAYERS];
  const float* b_hh[ASR_ATT_BEAM_LM_MAX_LAYERS];
  const float* w_out;
  const float* b_out;
  double weight;
} asr_att_beam_lm_t;
typedef struct {
  int cell;
  const asr_att_beam_ctc_t* ctc; /* nullable */
  const asr_att_beam_lm_t* lm;   /* nullable */
} asr_att_beam_ex_t;
size_t asr_att_beam_ws_bytes(const asr_attdec_dims_t* dims, int W, int V, int Y, int Dz,
                             int max_len, const asr_att_beam_ex_t* ex);
int asr_att_beam_decode(const asr_attdec_dims_t* dims, const asr_att_beam_opts_t* opts,
                        const asr_att_beam_ex_t* ex, const float* enc, const float* enc_a,
                        const int32_t* lens, const float* h0, void* workspace, size_t ws_bytes,
                        long long* tokens, int32_t* hyp_lens, double* scores, float* aw,
                        void* stream);

/* Test / diagnostics: the attention-step kernel instantiations the last
 * asr_attdec_forward_ex / _backward_ex launched: out4 = {forward conv-channel
 * template (10 or 3; 0 = generic), forward 32-frame chunks per utterance,
 * backward template, backward chunks}. */
int asr_attdec_last_launch(int* out4);
/* {forward, backward}: 1 if the last decoder pass of that direction ran as one
 * persistent launch (bf16, B <= 32, no scheduled sampling; ASR_ATT_PERSIST=0
 * disables it). */
int asr_attdec_persist_last(int* out2);
size_t asr_attdec_conv_feat_bytes(const asr_attdec_dims_t* dims);
int asr_attdec_backward_ex(const asr_attdec_dims_t* dims, const asr_attdec_opts_t* opts,
                           int compute_dtype, const float* enc, const float* enc_a,
                           const int32_t* lens, const float* w_ih_ctx, long long ld_ih,
                           const float* w_hh, const float* w_dec, const float* w_conv,
                           const float* conv_w, const float* v, const float* dec,
                           const float* c, const float* aw, const float* d_dec_in,
                           const float* d_ctx_in, float* gates_dg, float* dctx_tot,
                           float* d_enc_a, float* d_h0, float* dwd_all, float* dv_part,
                           float* dwc_part, float* dcw_part, void* workspace, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------- VGG front-end
 * Replaces CNNEncoder (models/pytorch_v3/encoders/cnn.py:124-165): Conv2d 3x3
 * (padding 1) -> ReLU -> MaxPool (first floor mode, later ceil) -> BatchNorm2d
 * -> Dropout per layer, input viewed [B, 1, F, T] (cnn.py:143-149), output
 * [B, T', F'*C] (cnn.py:155-157).  Layer tensors are channels-last with a zero
 * halo: [B][T+2][F+2][C] ("padded pixels").  Layers with C_in >= 16 run the
 * 3x3 convolution as one asr_gemm with tap addressing (asr_operand_t);
 * C_in = 1 (and channel counts that are not multiples of 16) use
 * asr_conv_direct_*.
 * asr_vgg_pool_dims: output extent of a pool (kernel = stride), torch's
 *   floor / ceil rules.
 * asr_vgg_block_forward / _backward: ReLU + pool + BatchNorm (training batch
 *   statistics over every (b, f, t) incl. padding frames, running stats with
 *   momentum / unbiased variance; or eval with running stats) + dropout (asr
 *   dropout RNG, index = element of [B][T'][F'][C]).  See cnn.hip. */
int asr_vgg_pad_input(const float* xs, int B, int T, int F, float* out, void* stream);
/* ... as a Cp-channel image (channel 0 = xs, the rest 0; out_dtype f32 / bf16):
 * the first conv layer on the GEMM path with its one input channel padded to 16 */
int asr_vgg_pad_input_ch(const float* xs, int B, int T, int F, int Cp, int out_dtype, void* out,
                         void* stream);
/* GEMM images of a Conv2d weight W [Co][Ci][3][3] (tap j = kw*3 + kh):
 * mode 0 out[co][j*Ci + ci] (forward B operand), mode 1 out[ci][j*Co + co]
 * (input-gradient B operand); unpack_acc: dW [Co][Ci][3][3] += [Co][9 Ci]. */
int asr_conv_weight_pack(const float* w, int Co, int Ci, int mode, int out_dtype, void* out,
                         void* stream);
int asr_conv_weight_unpack_acc(const float* packed, int Co, int Ci, float* dw, void* stream);
/* mode-0 image / unpack with an input-channel pitch Cip >= Ci (padded channels
 * stay as the caller zeroed them) */
int asr_conv_weight_pack_pad(const float* w, int Co, int Ci, int Cip, int mode, int out_dtype,
                             void* out, void* stream);
/* The same from the transposed image packed_t [9 Cip][Co] (the weight
 * gradient computed as X^T dZ, so that C_out is the product's narrow N). */
int asr_conv_weight_unpack_acc_pad_t(const float* packed_t, int Co, int Ci, int Cip, float* dw,
                                     void* stream);
int asr_conv_weight_unpack_acc_pad(const float* packed, int Co, int Ci, int Cip, float* dw,
                                   void* stream);
/* Direct 3x3 convolution (layers the tap-addressed GEMM cannot take: C_in = 1,
 * channel counts not multiples of 16): x [padded pixels][Ci] f32, w the torch
 * weight [Co][Ci][3][3]; z / dx over valid pixels; dw / dbias accumulate. */
int asr_conv_direct_forward(const float* x, int B, int T, int F, int Ci, int Co, const float* w,
                            const float* bias, float* z, void* stream);
/* Single-input-channel 3x3 convolution forward (the first VGG layer) from
 * channel 0 of a padded operand x [B][T+2][F+2][cstride] (x_dtype ASR_DT_F32
 * or ASR_DT_BF16, e.g. the GEMM path's 16-channel bf16 staging): z
 * [B][T+2][F+2][Co] f32 at valid pixels (+ bias); Co % 4 == 0, Co <= 512.
 * Same sum as asr_conv_direct_forward with Ci = 1 (CNNEncoder's first Conv2d,
 * cnn.py:124-165). */
int asr_conv3x3_c1_forward(const void* x, int x_dtype, int cstride, int B, int T, int F, int Co,
                           const float* w, const float* bias, float* z, void* stream);
/* asr_conv3x3_c1_forward reading the raw features xs [B][T][F] f32 (the first
 * VGG layer, encoders/cnn.py:124-165), each value rounded to bf16 first when
 * round_bf16 (the bf16 operand's values); Co / 4 must divide 256. */
int asr_conv3x3_c1_forward_xs(const float* xs, int round_bf16, int B, int T, int F, int Co,
                              const float* w, const float* bias, void* z, int z_dtype,
                              void* stream);
/* 3x3 convolution of a zero-haloed channels-last bf16 operand, tap-resident
 * (csrc/conv.hip; replaces the tap-addressed asr_gemm product of the VGG
 * convolutions, encoders/cnn.py:124-165 Conv2d 3x3 padding 1):
 *   out[p][n] = bias[n] + sum_{tap < 9} sum_{c < Cin} in[p + s(tap)][c] * w[n][tap Cin + c],
 *   s(tap) = sign * ((tap / 3 - 1) * Fp + (tap % 3 - 1)), rows outside [0, P) zero,
 * for every padded pixel row p < P (Fp = F + 2: the grid's row pitch).  in bf16
 * [P][Cin], w bf16 [Cout][9 Cin] (asr_conv_weight_pack_pad / _pack images),
 * bias f32 [Cout] or NULL, out [P][Cout] f32 or bf16 (out_dtype).  sign = 1:
 * the forward; sign = -1 with the mirrored weight image: the input gradient.
 * The f32 sums are asr_gemm's (same k order).  Cin, Cout in {64, 128};
 * ASR_ERR_UNSUPPORTED otherwise (asr_conv3x3_tr_supported says which). */
int asr_conv3x3_tr_supported(int Cin, int Cout, int Fp);
/* The plan asr_conv3x3_tr launches with (host only, no GPU): out = {wpx (pixels
 * per wave; a tile is 4 wpx pixel rows), nw (weight-ring slots, 0 = the whole
 * weight image resident in LDS), RC (pixel rows of the LDS input ring), LDS
 * bytes}; returns 1, or 0 where asr_conv3x3_tr_supported is 0.  The plan only
 * names (Cin, Cout, wpx, nw) combinations asr_conv3x3_tr_has_kernel reports,
 * the list the launcher dispatches over.  asr_conv3x3_tr_wgrad_plan: the same
 * for asr_conv3x3_tr_wgrad, out = {RC, LDS bytes}. */
int asr_conv3x3_tr_plan(int Cin, int Cout, int Fp, int out[4]);
int asr_conv3x3_tr_has_kernel(int Cin, int Cout, int wpx, int nw);
int asr_conv3x3_tr_wgrad_plan(int Cin, int Cout, int Fp, int out[2]);
int asr_conv3x3_tr(const void* in, long long P, int Cin, int Fp, int sign, const void* w,
                   int Cout, const float* bias, void* out, int out_dtype, void* stream);
/* Weight-gradient image of the same convolution (csrc/conv.hip, replaces the
 * dz^T X tap GEMM): packed[n][tap Cin + c] = sum_p dz[p][n] * x[p + s(tap)][c]
 * (sign +1), overwritten, f32 [Cout][9 Cin] -- the image
 * asr_conv_weight_unpack_acc_pad accumulates into the Conv2d weight gradient.
 * x bf16 [P][Cin], dz bf16 [P][Cout]; per-chunk partials in the workspace
 * (asr_conv3x3_tr_wgrad_workspace_bytes, 0 = shape not supported), summed in a
 * fixed order (deterministic).  Cin, Cout in {64, 128}. */
/* Weight-gradient image of the first VGG layer (one input channel) straight
 * from the raw features xs [B][T][F] f32 (rounded to bf16 when round_bf16):
 * packed [Co][9 Cip] f32 (overwritten) = the tap GEMM's dz^T X image over the
 * Cip-channel padded operand whose channel 0 holds xs (channels >= 1 zero);
 * dz bf16 [B (T+2) (F+2)][Co].  Co = 64; workspace
 * asr_conv3x3_c1_wgrad_workspace_bytes(Co). */
size_t asr_conv3x3_c1_wgrad_workspace_bytes(int Co);
int asr_conv3x3_c1_wgrad_xs(const float* xs, int round_bf16, int B, int T, int F, int Co,
                            const void* dz, int Cip, float* packed, void* ws, size_t ws_bytes,
                            void* stream);
/* Zero the one-pixel halo (rows t = 0, T + 1 and columns f = 0, F + 1) of a
 * channels-last padded grid [B][T+2][F+2][C] of dtype (ASR_DT_F32 / _BF16;
 * C * size % 16 == 0): the producers of the VGG layer operands write only the
 * interior, so the buffer need not be zero-filled whole. */
int asr_vgg_zero_halo(void* buf, int dtype, int B, int T, int F, int C, void* stream);
size_t asr_conv3x3_tr_wgrad_workspace_bytes(long long P, int Cin, int Cout, int Fp);
int asr_conv3x3_tr_wgrad(const void* x, const void* dz, long long P, int Cin, int Fp, int Cout,
                         float* packed, void* ws, size_t ws_bytes, void* stream);
int asr_conv_direct_dgrad(const float* dz, int B, int T, int F, int Ci, int Co, const float* w,
                          float* dx, void* stream);
size_t asr_conv_direct_wgrad_workspace_bytes(int B, int T, int F, int Ci, int Co);
int asr_conv_direct_wgrad(const float* x, const float* dz, int B, int T, int F, int Ci, int Co,
                          float* dw, float* dbias, void* workspace, size_t ws_bytes,
                          void* stream);
int asr_vgg_accumulate(const float* a, float* dst, int n, const float* a2, float* dst2, int n2,
                       void* stream);
int asr_vgg_pool_dims(int T, int F, int pt, int pf, int ceil_mode, int* To, int* Fo);
size_t asr_vgg_block_workspace_bytes(int B, int To, int Fo, int C);
int asr_vgg_block_forward(const float* z, int B, int T, int F, int C, int pt, int pf,
                          int ceil_mode, float* P, uint8_t* slot, const float* gamma,
                          const float* beta, float* run_mean, float* run_var, int training,
                          float momentum, float eps, float* bn_mean, float* bn_rstd, float drop,
                          unsigned long long seed, void* out, int out_dtype, int flat,
                          void* workspace, size_t ws_bytes, void* stream);
int asr_vgg_block_backward(const float* dnext, int flat, const float* z, int B, int T, int F,
                           int C, int pt, int pf, int ceil_mode, const float* P,
                           const uint8_t* slot, const float* gamma, const float* bn_mean,
                           const float* bn_rstd, float* dgamma, float* dbeta, float drop,
                           unsigned long long seed, void* dz, int dz_dtype, void* workspace,
                           size_t ws_bytes, void* stream);
/* ... and dbias (nullable) += the conv bias gradient (per-channel sum of the
 * f32 dZ values, fixed order), so dZ can be stored as a bf16 GEMM operand. */
int asr_vgg_block_backward_ex(const float* dnext, int flat, const float* z, int B, int T, int F,
                              int C, int pt, int pf, int ceil_mode, const float* P,
                              const uint8_t* slot, const float* gamma, const float* bn_mean,
                              const float* bn_rstd, float* dgamma, float* dbeta, float drop,
                              unsigned long long seed, void* dz, int dz_dtype, float* dbias,
                              void* workspace, size_t ws_bytes, void* stream);
/* asr_vgg_block_forward / asr_vgg_block_backward_ex with the conv output z of
 * dtype z_dtype (ASR_DT_F32 or ASR_DT_BF16, C % 4 == 0): in bf16 mode the
 * convolution GEMMs write z as bf16 (asr_gemm_t.c_dtype), halving its
 * write and its two reads (ReLU + pool forward, ReLU mask backward). */
int asr_vgg_block_forward_z(const void* z, int z_dtype, int B, int T, int F, int C, int pt,
                            int pf, int ceil_mode, float* P, uint8_t* slot, const float* gamma,
                            const float* beta, float* run_mean, float* run_var, int training,
                            float momentum, float eps, float* bn_mean, float* bn_rstd, float drop,
                            unsigned long long seed, void* out, int out_dtype, int flat,
                            void* workspace, size_t ws_bytes, void* stream);
int asr_vgg_block_backward_z(const float* dnext, int flat, const void* z, int z_dtype, int B,
                             int T, int F, int C, int pt, int pf, int ceil_mode, const float* P,
                             const uint8_t* slot, const float* gamma, const float* bn_mean,
                             const float* bn_rstd, float* dgamma, float* dbeta, float drop,
                             unsigned long long seed, void* dz, int dz_dtype, float* dbias,
                             void* workspace, size_t ws_bytes, void* stream);
/* asr_vgg_block_backward_z with the incoming gradient's dtype: dnext_dtype
 * ASR_DT_BF16 (C % 4 == 0, bf16 z and dz, full-resolution pass) reads a bf16
 * dnext (the input-gradient convolution of the layer above writes it so). */
int asr_vgg_block_backward_zd(const void* dnext, int dnext_dtype, int flat, const void* z,
                              int z_dtype, int B, int T, int F, int C, int pt, int pf,
                              int ceil_mode, const float* P, const uint8_t* slot,
                              const float* gamma, const float* bn_mean, const float* bn_rstd,
                              float* dgamma, float* dbeta, float drop, unsigned long long seed,
                              void* dz, int dz_dtype, float* dbias, void* workspace,
                              size_t ws_bytes, void* stream);
/* The two above with the pooled-value store P of dtype p_dtype: ASR_DT_BF16
 * (bf16 z, C % 4 == 0, P 8-B aligned) stores P = max(0, max z) as bf16 --
 * exact, since every candidate is a bf16 value -- halving P's write and its
 * four reads (BN moments, BN apply, BN backward moments, ReLU mask). */
int asr_vgg_block_forward_zp(const void* z, int z_dtype, int B, int T, int F, int C, int pt,
                             int pf, int ceil_mode, void* P, int p_dtype, uint8_t* slot,
                             const float* gamma, const float* beta, float* run_mean,
                             float* run_var, int training, float momentum, float eps,
                             float* bn_mean, float* bn_rstd, float drop, unsigned long long seed,
                             void* out, int out_dtype, int flat, void* workspace,
                             size_t ws_bytes, void* stream);
int asr_vgg_block_backward_zdp(const void* dnext, int dnext_dtype, int flat, const void* z,
                               int z_dtype, int B, int T, int F, int C, int pt, int pf,
                               int ceil_mode, const void* P, int p_dtype, const uint8_t* slot,
                               const float* gamma, const float* bn_mean, const float* bn_rstd,
                               float* dgamma, float* dbeta, float drop, unsigned long long seed,
                               void* dz, int dz_dtype, float* dbias, void* workspace,
                               size_t ws_bytes, void* stream);
/* The first VGG layer (one input channel, stencil from the raw features as
 * asr_conv3x3_c1_forward_xs) when it is unpooled and followed by batch norm:
 * writes P = max(0, bf16(z)) [B][T][F][Co] bf16 directly -- the value the
 * ReLU pass would store -- and, with mpart / qpart, per-block partial sums of
 * P - shift and its square ([asr_vgg_c1_relu_p_blocks(B, T)][Co] each; shift =
 * the running mean), so no conv output z is written or read back
 * (cnn.py:124-165's Conv2d -> ReLU -> BatchNorm2d of layer 0). */
int asr_vgg_c1_relu_p_blocks(int B, int T);
int asr_vgg_c1_forward_relu_p(const float* xs, int round_bf16, int B, int T, int F, int Co,
                              const float* w, const float* bias, uint16_t* P, const float* shift,
                              float* mpart, float* qpart, void* stream);
/* asr_vgg_block_forward_zp from that P and its partials: batch statistics
 * (training) or running statistics, the running-stat update, and the next
 * layer's input (bf16 padded rows, or flat f32).  workspace >= C floats. */
int asr_vgg_block_forward_given_p(const uint16_t* P, int B, int T, int F, int C,
                                  const float* gamma, const float* beta, float* run_mean,
                                  float* run_var, int training, float momentum, float eps,
                                  float* bn_mean, float* bn_rstd, float drop,
                                  unsigned long long seed, void* out, int out_dtype, int flat,
                                  const float* mpart, const float* qpart, int nblk,
                                  void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------- kf x kt convolutions (pure-CNN encoder)
 * Replaces the Conv2d of CNNEncoder layers whose kernel is not 3x3
 * (encoders/cnn.py:68-73: kernel_size = (kf, kt) over [B, C, freq, time],
 * stride 1, padding 1), kf, kt in {3, 5}; csrc/conv_taps.hip.  Operands use the
 * VGG front-end's layout: channels-last with a one-pixel zero halo,
 * x [B][T+2][F+2][Cin].  The output grid is To x Fo = (T + 3 - kt) x (F + 3 - kf)
 * valid pixels, written to the interior of z [B][To+2][Fo+2][Cout] f32 (the
 * caller zeroes the halo, asr_vgg_zero_halo): input and output rows have their
 * own pitches.  Tap index = dt * kf + df (time-major).  compute_dtype
 * ASR_DT_BF16: bf16 operands, bf16 MFMA, f32 sums; Cin, Cout multiples of 16 up
 * to 256.  ASR_DT_F32: f32 operands, exact f32 products and sums in k order;
 * Cout % 8 == 0.  A shape a kernel does not take returns ASR_ERR_UNSUPPORTED
 * before any launch (asr_last_error says why).
 * asr_conv_taps_supported: 1 when forward, input gradient and weight gradient
 *   all take the shape (T, F = the layer input's valid extents).
 * asr_conv_taps_forward: z(to, fo)[n] = bias[n] + sum_{dt, df, c}
 *   x_p(to + dt, fo + df)[c] * w[n][(dt kf + df) Cin + c]; w = the mode-0 image
 *   [Cout][kf kt Cin] of asr_conv_taps_weight_pack, bias f32 [Cout] or NULL.
 * asr_conv_taps_dgrad (autograd of that Conv2d w.r.t. its input): dx interior
 *   [B][T+2][F+2][Cin] f32 from dz [B][To+2][Fo+2][Cout] (zero halo) and wt =
 *   the mode-1 image [Cin][kf kt Cout] (mirrored, transposed): the forward
 *   kernel with the pitches exchanged, writing a grid k - 3 larger per axis.
 * asr_conv_taps_wgrad: packed [Cout][kf kt Cin] f32 (overwritten) =
 *   sum over pixels of dz(to, fo)[n] * x_p(to + dt, fo + df)[c]; bf16 mode sums
 *   per-chunk partials from the workspace in a fixed order (two runs are
 *   bitwise equal).  asr_conv_taps_wgrad_workspace_bytes: 0 = shape not taken.
 * asr_conv_taps_weight_pack: images of the torch weight W [Co][Ci][kf][kt]:
 *   mode 0 out[co][(dt kf + df) Cip + ci] = W[co][ci][df][dt] (channels ci >= Ci
 *   of the pitch Cip written 0), mode 1 (Cip == Ci) out[ci][(dt kf + df) Co + co]
 *   = W[co][ci][kf-1-df][kt-1-dt]; out_dtype f32 / bf16.
 * asr_conv_taps_weight_unpack_acc: dW [Co][Ci][kf][kt] += the mode-0 image. */
int asr_conv_taps_supported(int compute_dtype, int B, int T, int F, int Cin, int Cout, int kf,
                            int kt);
int asr_conv_taps_forward(int compute_dtype, const void* x, int B, int T, int F, int Cin,
                          const void* w, int Cout, int kf, int kt, const float* bias, float* z,
                          void* stream);
int asr_conv_taps_dgrad(int compute_dtype, const void* dz, int B, int T, int F, int Cin,
                        const void* wt, int Cout, int kf, int kt, float* dx, void* stream);
size_t asr_conv_taps_wgrad_workspace_bytes(int compute_dtype, int B, int T, int F, int Cin,
                                           int Cout, int kf, int kt);
int asr_conv_taps_wgrad(int compute_dtype, const void* x, const void* dz, int B, int T, int F,
                        int Cin, int Cout, int kf, int kt, float* packed, void* ws,
                        size_t ws_bytes, void* stream);
int asr_conv_taps_weight_pack(const float* w, int Co, int Ci, int Cip, int kf, int kt, int mode,
                              int out_dtype, void* out, void* stream);
int asr_conv_taps_weight_unpack_acc(const float* packed, int Co, int Ci, int Cip, int kf, int kt,
                                    float* dw, void* stream);
/* Activation -> MaxPool2d -> BatchNorm2d -> Dropout of a CNNEncoder layer
 * (encoders/cnn.py:78-111) with the activation given: ReLU, PReLU (cnn.py:82,
 * slope = device pointer to the one learnable slope) or hard-tanh(0, 20)
 * (cnn.py:84); csrc/cnn_act.hip.  Arguments as asr_vgg_block_forward /
 * _backward_ex (z, dz haloed f32 [B][T+2][F+2][C]; P f32 [B][To][Fo][C]; out
 * the next layer's haloed operand f32 / bf16, or flat f32; dnext f32, haloed or
 * flat).  The pool returns the maximum of the activated values present in its
 * window (they may be negative).  Backward: PReLU dz = dy where z > 0 else
 * slope * dy, *dslope += sum of dy * z over z <= 0; hard-tanh dz = dy where
 * 0 < z < 20; dbias (nullable) += per-channel sum of dz; training = the
 * forward's flag (eval: BatchNorm used the running statistics).  Every sum is
 * taken in a fixed order (two runs are bitwise equal). */
#define ASR_ACT_RELU 0
#define ASR_ACT_PRELU 1
#define ASR_ACT_HARDTANH 2
size_t asr_cnn_act_workspace_bytes(int B, int T, int F, int C);
int asr_cnn_act_forward(const float* z, int B, int T, int F, int C, int act, const float* slope,
                        int pt, int pf, int ceil_mode, float* P, uint8_t* slot,
                        const float* gamma, const float* beta, float* run_mean, float* run_var,
                        int training, float momentum, float eps, float* bn_mean, float* bn_rstd,
                        float drop, unsigned long long seed, void* out, int out_dtype, int flat,
                        void* workspace, size_t ws_bytes, void* stream);
int asr_cnn_act_backward(const float* dnext, int flat, const float* z, int B, int T, int F, int C,
                         int act, const float* slope, int pt, int pf, int ceil_mode,
                         const float* P, const uint8_t* slot, const float* gamma,
                         const float* bn_mean, const float* bn_rstd, int training, float* dgamma,
                         float* dbeta, float drop, unsigned long long seed, void* dz, int dz_dtype,
                         float* dbias, float* dslope, void* workspace, size_t ws_bytes,
                         void* stream);

/* ----------------------------------------------------------- profiling
 * Sampled HIP-event timing of the recurrence step kernels on their own stream
 * (bench.py's live roofline measurement).  asr_prof_begin(stride): bracket
 * every stride-th launch of each tracked kernel with an event pair.
 * asr_prof_end: synchronises on the recorded events (the only entry point
 * that does), fills mean_us[k] (mean launch duration, microseconds) and
 * launches[k] (all launches seen) for k = 0 lstm forward step, 1 lstm
 * backward step (per-step kernels, sampled), 2 lstm forward pass, 3 lstm
 * backward pass (persistent kernels, one launch per layer pass, all timed),
 * 4 the asr_gemm main kernel (all timed; mean_work[4] = mean algorithmic
 * flops 2*M*N*K per timed launch).  mean_work may be NULL.
 */
int asr_prof_begin(int stride);
int asr_prof_end(double* mean_us, long long* launches, double* mean_work, int nkinds);
/* Every timed sample of kind `kind` after asr_prof_end: per sample the tag
 * naming the kernel instantiation (GEMM / convolution family x 4 + operand
 * modes, the CTC vocabulary V, the persistent LSTM pass form; prof.h
 * ASR_PTAG_*), its algorithmic work and its duration in microseconds, up to
 * `max` samples.  Returns the sample count, -1 before asr_prof_end. */
long long asr_prof_samples(int kind, int* tags, double* work, double* us, long long max);

/* Status word of the persistent recurrence kernels: bit 0 set when a bounded
 * inter-work-group wait gave up (a co-residency failure; that pass's outputs
 * are invalid).  Synchronises `stream`; clear != 0 resets the word. */
int asr_lstm_persist_status(int* status, int clear, void* stream);

/* The same two status words, stream-ordered and without a host sync:
 * dst (device int32[2]) = {counter-form word, tagged-granule word}; clear != 0
 * then zeroes both.  The training step gathers them after its backward and
 * hands dst (MAX-all-reduced over data-parallel ranks) to
 * asr_optim_step_guarded, so a pass whose spin gave up never updates the
 * weights; the host reads dst at the step's loss read-back and skips the
 * batch (training_loop.py:69-76 semantics).  asr_lstm_status_inject sets the
 * tagged-granule word (test hook: what a spin give-up does). */
int asr_lstm_status_gather(int* dst, int clear, void* stream);
int asr_lstm_status_inject(int bits, void* stream);

/* Hand-off protocols the tagged-granule recurrence (lstm_xg.hip) has run
 * since the last clear: bit 0 write-through (sc1, any placement), bit 1
 * XCD-local (every group's work-groups registered on one XCD).  Synchronises
 * the device. */
int asr_lstm_xg_mode(int* mode, int clear);

/* Which recurrence implementation the last BLSTM layer pass ran (host-side
 * record), out2 = {forward pass, backward pass}: 0 per-step kernels, 1
 * tagged-granule bf16, 2 tagged-granule f32 (reference precision), 3
 * tagged-granule bf16 with the fused input projection, 4 counter-form
 * persistent. */
int asr_lstm_last_path(int* out2);

/* Diagnostics (ASR_XG_TRACE=1 at the first recurrence launch): copies the
 * per-step phase timestamps of work-groups 0..63 (64 x 128 steps x 12 u64) to
 * `host` (may be NULL); returns the element count, 0 when tracing is off. */
long long asr_xg_trace_read(unsigned long long* host);
/* Work-groups the tagged-granule backward recurrence launches for [B, *, H]
 * with xu units per work-group (0: ASR_XG_BWD_XU, else 16; 16; 32 where the
 * shape supports it); 0 if the shape cannot take that path. */
int asr_lstm_backward_grid(int B, int H, int xu);
/* Arrivals a launch with opts->bwd_units = xu adds to opts->progress at each
 * reporting step, 0 if the shape cannot take that path.  asr_lstm_progress_gate
 * enqueues a wait on `stream` until *counter >= target, the running total (bounded; a
 * timeout sets the recurrence status word, so the step is skipped). */
long long asr_lstm_bwd_progress_arrivals(int B, int H, int xu);
int asr_lstm_progress_gate(const unsigned long long* counter, long long target, void* stream);
/* Leading bytes of a recurrence workspace a tagged-granule launch of [B, *, H]
 * zeroes (what opts->ws_prezeroed promises; the arena clears only these). */
size_t asr_lstm_ws_zero_bytes(int B, int H);
/* Stream-ordered: flags[k] = epoch after the work enqueued before it. */
int asr_lstm_dy_signal(int* flags, int k, int epoch, void* stream);
/* Diagnostics only (tools/cores_locate.py): backward recurrence launches
 * enqueued on `stream` after this call record every dh_t their cell waves form
 * into dh ([B][T][2][H] f32), each step's sweep spin count into spins
 * ([ceil(B/R)][T][2][H/16] u32) and, per cell and step, the four gate
 * gradients computed, the four activations, c_t, c_{t-1}, dy and the incoming
 * dc into cell ([B][T][2][H][12] f32); NULL pointers switch recording off. */
int asr_lstm_debug_dh(float* dh, unsigned* spins, float* cell, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H_ */
