// Attention beam search on gfx950 (AttentionSeq2seq._decode_infer_beam,
// attention_seq2seq.py:1038-1237 of the reference) for bahdanau order, one
// decoder layer without residual -- an LSTMCell (the decoders the fused pass
// covers) or a GRUCell (ex->cell; the TIMIT attention recipes) --
// and one head of location or content attention.  f32 arithmetic in both
// compute modes: a beam of at most W rows needs no MFMA throughput, and a bf16
// near-tie flip changes whole hypotheses.
//
// Semantics (those of the host path, which the recorded fixtures pin):
//   * each utterance decodes over its own frames: T = lens[b], enc[b, :L].
//     The attention mask is multiplicative, so a frame past the length would
//     get energy 0 and a non-zero weight; here the convolution window, the
//     softmax and the context all stop at L, as if the utterance were alone.
//   * step 0 runs one row from <sos> and the initial state (no cell step, the
//     first attention uses h0); later steps run the live hypotheses (<= W).
//   * per row: f32 log-softmax (lg - max) - log(sum(exp(lg - max))), then the
//     min(W, V) best classes in descending order, the lower class index first
//     among equal values.
//   * candidates in (parent ascending, rank ascending) order; <eos> is dropped
//     while len(hyp) < min_decode_len (len counts <sos>: t + 1 at step t);
//     score = (parent score + log-prob) + length_penalty, in double.
//   * sort by score, descending and stable (ties keep generation order), keep
//     the first W: those ending in <eos> join `complete`, the others form the
//     next beam.
//   * an utterance stops once `complete` holds W entries (the first W in
//     insertion order are kept), or its beam is empty, or at max_decode_len.
//     If nothing completed, the final beam is `complete`.  The answer is the
//     top score of a stable descending sort of `complete`.
//   * the hypothesis includes its final <eos> if it completed; its attention
//     weights follow its parent rows step by step ([len][L]).
//
// Kernels, launched in a fixed order on the caller's stream, max_decode_len
// times (no host read, no spin-wait, no hand-off between work-groups; every
// work-group reads its utterance's done word first and leaves uniformly):
//   beam_cell    (row)  t >= 1: embedding of the row's token, LSTMCell on
//                       [e; ctx; h] of the parent row -> h, c
//   beam_cell_gru (row) in beam_cell's place for a GRU decoder: GRUCell (gate
//                       rows r, z, n) on the same [e; ctx; h] -> h; c is unused.
//                       Only the cell kernel knows the cell type: every kernel
//                       below, the joint search's included, is shared
//   beam_attend  (row)  W_dec h, conv(aw of the parent row), energies,
//                       sharpening, softmax / sigmoid over L, context; aw goes
//                       to the per-step record [step][row][T]
//   beam_expand  (row)  z = tanh(W_d h + b_d + W_c ctx + b_c), the V logits,
//                       log-softmax, the min(W, V) best in order
//   beam_select  (utt)  one wave: the <= W x W candidates, W rounds of
//                       (score descending, generation index ascending), then
//                       completion and the next beam (token, parent, score)
//   beam_backtrack (utt) at the end: best entry, its tokens and aw rows
// The state is double buffered by step parity and read through the parent
// index, so no gather pass exists.
//
// Joint CTC/attention search (ex->ctc, weight = lambda in
// (0, 1]; the host path of the model follows the same contract; lambda == 0 is
// the search above, with the launches above):
//   * label spaces: attention class c (c != <eos>) is CTC class c +
//     label_offset (1: decode_ctc's h - 1 mapping), blank is its own class,
//     <eos> has no CTC class.
//   * lp_t(k): the f32 log-softmax (lg - max) - log(sum(exp(lg - max))) of the
//     CTC head's logits [b, t], over the utterance's own frames t < L only.
//     Everything below is double; LOGZERO = -1.0e10 stands for log 0 and
//     logaddexp is the ordinary one on these finite values.
//   * prefix state of a hypothesis g (its tokens after <sos>): gn_t(g), gb_t(g),
//     t < L, the log-probability of the alignments of g over frames 0..t that
//     end in a non-blank / in a blank.  Empty g: gn_t = LOGZERO, gb_t = the
//     running sum of lp_tau(blank), psi = 0.
//   * prefix score of g.c, c != <eos>: with phi_t = logaddexp(gn_t(g), gb_t(g)),
//     or gb_t(g) alone when c == last(g), and r_n[0] = lp_0(c) if g is empty
//     else LOGZERO:  psi(g.c) = logaddexp over {r_n[0]} and {phi_{t-1} +
//     lp_t(c) : 1 <= t < L} -- the parent's state only, a reduction over frames.
//   * new state of a kept row: gn_t(g.c) = logaddexp(gn_{t-1}(g.c), phi_{t-1}) +
//     lp_t(c), gb_t(g.c) = logaddexp(gn_{t-1}(g.c), gb_{t-1}(g.c)) + lp_t(blank),
//     gn_0 = r_n[0], gb_0 = LOGZERO.
//   * CTC term of a candidate: delta = psi(g.c) - psi(g), or for <eos>
//     logaddexp(gn_{L-1}(g), gb_{L-1}(g)) - psi(g); psi(g) travels with the row.
//   * the search is the one above except for the score: the candidates are
//     still the min(W, V) best ATTENTION classes of each row in (parent, rank)
//     order, and score = (parent score + (1 - lambda) lp_att(c) + lambda delta)
//     + length_penalty, in double.
// What is stored per row is (phi_t, gb_t) = (logaddexp(gn_t, gb_t), gb_t): a
// child needs nothing else of its parent (gn only inside phi), so the score
// kernel does no logaddexp per frame.  Added kernels:
//   beam_ctc_lse   (frame) once: max and log-sum of the head's logits per valid
//                       frame.  lp_t(k) is formed from them where it is read;
//                       the logits stay in place.  A candidate's column
//                       lp_.(c) is strided by Vc floats, and every candidate's
//                       column is read exactly once per step (the <= W kept
//                       rows' once more), so gathering the <= W min(W, V)
//                       columns first would do the same strided reads plus a
//                       write and a re-read: columns are read in place.
//   beam_ctc_empty (utt)   once: the empty prefix's state, a wave scan
//   beam_ctc_advance (row) t >= 1, before beam_ctc_score: the row's (phi, gb)
//                       from its parent's and its token; 64-frame chunks are
//                       loaded by the wave, scanned by one lane, stored by
//                       the wave (the only part sequential in the frames)
//   beam_ctc_score (row)   between beam_expand and beam_select: one wave per
//                       candidate, lanes over frames, a wave log-sum-exp:
//                       psi(g.c) and delta of the row's min(W, V) candidates
//   beam_select_ctc (utt)  beam_select with the joint score; hands psi on
//
// Shallow fusion with an RNN language model (ex->lm, weight =
// gamma > 0; the host path of the model follows the same contract; gamma == 0 or
// no LM is the search above, with the launches above):
//   * label spaces: LM class c is attention class c, <eos> included (an ordinary
//     LM class); <sos> is the <eos> index.
//   * candidates are still the min(W, V) best ATTENTION classes of each row in
//     (parent, rank) order: the LM re-ranks the candidates, it nominates none.
//   * LM state of a row: (h, c) per LM layer (stacked LSTM layers, torch's gate
//     rows i, f, g, o), zero before step 0.  At EVERY step t >= 0 the row feeds
//     its last token (<sos> at t = 0) from its PARENT's LM state: the attention
//     cell takes no step at t = 0, the LM does.
//   * lp_lm(c | g): the f32 log-softmax (lg - max) - log(sum(exp(lg - max))) of
//     the LM's output logits W_out h_top + b_out after that step.
//   * score = (parent score + (1 - lambda) lp_att(c) + lambda delta_ctc +
//     gamma lp_lm(c | g)) + length_penalty, in double; the CTC term only when
//     lambda > 0 (else lp_att(c) stands alone).  The tie rules, the
//     min_decode_len rule, completion and backtracking are unchanged.
// Added kernels:
// (the LM's arithmetic is csrc/beam_lm.h's, shared with the CTC prefix search)
//   beam_lm_cell   (row)  every t, before beam_lm_score: embedding of the row's
//                       token, then the LM's layers in order inside the
//                       work-group: [x; h] of the parent row in LDS, one wave per
//                       hidden unit as beam_cell, a barrier between layers (a
//                       layer's h is the next one's x).  State [2][R][layers][H],
//                       double buffered by step parity, read through the parent
//                       index
//   beam_lm_score  (row)  after beam_expand: the V output logits, one wave per
//                       class, to the workspace; max and log-sum; lp_lm of the
//                       row's min(W, V) candidates to a [row][W] table
//   beam_select_lm / beam_select_ctc_lm (utt)  beam_select / beam_select_ctc
//                       with the gamma term
#include <limits.h>

#include "beam_lm.h"

namespace asr {
namespace {

constexpr int kMinBeam = 2, kMaxBeam = 32;
constexpr int CELL_THREADS = 256, ATT_THREADS = 512, EXP_THREADS = 256, BT_THREADS = 256;
constexpr int kMaxC = 16;

struct BeamP {
  int B, T, E, A, C, K, D, W, V, Y, Dz, max_len, min_len, eos, sigmoid, emb_trans;
  float sharpen;
  double penalty;
  long long ld_ih;
  const float *enc, *enc_a, *h0;
  const int32_t* lens;
  const float *w_ih, *w_hh, *b_ih, *b_hh, *w_dec, *w_conv, *conv_w, *v;
  const float *w_d, *b_d, *w_c, *b_c, *w_fc, *b_fc, *emb_w;
  // workspace
  float *h, *c, *ctx;      // [2][R][D], [2][R][D], [2][R][E]   (R = B * W)
  float *lg;               // [R][V]
  float *awrec;            // [max_len][R][T]
  float *topv;             // [R][W]
  int *topc;               // [R][W]
  double *sc;              // [B][W] scores of the live rows
  int *tok_tab, *par_tab;  // [max_len][B][W]: row j of step t + 1 = (token, parent row) picked at t
  int *n_live, *done, *ncomp, *last_t;   // [B]
  double *comp_score;      // [B][W]
  int *comp_t, *comp_par;  // [B][W]: completed at step t from parent row
  int *rows;               // [B][max_len]: the best hypothesis' row per step
};

// the joint search's additions (ex->ctc)
struct CtcP {
  const float* lg;         // [B][T][Vc] logits of the CTC head
  int Vc, blank, off;
  double weight;
  // workspace
  float *mx, *lse;         // [B][T] per valid frame
  double *phi, *gb;        // [2][R][T] by step parity: logaddexp(gn_t, gb_t), gb_t of the row's prefix
  double *psi;             // [2][R]
  double *delta, *psic;    // [R][W] per candidate: CTC term, psi(g.c)
};
constexpr double kLogZero = -1.0e10;

// the language model's additions (ex->lm); net.V is p.V
struct LmP {
  LmNet net;
  double weight;
  // workspace
  float *h, *c;            // [2][R][layers][H] by step parity
  float *lg;               // [R][V] output logits
  float *lp;               // [R][W] lp_lm of the row's candidates
};

__device__ __forceinline__ int utt_len(const BeamP& p, int b) {
  return max(0, min(p.lens[b], p.T));
}

__device__ __forceinline__ float block_red(float v, float* red, bool is_max) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256) beam_init(BeamP p) {
  const int b = blockIdx.x;
  const long long r = (long long)b * p.W;
  for (int j = threadIdx.x; j < p.D; j += blockDim.x) {
    p.h[r * p.D + j] = p.h0 ? p.h0[(long long)b * p.D + j] : 0.f;
    p.c[r * p.D + j] = 0.f;
  }
  if (threadIdx.x == 0) {
    p.n_live[b] = 1;
    p.done[b] = (utt_len(p, b) <= 0 || p.max_len <= 0) ? 1 : 0;
    p.ncomp[b] = 0;
    p.last_t[b] = -1;
    p.sc[r] = 0.0;
  }
}

// ------------------------------------------------------------------- cell
// Row i of step t: its state's place (cur) and its parent's (prev), and [e; ctx;
// h] of the parent row staged to x ([Y + E + D], LDS) for the whole work-group.
struct CellRow { long long cur, prev; };

__device__ __forceinline__ CellRow cell_stage(int t, const BeamP& p, int i, int b, float* x) {
  const int tid = threadIdx.x;
  const long long R = (long long)p.B * p.W;
  const long long tab = ((long long)(t - 1) * p.B + b) * p.W + i;
  const int par = p.par_tab[tab], tok = p.tok_tab[tab];
  const long long r = (long long)b * p.W + i, pr = (long long)b * p.W + par;
  const int cur = t & 1, prev = cur ^ 1;
  for (int y = tid; y < p.Y; y += CELL_THREADS)
    x[y] = p.emb_trans ? p.emb_w[(long long)y * p.V + tok] : p.emb_w[(long long)tok * p.Y + y];
  for (int e = tid; e < p.E; e += CELL_THREADS) x[p.Y + e] = p.ctx[(prev * R + pr) * p.E + e];
  for (int j = tid; j < p.D; j += CELL_THREADS) x[p.Y + p.E + j] = p.h[(prev * R + pr) * p.D + j];
  __syncthreads();
  return {cur * R + r, prev * R + pr};
}

__global__ void __launch_bounds__(CELL_THREADS) beam_cell(int t, BeamP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = CELL_THREADS / 64;
  const int YE = p.Y + p.E;
  float* x = sm;
  const CellRow cr = cell_stage(t, p, i, b, x);
  for (int u = w; u < p.D; u += nw) {   // one wave per hidden unit, lanes over K
    float s[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const long long row = (long long)g * p.D + u;
      const float* wi = p.w_ih + row * p.ld_ih;
      const float* wh = p.w_hh + row * p.D;
      float a = 0.f;
      for (int k = lane; k < YE; k += 64) a += wi[k] * x[k];
      for (int k = lane; k < p.D; k += 64) a += wh[k] * x[YE + k];
      s[g] = wave_sum(a) + p.b_ih[row] + p.b_hh[row];
    }
    if (lane == 0) {
      const float ig = sigmoidf_(s[0]), fg = sigmoidf_(s[1]);
      const float gg = tanhf_(s[2]), og = sigmoidf_(s[3]);
      const float cn = fg * p.c[cr.prev * p.D + u] + ig * gg;
      p.c[cr.cur * p.D + u] = cn;
      p.h[cr.cur * p.D + u] = og * tanhf_(cn);
    }
  }
}

// GRUCell (gate rows r, z, n): beam_cell's row, tables and staging.  r scales the hidden part of the n gate only, its bias included,
// so that gate's two parts are summed apart.  No c state.
__global__ void __launch_bounds__(CELL_THREADS) beam_cell_gru(int t, BeamP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = CELL_THREADS / 64;
  const int YE = p.Y + p.E;
  float* x = sm;
  const CellRow cr = cell_stage(t, p, i, b, x);
  for (int u = w; u < p.D; u += nw) {   // one wave per hidden unit, lanes over K
    float si[3], sh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const long long row = (long long)g * p.D + u;
      const float* wi = p.w_ih + row * p.ld_ih;
      const float* wh = p.w_hh + row * p.D;
      float a = 0.f, c = 0.f;
      for (int k = lane; k < YE; k += 64) a += wi[k] * x[k];
      for (int k = lane; k < p.D; k += 64) c += wh[k] * x[YE + k];
      si[g] = wave_sum(a) + p.b_ih[row];
      sh[g] = wave_sum(c) + p.b_hh[row];
    }
    if (lane == 0) {
      const float rg = sigmoidf_(si[0] + sh[0]), zg = sigmoidf_(si[1] + sh[1]);
      const float ng = tanhf_(si[2] + rg * sh[2]);
      p.h[cr.cur * p.D + u] = (1.f - zg) * ng + zg * x[YE + u];
    }
  }
}

// -------------------------------------------------------------- attention
__host__ __device__ inline size_t attend_lds_floats(int D, int A, int C, int K, int T) {
  return (size_t)D + 2 * (size_t)A + (size_t)C * K + (size_t)A * C + ((size_t)T + K - 1) + T + 64;
}

__global__ void __launch_bounds__(ATT_THREADS) beam_attend(int t, BeamP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = ATT_THREADS / 64;
  const int L = utt_len(p, b), half = p.K / 2;
  const long long R = (long long)p.B * p.W;
  const long long r = (long long)b * p.W + i;
  const int cur = t & 1;
  float* hS = sm;                          // [D]
  float* wd = hS + p.D;                    // [A]  W_dec h
  float* vS = wd + p.A;                    // [A]
  float* cw = vS + p.A;                    // [C*K]
  float* wc = cw + (size_t)p.C * p.K;      // [A*C]
  float* awp = wc + (size_t)p.A * p.C;     // [L + K - 1] aw_{t-1}[tt - half + k], 0 outside [0, L)
  float* e = awp + (p.T + p.K - 1);        // [L] energies, then aw_t
  float* red = e + p.T;                    // [64]
  for (int j = tid; j < p.D; j += ATT_THREADS) hS[j] = p.h[(cur * R + r) * p.D + j];
  for (int j = tid; j < p.A; j += ATT_THREADS) vS[j] = p.v[j];
  for (int j = tid; j < p.C * p.K; j += ATT_THREADS) cw[j] = p.conv_w[j];
  for (int j = tid; j < p.A * p.C; j += ATT_THREADS) wc[j] = p.w_conv[j];
  if (t > 0) {
    const int par = p.par_tab[((long long)(t - 1) * p.B + b) * p.W + i];
    const float* ap = p.awrec + ((long long)(t - 1) * R + (long long)b * p.W + par) * p.T;
    for (int j = tid; j < L + p.K - 1; j += ATT_THREADS) {
      const int tt = j - half;
      awp[j] = (tt >= 0 && tt < L) ? ap[tt] : 0.f;
    }
  }
  __syncthreads();
  for (int a = w; a < p.A; a += nw) {
    const float* wr = p.w_dec + (long long)a * p.D;
    float s = 0.f;
    for (int k = lane; k < p.D; k += 64) s += wr[k] * hS[k];
    s = wave_sum(s);
    if (lane == 0) wd[a] = s;
  }
  __syncthreads();
  for (int tt = w; tt < L; tt += nw) {     // one wave per frame
    float f[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      f[c] = 0.f;
      if (c < p.C && t > 0) {              // wave-uniform
        float s = 0.f;
        for (int k = lane; k < p.K; k += 64) s += cw[c * p.K + k] * awp[tt + k];
        f[c] = wave_sum(s);
      }
    }
    const float* er = p.enc_a + ((long long)b * p.T + tt) * p.A;
    float s = 0.f;
    for (int a = lane; a < p.A; a += 64) {
      float q = er[a] + wd[a];
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < p.C) q += f[c] * wc[a * p.C + c];
      s += vS[a] * tanhf(q);
    }
    s = wave_sum(s);
    if (lane == 0) e[tt] = s * p.sharpen;
  }
  __syncthreads();
  if (p.sigmoid) {
    for (int j = tid; j < L; j += ATT_THREADS) e[j] = sigmoidf_(e[j]);
  } else {
    float mx = neg_inf();
    for (int j = tid; j < L; j += ATT_THREADS) mx = fmaxf(mx, e[j]);
    mx = block_red(mx, red, true);
    float s = 0.f;
    for (int j = tid; j < L; j += ATT_THREADS) {
      const float q = __expf(e[j] - mx);
      e[j] = q;
      s += q;
    }
    s = block_red(s, red, false);
    const float inv = 1.f / s;
    for (int j = tid; j < L; j += ATT_THREADS) e[j] *= inv;
  }
  __syncthreads();
  float* rec = p.awrec + ((long long)t * R + r) * p.T;
  for (int j = tid; j < p.T; j += ATT_THREADS) rec[j] = j < L ? e[j] : 0.f;
  for (int col = tid; col < p.E; col += ATT_THREADS) {
    const float* er = p.enc + (long long)b * p.T * p.E + col;
    float s = 0.f;
    int tt = 0;
    for (; tt + 8 <= L; tt += 8) {
      float u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = er[(long long)(tt + j) * p.E];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += e[tt + j] * u[j];
    }
    for (; tt < L; ++tt) s += e[tt] * er[(long long)tt * p.E];
    p.ctx[(cur * R + r) * p.E + col] = s;
  }
}

// ----------------------------------------------------------------- expand
__device__ __forceinline__ void arg_pair(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ void __launch_bounds__(EXP_THREADS) beam_expand(int t, BeamP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = EXP_THREADS / 64;
  const long long R = (long long)p.B * p.W;
  const long long r = (long long)b * p.W + i;
  const int cur = t & 1;
  float* hS = sm;             // [D]
  float* cS = hS + p.D;       // [E]
  float* z = cS + p.E;        // [Dz]
  float* red = z + p.Dz;      // [4]
  int* redi = (int*)(red + 4);   // [4]
  for (int j = tid; j < p.D; j += EXP_THREADS) hS[j] = p.h[(cur * R + r) * p.D + j];
  for (int j = tid; j < p.E; j += EXP_THREADS) cS[j] = p.ctx[(cur * R + r) * p.E + j];
  __syncthreads();
  for (int k = w; k < p.Dz; k += nw) {
    const float* wdr = p.w_d + (long long)k * p.D;
    const float* wcr = p.w_c + (long long)k * p.E;
    float sa = 0.f, sc = 0.f;
    for (int j = lane; j < p.D; j += 64) sa += wdr[j] * hS[j];
    for (int j = lane; j < p.E; j += 64) sc += wcr[j] * cS[j];
    sa = wave_sum(sa);
    sc = wave_sum(sc);
    if (lane == 0) z[k] = tanhf((sa + (p.b_d ? p.b_d[k] : 0.f)) + (sc + (p.b_c ? p.b_c[k] : 0.f)));
  }
  __syncthreads();
  float* lg = p.lg + r * p.V;
  float mx = neg_inf();
  for (int v = w; v < p.V; v += nw) {      // one wave per class
    const float* wr = p.w_fc + (long long)v * p.Dz;
    float s = 0.f;
    for (int k = lane; k < p.Dz; k += 64) s += wr[k] * z[k];
    s = wave_sum(s) + (p.b_fc ? p.b_fc[v] : 0.f);
    if (lane == 0) lg[v] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_red(mx, red, true);           // its barriers also publish lg to the work-group
  float se = 0.f;
  for (int v = tid; v < p.V; v += EXP_THREADS) se += expf(lg[v] - mx);
  se = block_red(se, red, false);
  const float lse = logf(se);
  // round k takes the best of what lies strictly after round k - 1's pick in
  // the order (log-prob descending, class ascending)
  const int ktop = min(p.W, p.V);
  float pv = __builtin_huge_valf();
  int pi = -1;
  for (int k = 0; k < ktop; ++k) {
    float bv = neg_inf();
    int bi = INT_MAX;
    for (int v = tid; v < p.V; v += EXP_THREADS) {
      const float lp = (lg[v] - mx) - lse;
      if (lp < pv || (lp == pv && v > pi)) arg_pair(bv, bi, lp, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      arg_pair(bv, bi, ov, oi);
    }
    __syncthreads();
    if (lane == 0) { red[w] = bv; redi[w] = bi; }
    __syncthreads();
    bv = red[0];
    bi = redi[0];
    for (int q = 1; q < nw; ++q) arg_pair(bv, bi, red[q], redi[q]);
    if (tid == 0) {
      p.topv[r * p.W + k] = bv;
      p.topc[r * p.W + k] = bi == INT_MAX ? -1 : bi;
    }
    pv = bv;
    pi = bi;
  }
}

// ----------------------------------------------------------- language model
// One step of the LM's stacked LSTM for row i of step t: token and parent from
// the tables (t == 0: <sos> from the zero state).  The loop is lm_lstm_step's
// (csrc/beam_lm.h), kept in its own text here: through the shared function this
// kernel measured 3 % slower (620 ms against 601 ms a call at W 4, V 29, a 2 x
// 512 LM), with the same registers and the same instructions in the loop.  A
// change to either copy goes into both.
__global__ void __launch_bounds__(LM_THREADS) beam_lm_cell(int t, BeamP p, LmP m) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const long long R = (long long)p.B * p.W;
  int par = 0, tok = p.eos;
  if (t > 0) {
    const long long tab = ((long long)(t - 1) * p.B + b) * p.W + i;
    par = p.par_tab[tab];
    tok = p.tok_tab[tab];
  }
  const long long r = (long long)b * p.W + i, pr = (long long)b * p.W + par;
  const int cur = t & 1, prev = cur ^ 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = LM_THREADS / 64;
  const LmNet& n = m.net;
  const int H = n.H, XM = max(n.Y, H);
  float* xa = sm;            // [max(Y, H)]
  float* xb = xa + XM;       // [max(Y, H)]
  float* hp = xb + XM;       // [H]
  for (int y = tid; y < n.Y; y += LM_THREADS) xa[y] = n.emb[(long long)tok * n.Y + y];
  for (int l = 0; l < n.layers; ++l) {
    const int in = l == 0 ? n.Y : H;
    const long long so = ((cur * R + r) * n.layers + l) * H;    // this row's state
    const long long sp = ((prev * R + pr) * n.layers + l) * H;  // the parent's
    for (int j = tid; j < H; j += LM_THREADS) hp[j] = t > 0 ? m.h[sp + j] : 0.f;
    __syncthreads();
    const float* wi_l = n.w_ih[l];
    const float* wh_l = n.w_hh[l];
    for (int u = w; u < H; u += nw) {   // one wave per hidden unit, lanes over K
      float s[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long long row = (long long)g * H + u;
        const float* wi = wi_l + row * in;
        const float* wh = wh_l + row * H;
        float a = 0.f;
        for (int k = lane; k < in; k += 64) a += wi[k] * xa[k];
        for (int k = lane; k < H; k += 64) a += wh[k] * hp[k];
        s[g] = wave_sum(a) + n.b_ih[l][row] + n.b_hh[l][row];
      }
      if (lane == 0) {
        const float ig = sigmoidf_(s[0]), fg = sigmoidf_(s[1]);
        const float gg = tanhf_(s[2]), og = sigmoidf_(s[3]);
        const float cn = fg * (t > 0 ? m.c[sp + u] : 0.f) + ig * gg;
        const float hn = og * tanhf_(cn);
        m.c[so + u] = cn;
        m.h[so + u] = hn;
        xb[u] = hn;
      }
    }
    __syncthreads();         // xb is complete; xa and hp are free
    float* sw = xa;
    xa = xb;
    xb = sw;
  }
}

// lp_lm of the row's candidates (beam_expand's topc) from the top layer's h
__global__ void __launch_bounds__(LM_THREADS) beam_lm_score(int t, BeamP p, LmP m) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int tid = threadIdx.x;
  const long long R = (long long)p.B * p.W;
  const long long r = (long long)b * p.W + i;
  const int cur = t & 1, H = m.net.H;
  float* hS = sm;            // [H]
  float* red = hS + H;       // [4]
  const float* hs = m.h + (((cur * R + r) * m.net.layers) + (m.net.layers - 1)) * H;
  for (int j = tid; j < H; j += LM_THREADS) hS[j] = hs[j];
  __syncthreads();
  float* lg = m.lg + r * p.V;
  float mx, lse;
  lm_output_lse<wave_sum>(m.net, hS, lg, red, mx, lse);
  const int ktop = min(p.W, p.V);
  for (int k = tid; k < ktop; k += LM_THREADS) {
    const int c = p.topc[r * p.W + k];
    m.lp[r * p.W + k] = c >= 0 ? (lg[c] - mx) - lse : 0.f;
  }
}

// ----------------------------------------------------------------- select
// CTC: the joint score, and psi(g.c) of a kept candidate goes on with its row;
// LM: the candidate's gamma lp_lm(c | g) joins the sum inside the parentheses
template <bool CTC, bool LM>
__device__ __forceinline__ void select_body(int t, const BeamP& p, const CtcP* q, const LmP* m) {
  __shared__ double s_score[kMaxBeam * kMaxBeam];
  __shared__ int s_tok[kMaxBeam * kMaxBeam];
  __shared__ double s_selv[kMaxBeam];
  __shared__ int s_seli[kMaxBeam];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (p.done[b]) return;
  const int n = p.n_live[b];
  const int ktop = min(p.W, p.V);
  const int nc = n * ktop;                 // <= W * W
  const long long r0 = (long long)b * p.W;
  for (int e = lane; e < nc; e += 64) {
    const int i = e / ktop, k = e - i * ktop;
    const int tok = p.topc[(r0 + i) * p.W + k];
    const bool drop = tok < 0 || (tok == p.eos && t + 1 < p.min_len);
    s_tok[e] = drop ? -1 : tok;
    // ((sc + att) [+ lam d] [+ gl]) + penalty, in this order
    const long long ck = (r0 + i) * p.W + k;
    double s = p.sc[r0 + i];
    if constexpr (CTC) {
      const double lam = q->weight, d = tok < 0 ? 0.0 : q->delta[ck];
      s = s + (1.0 - lam) * (double)p.topv[ck] + lam * d;
    } else {
      s = s + (double)p.topv[ck];
    }
    if constexpr (LM) s = s + (tok < 0 ? 0.0 : m->weight * (double)m->lp[ck]);
    s_score[e] = s + p.penalty;
  }
  __syncthreads();
  // W rounds of (score descending, generation index ascending)
  double ps = __builtin_huge_val();
  int pi = -1, nsel = 0;
  for (int rd = 0; rd < p.W; ++rd) {
    double bs = -__builtin_huge_val();
    int bi = INT_MAX;
    for (int e = lane; e < nc; e += 64) {
      if (s_tok[e] < 0) continue;
      const double s = s_score[e];
      const bool after = s < ps || (s == ps && e > pi);
      if (after && (bi == INT_MAX || s > bs)) { bs = s; bi = e; }   // e ascending: first wins
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
    }
    if (bi == INT_MAX) break;              // wave-uniform
    if (lane == 0) { s_selv[rd] = bs; s_seli[rd] = bi; }
    ps = bs;
    pi = bi;
    ++nsel;
  }
  __syncthreads();
  if (lane == 0) {
    // p.sc was last read before the barrier above: the new beam's scores go
    // straight over it (unused if the utterance completes at this step)
    int ncomp = p.ncomp[b], nb = 0;
    for (int rd = 0; rd < nsel; ++rd) {
      const int e = s_seli[rd], i = e / ktop, tok = s_tok[e];
      if (tok == p.eos) {
        if (ncomp < p.W) {
          p.comp_score[r0 + ncomp] = s_selv[rd];
          p.comp_t[r0 + ncomp] = t;
          p.comp_par[r0 + ncomp] = i;
        }
        ++ncomp;
      } else {
        const long long tab = ((long long)t * p.B + b) * p.W + nb;
        p.tok_tab[tab] = tok;
        p.par_tab[tab] = i;
        p.sc[r0 + nb] = s_selv[rd];
        if constexpr (CTC) {
          const long long R = (long long)p.B * p.W;
          q->psi[((t + 1) & 1) * R + r0 + nb] = q->psic[(r0 + i) * p.W + (e - i * ktop)];
        }
        ++nb;
      }
    }
    if (ncomp >= p.W) {                    // complete = complete[:W]; break
      p.ncomp[b] = p.W;
      p.done[b] = 1;
    } else {
      p.ncomp[b] = ncomp;
      p.n_live[b] = nb;
      p.last_t[b] = t;
      if (nb == 0) p.done[b] = 1;
    }
  }
}

__global__ void __launch_bounds__(64) beam_select(int t, BeamP p) {
  select_body<false, false>(t, p, nullptr, nullptr);
}

__global__ void __launch_bounds__(64) beam_select_ctc(int t, BeamP p, CtcP q) {
  select_body<true, false>(t, p, &q, nullptr);
}

__global__ void __launch_bounds__(64) beam_select_lm(int t, BeamP p, LmP m) {
  select_body<false, true>(t, p, nullptr, &m);
}

__global__ void __launch_bounds__(64) beam_select_ctc_lm(int t, BeamP p, CtcP q, LmP m) {
  select_body<true, true>(t, p, &q, &m);
}

// ------------------------------------------------------ CTC prefix scoring
constexpr int LSE_THREADS = 256, SCORE_THREADS = 256;

__device__ __forceinline__ double logaddexp_(double a, double b) {
  return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

// lp_t(k) of utterance b, t < L
__device__ __forceinline__ double ctc_lp(const BeamP& p, const CtcP& q, int b, int t, int k) {
  const long long f = (long long)b * p.T + t;
  return (double)((q.lg[f * q.Vc + k] - q.mx[f]) - q.lse[f]);
}

__global__ void __launch_bounds__(LSE_THREADS) beam_ctc_lse(BeamP p, CtcP q) {
  __shared__ float red[LSE_THREADS / 64];
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= utt_len(p, b)) return;
  const long long f = (long long)b * p.T + t;
  const float* lg = q.lg + f * q.Vc;
  float mx = neg_inf();
  for (int v = threadIdx.x; v < q.Vc; v += LSE_THREADS) mx = fmaxf(mx, lg[v]);
  mx = block_red(mx, red, true);
  float se = 0.f;
  for (int v = threadIdx.x; v < q.Vc; v += LSE_THREADS) se += expf(lg[v] - mx);
  se = block_red(se, red, false);
  if (threadIdx.x == 0) {
    q.mx[f] = mx;
    q.lse[f] = logf(se);
  }
}

// the empty prefix: gb_t = sum_{tau <= t} lp_tau(blank), gn_t = LOGZERO, psi = 0 (row 0, parity 0)
__global__ void __launch_bounds__(64) beam_ctc_empty(BeamP p, CtcP q) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int L = utt_len(p, b);
  const long long r0 = (long long)b * p.W;
  double carry = 0.0;
  for (int base = 0; base < L; base += 64) {
    const int t = base + lane;
    double v = t < L ? ctc_lp(p, q, b, t, q.blank) : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    v += carry;
    if (t < L) {
      q.gb[r0 * p.T + t] = v;
      q.phi[r0 * p.T + t] = logaddexp_(kLogZero, v);
    }
    carry = __shfl(v, 63, 64);
  }
  if (lane == 0) q.psi[r0] = 0.0;
}

__global__ void __launch_bounds__(64) beam_ctc_advance(int t, BeamP p, CtcP q) {
  __shared__ double s_a[64], s_phi[64], s_gb[64];
  __shared__ float s_lc[64], s_lb[64];
  const int i = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int L = utt_len(p, b);
  const long long R = (long long)p.B * p.W;
  const long long tab = ((long long)(t - 1) * p.B + b) * p.W + i;
  const int par = p.par_tab[tab], tok = p.tok_tab[tab];
  const int cur = t & 1, prev = cur ^ 1;
  const long long r = (long long)b * p.W + i, pr = (long long)b * p.W + par;
  // the parent's own last token: it has one from step 2 on
  bool rep = false;
  if (t >= 2) rep = p.tok_tab[((long long)(t - 2) * p.B + b) * p.W + par] == tok;
  const double* pa = (rep ? q.gb : q.phi) + (prev * R + pr) * p.T;   // phi'_t of the parent
  double* ophi = q.phi + (cur * R + r) * p.T;
  double* ogb = q.gb + (cur * R + r) * p.T;
  const int k = tok + q.off;
  double gn = 0.0, gb = 0.0, ph = 0.0;   // lane 0's carry: gn_{t-1}, gb_{t-1}, their logaddexp
  for (int base = 0; base < L; base += 64) {
    const int f = base + lane;
    if (f < L) {
      const long long fr = (long long)b * p.T + f;
      const float m = q.mx[fr], ls = q.lse[fr];
      s_lc[lane] = (q.lg[fr * q.Vc + k] - m) - ls;
      s_lb[lane] = (q.lg[fr * q.Vc + q.blank] - m) - ls;
      s_a[lane] = f > 0 ? pa[f - 1] : 0.0;
    }
    __syncthreads();
    if (lane == 0) {
      const int n = min(64, L - base);
      for (int j = 0; j < n; ++j) {
        double ngn, ngb;
        if (base + j == 0) {   // gn_0 = r_n[0]: lp_0(c) only if the parent is the empty prefix
          ngn = t == 1 ? (double)s_lc[0] : kLogZero;
          ngb = kLogZero;
        } else {
          ngn = logaddexp_(gn, s_a[j]) + (double)s_lc[j];
          ngb = ph + (double)s_lb[j];   // ph = logaddexp(gn_{t-1}, gb_{t-1}), formed for the store
        }
        gn = ngn;
        gb = ngb;
        ph = logaddexp_(gn, gb);
        s_phi[j] = ph;
        s_gb[j] = gb;
      }
    }
    __syncthreads();
    if (f < L) {
      ophi[f] = s_phi[lane];
      ogb[f] = s_gb[lane];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(SCORE_THREADS) beam_ctc_score(int t, BeamP p, CtcP q) {
  const int i = blockIdx.x, b = blockIdx.y;
  if (p.done[b] || i >= p.n_live[b]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = SCORE_THREADS / 64;
  const int L = utt_len(p, b), ktop = min(p.W, p.V);
  const long long R = (long long)p.B * p.W;
  const long long r = (long long)b * p.W + i;
  const int cur = t & 1;
  const double* phi = q.phi + (cur * R + r) * p.T;
  const double* gb = q.gb + (cur * R + r) * p.T;
  const double psi_g = q.psi[cur * R + r];
  const int last = t > 0 ? p.tok_tab[((long long)(t - 1) * p.B + b) * p.W + i] : -1;
  for (int kk = w; kk < ktop; kk += nw) {   // one wave per candidate
    const int c = p.topc[r * p.W + kk];
    double psi_c = kLogZero, d = 0.0;
    if (c == p.eos) {
      d = phi[L - 1] - psi_g;
    } else if (c >= 0) {
      const double* pa = c == last ? gb : phi;
      const int k = c + q.off;
      // per lane a running (max, sum of exp(x - max)) over its frames
      double m = -__builtin_huge_val(), s = 0.0;
      for (int f = lane; f < L; f += 64) {
        double x;
        if (f == 0) x = t == 0 ? ctc_lp(p, q, b, 0, k) : kLogZero;
        else x = pa[f - 1] + ctc_lp(p, q, b, f, k);
        if (x > m) {
          s = s * exp(m - x) + 1.0;
          m = x;
        } else {
          s += exp(x - m);
        }
      }
      double M = m;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o, 64));
      s = s > 0.0 ? s * exp(m - M) : 0.0;   // M is finite: lane 0 holds frame 0
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      psi_c = M + log(s);
      d = psi_c - psi_g;
    }
    if (lane == 0) {
      q.delta[r * p.W + kk] = d;
      q.psic[r * p.W + kk] = psi_c;
    }
  }
}

// -------------------------------------------------------------- backtrack
__global__ void __launch_bounds__(BT_THREADS) beam_backtrack(BeamP p, long long* __restrict__ tokens,
                                                             int32_t* __restrict__ hyp_lens,
                                                             double* __restrict__ scores,
                                                             float* __restrict__ aw) {
  __shared__ int s_len;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long r0 = (long long)b * p.W;
  const long long R = (long long)p.B * p.W;
  int* rows = p.rows + (long long)b * p.max_len;
  long long* out = tokens + (long long)b * p.max_len;
  if (tid == 0) {
    int len = 0, tf = -1, par = 0, tok = -1;
    double best = 0.0;
    const int ncomp = p.ncomp[b];
    if (ncomp > 0) {                       // stable descending sort: the first maximum
      int q = 0;
      for (int j = 1; j < ncomp; ++j)
        if (p.comp_score[r0 + j] > p.comp_score[r0 + q]) q = j;
      best = p.comp_score[r0 + q];
      tf = p.comp_t[r0 + q];
      par = p.comp_par[r0 + q];
      tok = p.eos;
    } else if (p.last_t[b] >= 0 && p.n_live[b] > 0) {   // nothing completed: the final beam
      int q = 0;
      for (int j = 1; j < p.n_live[b]; ++j)
        if (p.sc[r0 + j] > p.sc[r0 + q]) q = j;
      best = p.sc[r0 + q];
      tf = p.last_t[b];
      const long long tab = ((long long)tf * p.B + b) * p.W + q;
      par = p.par_tab[tab];
      tok = p.tok_tab[tab];
    }
    if (tf >= 0) {
      len = tf + 1;
      out[tf] = tok;
      rows[tf] = par;
      for (int s = tf; s > 0; --s) {
        const long long tab = ((long long)(s - 1) * p.B + b) * p.W + rows[s];
        out[s - 1] = p.tok_tab[tab];
        rows[s - 1] = p.par_tab[tab];
      }
    }
    for (int s = len; s < p.max_len; ++s) out[s] = -1;
    hyp_lens[b] = len;
    scores[b] = best;
    s_len = len;
  }
  __syncthreads();
  const int len = s_len, L = utt_len(p, b);
  for (int s = 0; s < p.max_len; ++s) {
    float* dst = aw + ((long long)b * p.max_len + s) * p.T;
    const float* src = s < len ? p.awrec + ((long long)s * R + r0 + rows[s]) * p.T : nullptr;
    for (int j = tid; j < p.T; j += BT_THREADS) dst[j] = (src && j < L) ? src[j] : 0.f;
  }
}

inline size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

struct BeamWs {
  size_t h, c, ctx, lg, awrec, topv, topc, sc, tok_tab, par_tab, n_live, done, ncomp, last_t,
      comp_score, comp_t, comp_par, rows, total;
};

BeamWs beam_ws(int B, int T, int E, int D, int W, int V, int max_len) {
  BeamWs w;
  const size_t R = (size_t)B * W, ml = (size_t)(max_len > 0 ? max_len : 1);
  size_t o = 0;
  w.h = o; o += al256(2 * R * D * 4);
  w.c = o; o += al256(2 * R * D * 4);
  w.ctx = o; o += al256(2 * R * E * 4);
  w.lg = o; o += al256(R * V * 4);
  w.awrec = o; o += al256(ml * R * T * 4);
  w.topv = o; o += al256(R * W * 4);
  w.topc = o; o += al256(R * W * 4);
  w.sc = o; o += al256(R * 8);
  w.tok_tab = o; o += al256(ml * R * 4);
  w.par_tab = o; o += al256(ml * R * 4);
  w.n_live = o; o += al256((size_t)B * 4);
  w.done = o; o += al256((size_t)B * 4);
  w.ncomp = o; o += al256((size_t)B * 4);
  w.last_t = o; o += al256((size_t)B * 4);
  w.comp_score = o; o += al256(R * 8);
  w.comp_t = o; o += al256(R * 4);
  w.comp_par = o; o += al256(R * 4);
  w.rows = o; o += al256((size_t)B * ml * 4);
  w.total = o;
  return w;
}

// the joint search's part of the workspace, laid after the plain search's
struct CtcWs {
  size_t mx, lse, phi, gb, psi, delta, psic, total;
};

CtcWs ctc_ws(size_t base, int B, int T, int W) {
  CtcWs w;
  const size_t R = (size_t)B * W;
  size_t o = base;
  w.mx = o; o += al256((size_t)B * T * 4);
  w.lse = o; o += al256((size_t)B * T * 4);
  w.phi = o; o += al256(2 * R * T * 8);
  w.gb = o; o += al256(2 * R * T * 8);
  w.psi = o; o += al256(2 * R * 8);
  w.delta = o; o += al256(R * W * 8);
  w.psic = o; o += al256(R * W * 8);
  w.total = o;
  return w;
}

// the language model's part, laid after the joint search's
struct LmWs {
  size_t h, c, lg, lp, total;
};

LmWs lm_ws(size_t base, int B, int W, int V, int layers, int H) {
  LmWs w;
  const size_t R = (size_t)B * W;
  size_t o = base;
  w.h = o; o += al256(2 * R * layers * H * 4);
  w.c = o; o += al256(2 * R * layers * H * 4);
  w.lg = o; o += al256(R * V * 4);
  w.lp = o; o += al256(R * W * 4);
  w.total = o;
  return w;
}

constexpr LmWho kLmWho = {"att_beam_decode_lm", "att_beam_lm", "dims", "decoder", ""};

// ASR_OK, or the refusal with its reason in the error text
int beam_check(const asr_attdec_dims_t& d, int W, int V, int Y, int Dz, int max_len) {
  ASR_REQUIRE(d.B > 0 && d.T > 0 && d.E > 0 && d.A > 0 && d.C > 0 && d.K > 0 && d.D > 0 && V >= 2 &&
                  Y > 0 && Dz > 0 && max_len >= 0,
              ASR_ERR_ARG, "att_beam: bad dims");
  ASR_REQUIRE(d.K % 2 == 1, ASR_ERR_ARG, "att_beam: conv width must be odd");
  ASR_REQUIRE(W >= kMinBeam && W <= kMaxBeam, ASR_ERR_UNSUPPORTED,
              "att_beam: beam_width = %d outside [%d, %d]", W, kMinBeam, kMaxBeam);
  ASR_REQUIRE(d.C <= kMaxC, ASR_ERR_UNSUPPORTED, "att_beam: conv channels <= %d supported (C=%d)",
              kMaxC, d.C);
  const size_t la = attend_lds_floats(d.D, d.A, d.C, d.K, d.T) * 4;
  const size_t lc = ((size_t)Y + d.E + d.D) * 4;
  const size_t le = ((size_t)d.D + d.E + Dz + 8) * 4;
  ASR_REQUIRE(la <= kLdsLimit && lc <= kLdsLimit && le <= kLdsLimit, ASR_ERR_UNSUPPORTED,
              "att_beam: LDS need (attend %zu, cell %zu, expand %zu B) > %zu B", la, lc, le,
              kLdsLimit);
  return ASR_OK;
}

}  // namespace
}  // namespace asr

using namespace asr;

// plain; plain + the joint search's part; plain + the joint search's part + the
// LM's (whatever lambda is, so the LM's part has one place)
extern "C" size_t asr_att_beam_ws_bytes(const asr_attdec_dims_t* dims, int W, int V, int Y, int Dz,
                                        int max_len, const asr_att_beam_ex_t* ex) {
  if (!dims || beam_check(*dims, W, V, Y, Dz, max_len) != ASR_OK) return 0;
  const size_t plain = beam_ws(dims->B, dims->T, dims->E, dims->D, W, V, max_len).total;
  if (!ex || (!ex->ctc && !ex->lm)) return plain;
  const size_t joint = ctc_ws(plain, dims->B, dims->T, W).total;
  if (!ex->lm) return joint;
  if (lm_net_shape_check(ex->lm->layers, ex->lm->H, ex->lm->Y, kLmWho) != ASR_OK) return 0;
  return lm_ws(joint, dims->B, W, V, ex->lm->layers, ex->lm->H).total;
}

// ex null: an LSTM cell, no CTC term, no LM.  cell: which cell kernel steps the
// rows, the only difference it makes; ctc null or weight 0: the attention-only
// launches; lm null or weight 0: no LM launches
extern "C" int asr_att_beam_decode(const asr_attdec_dims_t* dims, const asr_att_beam_opts_t* o,
                                   const asr_att_beam_ex_t* ex, const float* enc,
                                   const float* enc_a, const int32_t* lens, const float* h0,
                                   void* workspace, size_t ws_bytes, long long* tokens,
                                   int32_t* hyp_lens, double* scores, float* aw, void* stream) {
  const int cell = ex ? ex->cell : ASR_ATT_BEAM_CELL_LSTM;
  const asr_att_beam_ctc_t* ctc = (ex && ex->ctc && ex->ctc->weight != 0.0) ? ex->ctc : nullptr;
  const asr_att_beam_lm_t* lm = (ex && ex->lm && ex->lm->weight != 0.0) ? ex->lm : nullptr;
  ASR_REQUIRE(dims && o, ASR_ERR_ARG, "att_beam_decode: dims / opts is null");
  ASR_REQUIRE(cell == ASR_ATT_BEAM_CELL_LSTM || cell == ASR_ATT_BEAM_CELL_GRU, ASR_ERR_ARG,
              "att_beam_decode: unknown cell %d", cell);
  const int rc = beam_check(*dims, o->W, o->V, o->Y, o->Dz, o->max_len);
  if (rc) return rc;
  ASR_REQUIRE(enc && enc_a && lens && workspace && tokens && hyp_lens && scores && aw &&
                  o->w_ih && o->w_hh && o->b_ih && o->b_hh && o->w_dec && o->w_conv && o->conv_w &&
                  o->v && o->w_d && o->w_c && o->w_fc && o->emb_w,
              ASR_ERR_ARG, "att_beam_decode: null pointer");
  ASR_REQUIRE(o->eos >= 0 && o->eos < o->V, ASR_ERR_ARG, "att_beam_decode: eos = %d outside [0, %d)",
              o->eos, o->V);
  ASR_REQUIRE(o->ld_ih >= (long long)o->Y + dims->E, ASR_ERR_ARG,
              "att_beam_decode: ld_ih = %lld < Y + E", o->ld_ih);
  ASR_REQUIRE(o->max_len > 0, ASR_ERR_ARG, "att_beam_decode: max_len = %d", o->max_len);
  const BeamWs w = beam_ws(dims->B, dims->T, dims->E, dims->D, o->W, o->V, o->max_len);
  const CtcWs cw = ctc_ws(w.total, dims->B, dims->T, o->W);
  if (ctc) {
    ASR_REQUIRE(ctc->ctc_logits, ASR_ERR_ARG, "att_beam_decode_ctc: ctc_logits is null");
    ASR_REQUIRE(ctc->weight > 0.0 && ctc->weight <= 1.0, ASR_ERR_ARG,
                "att_beam_decode_ctc: weight = %g outside (0, 1]", ctc->weight);
    // every class but <eos> maps into [0, Vc) and not onto blank
    const int hi = (o->eos == o->V - 1 ? o->V - 2 : o->V - 1) + ctc->label_offset;
    const int bl = ctc->blank - ctc->label_offset;   // the attention class that would hit blank
    ASR_REQUIRE(ctc->Vc >= 2 && ctc->label_offset >= 0 && hi < ctc->Vc && ctc->blank >= 0 &&
                    ctc->blank < ctc->Vc && (bl < 0 || bl >= o->V || bl == o->eos),
                ASR_ERR_ARG, "att_beam_decode_ctc: Vc = %d, blank = %d, label_offset = %d do not "
                "fit V = %d, eos = %d", ctc->Vc, ctc->blank, ctc->label_offset, o->V, o->eos);
  }
  LmWs lw = {};
  if (lm) {
    ASR_REQUIRE(lm->weight > 0.0, ASR_ERR_ARG, "att_beam_decode_lm: weight = %g is negative",
                lm->weight);
    const int lrc = lm_net_check(lm, o->V, kLmWho);
    if (lrc) return lrc;
    lw = lm_ws(cw.total, dims->B, o->W, o->V, lm->layers, lm->H);
  }
  const size_t need = lm ? lw.total : ctc ? cw.total : w.total;
  ASR_REQUIRE(ws_bytes >= need, ASR_ERR_WORKSPACE, "att_beam_decode: workspace %zu < %zu bytes",
              ws_bytes, need);
  ASR_REQUIRE(((uintptr_t)workspace & 255) == 0, ASR_ERR_ARG,
              "att_beam_decode: workspace not 256-B aligned");
  char* base = (char*)workspace;
  BeamP p;
  p.B = dims->B; p.T = dims->T; p.E = dims->E; p.A = dims->A; p.C = dims->C; p.K = dims->K;
  p.D = dims->D; p.W = o->W; p.V = o->V; p.Y = o->Y; p.Dz = o->Dz; p.max_len = o->max_len;
  p.min_len = o->min_len; p.eos = o->eos; p.sigmoid = dims->sigmoid_smoothing;
  p.emb_trans = o->emb_trans; p.sharpen = dims->sharpening; p.penalty = o->length_penalty;
  p.ld_ih = o->ld_ih;
  p.enc = enc; p.enc_a = enc_a; p.h0 = h0; p.lens = lens;
  p.w_ih = o->w_ih; p.w_hh = o->w_hh; p.b_ih = o->b_ih; p.b_hh = o->b_hh; p.w_dec = o->w_dec;
  p.w_conv = o->w_conv; p.conv_w = o->conv_w; p.v = o->v; p.w_d = o->w_d; p.b_d = o->b_d;
  p.w_c = o->w_c; p.b_c = o->b_c; p.w_fc = o->w_fc; p.b_fc = o->b_fc; p.emb_w = o->emb_w;
  p.h = (float*)(base + w.h); p.c = (float*)(base + w.c); p.ctx = (float*)(base + w.ctx);
  p.lg = (float*)(base + w.lg); p.awrec = (float*)(base + w.awrec);
  p.topv = (float*)(base + w.topv); p.topc = (int*)(base + w.topc); p.sc = (double*)(base + w.sc);
  p.tok_tab = (int*)(base + w.tok_tab); p.par_tab = (int*)(base + w.par_tab);
  p.n_live = (int*)(base + w.n_live); p.done = (int*)(base + w.done);
  p.ncomp = (int*)(base + w.ncomp); p.last_t = (int*)(base + w.last_t);
  p.comp_score = (double*)(base + w.comp_score); p.comp_t = (int*)(base + w.comp_t);
  p.comp_par = (int*)(base + w.comp_par); p.rows = (int*)(base + w.rows);

  hipStream_t s = (hipStream_t)stream;
  const size_t lds_cell = ((size_t)p.Y + p.E + p.D) * 4;
  const size_t lds_att = attend_lds_floats(p.D, p.A, p.C, p.K, p.T) * 4;
  const size_t lds_exp = ((size_t)p.D + p.E + p.Dz + 8) * 4;
  const dim3 rows(p.W, p.B);
  CtcP q = {};
  if (ctc) {
    q.lg = ctc->ctc_logits; q.Vc = ctc->Vc; q.blank = ctc->blank; q.off = ctc->label_offset;
    q.weight = ctc->weight;
    q.mx = (float*)(base + cw.mx); q.lse = (float*)(base + cw.lse);
    q.phi = (double*)(base + cw.phi); q.gb = (double*)(base + cw.gb);
    q.psi = (double*)(base + cw.psi); q.delta = (double*)(base + cw.delta);
    q.psic = (double*)(base + cw.psic);
  }
  LmP m = {};
  size_t lds_lmc = 0, lds_lms = 0;
  if (lm) {
    m.net = lm_net_from(lm);
    m.weight = lm->weight;
    m.h = (float*)(base + lw.h); m.c = (float*)(base + lw.c);
    m.lg = (float*)(base + lw.lg); m.lp = (float*)(base + lw.lp);
    lds_lmc = lm_cell_lds_floats(lm->Y, lm->H) * 4;
    lds_lms = ((size_t)lm->H + 8) * 4;
  }
  hipLaunchKernelGGL(beam_init, dim3(p.B), dim3(256), 0, s, p);
  ASR_LAUNCH_CHECK();
  if (ctc) {
    hipLaunchKernelGGL(beam_ctc_lse, dim3(p.T, p.B), dim3(LSE_THREADS), 0, s, p, q);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_ctc_empty, dim3(p.B), dim3(64), 0, s, p, q);
    ASR_LAUNCH_CHECK();
  }
  for (int t = 0; t < p.max_len; ++t) {
    if (t > 0) {
      if (cell == ASR_ATT_BEAM_CELL_GRU)
        hipLaunchKernelGGL(beam_cell_gru, rows, dim3(CELL_THREADS), lds_cell, s, t, p);
      else
        hipLaunchKernelGGL(beam_cell, rows, dim3(CELL_THREADS), lds_cell, s, t, p);
      ASR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(beam_attend, rows, dim3(ATT_THREADS), lds_att, s, t, p);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_expand, rows, dim3(EXP_THREADS), lds_exp, s, t, p);
    ASR_LAUNCH_CHECK();
    if (lm) {
      hipLaunchKernelGGL(beam_lm_cell, rows, dim3(LM_THREADS), lds_lmc, s, t, p, m);
      ASR_LAUNCH_CHECK();
      hipLaunchKernelGGL(beam_lm_score, rows, dim3(LM_THREADS), lds_lms, s, t, p, m);
      ASR_LAUNCH_CHECK();
    }
    if (ctc) {
      if (t > 0) {
        hipLaunchKernelGGL(beam_ctc_advance, rows, dim3(64), 0, s, t, p, q);
        ASR_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(beam_ctc_score, rows, dim3(SCORE_THREADS), 0, s, t, p, q);
      ASR_LAUNCH_CHECK();
      if (lm)
        hipLaunchKernelGGL(beam_select_ctc_lm, dim3(p.B), dim3(64), 0, s, t, p, q, m);
      else
        hipLaunchKernelGGL(beam_select_ctc, dim3(p.B), dim3(64), 0, s, t, p, q);
      ASR_LAUNCH_CHECK();
    } else {
      if (lm)
        hipLaunchKernelGGL(beam_select_lm, dim3(p.B), dim3(64), 0, s, t, p, m);
      else
        hipLaunchKernelGGL(beam_select, dim3(p.B), dim3(64), 0, s, t, p);
      ASR_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(beam_backtrack, dim3(p.B), dim3(BT_THREADS), 0, s, p, tokens, hyp_lens,
                     scores, aw);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
