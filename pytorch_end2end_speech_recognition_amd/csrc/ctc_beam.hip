// CTC prefix beam search on gfx950 (replaces the numpy BeamSearchDecoder,
// models/pytorch_v3/ctc/decoders/beam_search_decoder.py:22-124, alpha = beta = 0).
//
// The reference proposes every class for every beam entry (T x V x W Python
// iterations).  Here the W x V candidate set is never formed:
//   * an extension (p, c) that is not already a beam entry scores
//     lp[c] + base_p, base_p = p_b if c repeats p's last label, else
//     logaddexp(p_b, p_nb); per parent at most one class is the repeat, so only
//     the W + 1 best non-blank classes of a frame can reach the top W;
//   * an extension that IS a beam entry q (its parent is in the beam, c =
//     last(q)) is summed into q's p_nb whatever lp[c]'s rank: one gather per
//     entry, plus one for the blank.
//
// pass 1 (beam_rows_kernel): all B x T frames in parallel.  Per frame the
//   log-sum-exp (normalize) and the W + 1 best non-blank (value, class) pairs
//   in the order (value descending, class ascending): round k takes the
//   maximum of what lies strictly after round k - 1's pick in that order, so
//   nothing is marked and a NaN is never eligible.  One wave per frame up to
//   V = 128, one 256-thread work-group beyond.
// pass 2 (beam_search_kernel): one wave per utterance, the beam in LDS, the
//   prefixes as (parent, label) nodes in a global pool of T * W + 1 nodes.
//   Depth and a 64-bit hash of each beam entry's prefix and of its parent's
//   live with the entry.  Two beam entries never denote the same prefix: an
//   extension that equals an entry is found by depth and hash and CONFIRMED by
//   walking both parent chains until they meet -- node ids alone do not
//   identify a prefix, because a prefix that left the beam can come back under
//   a new id while a child of its old node is still in the beam.
//
// Order on exactly equal scores (independent of the launch geometry): stay
// entries before extensions; stays by their rank in the previous beam;
// extensions by the parent's rank, then by the class's place in the frame's
// (value descending, class ascending) list.
//
// With a language model and an insertion bonus (asr_ctc_beam_search_lm) -- the
// contract; alpha == 0 and beta == 0 at the public interface is the search
// above, by the launches above:
//   * inputs: logits or log-probabilities [B, T, V], lens, blank, W in [1, 64];
//     alpha >= 0 and beta, any finite float; an LM with exactly V classes,
//     <eos> included.  CTC class c != blank is LM class c - (c > blank); LM
//     <eos> is class V - 1 and is also the LM's start token.  With blank = 0 this
//     is the - 1 shift CTC.decode applies, so LM class c is the class decode()
//     returns, and the attention models' class c.
//   * score of a prefix l after t frames:
//       S_t(l) = log P_ctc,t(l) + alpha sum_i log p_lm(l_i | <eos>, l_<i) + beta |l|
//     with P_ctc,t = p_b + p_nb.  Every alignment of l crosses the edge
//     l_<i -> l_<=i exactly once, so the LM and bonus terms are added on the
//     extension edge and ride inside p_b / p_nb; stays and merges need no other
//     change.  An extension that equals a beam entry merges into that entry's
//     p_nb, as above, and carries its own parent's LM term.
//   * the beam after frame t holds the W best distinct prefixes by S_t; after
//     the last frame the entries are re-ranked by S_T(l) + alpha log
//     p_lm(<eos> | l), and that value is the returned score, in f32.  The LM
//     runs in f32 in both compute modes; all log-softmaxes, acoustic and LM, are
//     f32.
//   * candidate pruning: per parent p the W + 1 best non-blank classes by
//     lp_t[c] + alpha q_p[c] suffice (q_p: p's cached LM log-softmax row; value
//     descending, class ascending).  An extension of p scores that value + beta
//     + base_p; at most one class per parent is the repeat, whose base p_b is
//     below the total, so the other W of the list dominate every class below
//     it: the argument above, per parent.
//   * order on exactly equal scores, independent of the launch geometry: stays
//     before extensions; stays by their rank in the previous beam; extensions
//     by the parent's rank, then by the class's place in that parent's list.
//   * prefix identity stays depth + hash + confirmed chain walk.  A prefix that
//     leaves the beam and returns gets its LM state made again from its
//     parent's: correct by construction.
// Kernels: the acoustic log-sum-exp of all frames once (beam_rows_kernel, K =
// 0), lm_init_kernel, the root's LM step; per frame lm_topk_kernel (per entry),
// lm_select_kernel (per utterance) and, with an LM, lm_step_kernel (per extended
// entry: LSTM cell from the parent's state, output layer, log-softmax into the
// entry's row; the arithmetic is csrc/beam_lm.h's, shared with the attention
// search); lm_final_kernel.  No host read, no host synchronisation.
#include <limits.h>

#include "beam_lm.h"

namespace asr {
namespace {

constexpr int kMaxBeam = 64;
constexpr int kMaxTop = kMaxBeam + 1;
constexpr int kWaveModeMaxV = 128;

__device__ __forceinline__ void argmax_pair(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// log(exp(a) + exp(b)); -inf operands give no NaN
__device__ __forceinline__ float logaddexp_(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == neg_inf()) return m;
  return m + log1pf(expf(-fabsf(a - b)));
}

template <int WAVES>
__device__ __forceinline__ float group_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if (WAVES > 1) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v = fmaxf(v, sh[w]);
  }
  return v;
}

// the sum over a wave's lanes as this file has always formed it (an xor butterfly)
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int WAVES>
__device__ __forceinline__ float group_sum(float v, float* sh) {
  v = wave_sum_xor(v);
  if (WAVES > 1) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += sh[w];
  }
  return v;
}

template <int WAVES>
__device__ __forceinline__ void group_argmax(float& v, int& i, float* shv, int* shi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argmax_pair(v, i, ov, oi);
  }
  if (WAVES > 1) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = shv[0];
    i = shi[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) argmax_pair(v, i, shv[w], shi[w]);
  }
}

// WAVES waves share one frame; a block is 256 threads = 4 / WAVES frames.
template <int WAVES>
__global__ void __launch_bounds__(256) beam_rows_kernel(const float* __restrict__ logits,
                                                        long long st, long long sb, int T, int B,
                                                        int V, const int32_t* __restrict__ lens,
                                                        int blank, int K, int normalize,
                                                        float* __restrict__ lse_out,
                                                        float* __restrict__ topv,
                                                        int32_t* __restrict__ topc) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int tid = WAVES == 1 ? (threadIdx.x & 63) : threadIdx.x;
  constexpr int NTH = WAVES * 64;
  const long long f = WAVES == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (f >= (long long)B * T) return;      // the frames of one barrier group leave together
  const int b = (int)(f / T), t = (int)(f % T);
  if (t >= min(lens[b], T)) return;
  const float* x = logits + (long long)t * st + (long long)b * sb;

  float lse = 0.f;
  if (normalize) {
    float m = neg_inf();
    for (int v = tid; v < V; v += NTH) m = fmaxf(m, x[v]);
    m = group_max<WAVES>(m, shv);
    if (m > neg_inf()) {
      float s = 0.f;
      for (int v = tid; v < V; v += NTH) s += expf(x[v] - m);
      s = group_sum<WAVES>(s, shv);
      lse = m + logf(s);
    }
  }
  if (tid == 0) lse_out[f] = lse;

  float pv = __builtin_huge_valf();
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = neg_inf();
    int bi = INT_MAX;
    for (int v = tid; v < V; v += NTH) {
      const float xv = x[v];
      const bool after = xv < pv || (xv == pv && v > pi);   // false for a NaN
      if (after && v != blank) argmax_pair(bv, bi, xv, v);
    }
    group_argmax<WAVES>(bv, bi, shv, shi);
    const bool none = bi == INT_MAX;        // fewer than K eligible classes
    if (tid == 0) {
      topv[f * K + k] = none ? neg_inf() : bv;
      topc[f * K + k] = none ? -1 : bi;
    }
    if (none) { pv = neg_inf(); pi = INT_MAX; } else { pv = bv; pi = bi; }
  }
}

struct Node { int32_t parent, label; };

// floats as unsigned integers of the same order
__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// candidate key: score first, then the lower candidate index; 0 = no candidate
__device__ __forceinline__ unsigned long long make_key(float score, int idx) {
  if (!(score == score)) score = neg_inf();
  return ((unsigned long long)f2ord(score) << 32) | (unsigned)(0xffffffffu - (unsigned)idx);
}

__device__ __forceinline__ unsigned long long hash_push(unsigned long long h, int c) {
  h = (h ^ (unsigned long long)(unsigned)(c + 1)) * 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 29;
  return h;
}

// the prefixes of nodes a and b, known to have the same depth: equal?
__device__ __forceinline__ bool same_prefix(const Node* __restrict__ pool, int a, int b,
                                            int depth) {
  for (int d = 0; d < depth && a != b; ++d) {
    const Node na = pool[a], nb = pool[b];
    if (na.label != nb.label) return false;
    a = na.parent;
    b = nb.parent;
  }
  return a == b;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned lo = __shfl_xor((unsigned)v, o, 64);
    const unsigned long long ov = ((unsigned long long)hi << 32) | lo;
    v = ov > v ? ov : v;
  }
  return v;
}

// A beam in global memory: per row the entries in rank order, the node pool and,
// with an LM, the 2 W slots of h, c and q.  The LM search keeps it in its
// workspace between frames, a streaming session in its state between calls.
struct Beam {
  int32_t *n, *nnodes;           // [B]
  int32_t *node, *par, *last, *depth, *slot;   // [B][W]
  int32_t *src, *tok;            // [B][W] lm_step's work: parent slot (-1: zero state), LM token (-1: none)
  float *pb, *pnb;
  unsigned long long *hash, *phash;
  Node* pools;                   // [B][pool frames * W + 1]
  float *h, *c;                  // [B][2W][layers][H] by slot
  float* q;                      // [B][2W][V] by slot: the LM's log-softmax after the entry's prefix
};

// the root: the empty prefix, alone in row b's beam, in LM slot 0
__device__ __forceinline__ void beam_root(const Beam& m, int b, int W, int pool_frames) {
  const long long r = (long long)b * W;
  Node* pool = m.pools + (long long)b * ((long long)pool_frames * W + 1);
  pool[0].parent = 0;
  pool[0].label = -1;
  m.n[b] = 1; m.nnodes[b] = 1;
  m.node[r] = 0; m.par[r] = 0; m.last[r] = -1; m.depth[r] = 0; m.slot[r] = 0;
  m.pb[r] = 0.f; m.pnb[r] = neg_inf();
  m.hash[r] = 0; m.phash[r] = 0;
}

// A streaming session's search state (asr_ctc_beam_stream_*): the beam between
// calls, its node pools of max_frames * W + 1 nodes, and per row the frames
// consumed and a status word.
struct BeamState : Beam {
  int32_t *frames, *status;      // [B]
  int max_frames;
};

// The search over one row's Tb = min(lens[b], T) frames.  STREAM == false: from
// the empty prefix, the best entry's labels and score out.  STREAM == true
// (beam_stream_kernel): the beam comes from the session state S and goes back
// to it, one coalesced pass per array each way; lens[b] == 0 touches nothing.
template <bool STREAM>
__device__ __forceinline__ void beam_search_body(
    const float* __restrict__ logits, long long st, long long sb, int T, int V,
    const int32_t* __restrict__ lens, int blank, int W, const float* __restrict__ lse_in,
    const float* __restrict__ topv, const int32_t* __restrict__ topc, Node* __restrict__ pools,
    const BeamState* S, int32_t* __restrict__ hyps, int32_t* __restrict__ hyp_lens,
    float* __restrict__ scores) {
  // beam entry i < n, best first
  __shared__ int s_node[kMaxBeam], s_par[kMaxBeam], s_last[kMaxBeam], s_depth[kMaxBeam];
  __shared__ float s_pb[kMaxBeam], s_pnb[kMaxBeam], s_tot[kMaxBeam];
  __shared__ float s_npb[kMaxBeam], s_npnb[kMaxBeam];       // the entry after a stay
  __shared__ unsigned long long s_hash[kMaxBeam], s_phash[kMaxBeam];
  __shared__ float s_topv[kMaxTop];
  __shared__ int s_topc[kMaxTop];
  // candidates: [0, 64) stays, 64 + j * K + k = entry j extended by top class k
  __shared__ unsigned long long s_key[kMaxBeam + kMaxBeam * kMaxTop];

  const int b = blockIdx.x, lane = threadIdx.x;
  const int K = W + 1;
  const int Tb = max(0, min(lens[b], T));
  Node* pool = pools + (long long)b * ((long long)(STREAM ? S->max_frames : T) * W + 1);
  const long long r = (long long)b * W;
  int n = 1, nnodes = 1;
  if constexpr (STREAM) {
    if (Tb == 0) return;
    n = S->n[b];
    nnodes = S->nnodes[b];
    if (lane < n) {
      s_node[lane] = S->node[r + lane]; s_par[lane] = S->par[r + lane];
      s_last[lane] = S->last[r + lane]; s_depth[lane] = S->depth[r + lane];
      s_pb[lane] = S->pb[r + lane]; s_pnb[lane] = S->pnb[r + lane];
      s_hash[lane] = S->hash[r + lane]; s_phash[lane] = S->phash[r + lane];
    }
  } else {
    if (lane == 0) {
      pool[0].parent = 0;
      pool[0].label = -1;
      s_node[0] = 0; s_par[0] = 0; s_last[0] = -1; s_depth[0] = 0;
      s_pb[0] = 0.f; s_pnb[0] = neg_inf();
      s_hash[0] = 0; s_phash[0] = 0;
    }
  }
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    const float* x = logits + (long long)t * st + (long long)b * sb;
    const long long f = (long long)b * T + t;
    const float lse = lse_in[f];
    for (int k = lane; k < K; k += 64) {
      s_topv[k] = topv[f * K + k] - lse;
      s_topc[k] = topc[f * K + k];
    }
    const float lpb = x[blank] - lse;

    // A: entry `lane` stays: blank, repeat, and the extension that equals it
    int mpar = -1, my_last = -1;
    unsigned long long key = 0;
    if (lane < n) {
      my_last = s_last[lane];
      const float pb = s_pb[lane], pnb = s_pnb[lane];
      const float tot = logaddexp_(pb, pnb);
      const float npb = tot + lpb;
      float npnb = neg_inf();
      if (my_last >= 0) {
        const float xl = x[my_last] - lse;
        npnb = pnb + xl;
        const int dep = s_depth[lane] - 1, par = s_par[lane];
        const unsigned long long ph = s_phash[lane];
        for (int j = 0; j < n; ++j) {
          if (s_depth[j] != dep || s_hash[j] != ph) continue;
          if (!same_prefix(pool, s_node[j], par, dep)) continue;
          const float base = s_last[j] == my_last ? s_pb[j] : logaddexp_(s_pb[j], s_pnb[j]);
          npnb = logaddexp_(npnb, xl + base);
          mpar = j;
          break;                // beam entries are distinct prefixes: at most one
        }
      }
      s_tot[lane] = tot;
      s_npb[lane] = npb;
      s_npnb[lane] = npnb;
      key = make_key(logaddexp_(npb, npnb), lane);
    }
    s_key[lane] = key;
    __syncthreads();

    // B: extensions by the frame's W + 1 best non-blank classes
    for (int e = lane; e < n * K; e += 64) {
      const int j = e / K, k = e - j * K;
      const int c = s_topc[k];
      const float base = c == s_last[j] ? s_pb[j] : s_tot[j];
      s_key[kMaxBeam + e] = c >= 0 ? make_key(s_topv[k] + base, kMaxBeam + e) : 0ull;
    }
    __syncthreads();
    // C: ... except those counted in A
    if (mpar >= 0)
      for (int k = 0; k < K; ++k)
        if (s_topc[k] == my_last) s_key[kMaxBeam + mpar * K + k] = 0ull;
    __syncthreads();

    // D: the W best keys, one per round, round r's into lane r
    const int C = kMaxBeam + n * K;
    unsigned long long prev = ~0ull, mine = 0ull;
    int nsel = 0;
    for (int r = 0; r < W; ++r) {
      unsigned long long best = 0ull;
      for (int e = lane; e < C; e += 64) {
        const unsigned long long k = s_key[e];
        if (k < prev && k > best) best = k;
      }
      best = wave_max_u64(best);
      if (best == 0ull) break;
      if (lane == r) mine = best;
      prev = best;
      ++nsel;
    }

    // E: the new beam
    const bool sel = lane < nsel;
    const int idx = sel ? (int)(0xffffffffu - (unsigned)mine) : 0;
    const bool ext = sel && idx >= kMaxBeam;
    int e_node = 0, e_par = 0, e_last = -1, e_depth = 0;
    float e_pb = neg_inf(), e_pnb = neg_inf();
    unsigned long long e_hash = 0, e_phash = 0;
    if (sel && !ext) {
      e_node = s_node[idx]; e_par = s_par[idx]; e_last = s_last[idx]; e_depth = s_depth[idx];
      e_pb = s_npb[idx]; e_pnb = s_npnb[idx];
      e_hash = s_hash[idx]; e_phash = s_phash[idx];
    }
    const unsigned long long emask = __ballot(ext);
    if (ext) {
      const int e = idx - kMaxBeam;
      const int j = e / K, k = e - j * K;
      e_node = nnodes + __popcll(emask & ((1ull << lane) - 1ull));
      e_par = s_node[j];
      e_last = s_topc[k];
      e_depth = s_depth[j] + 1;
      e_pnb = ord2f((unsigned)(mine >> 32));
      e_phash = s_hash[j];
      e_hash = hash_push(e_phash, e_last);
      pool[e_node].parent = e_par;
      pool[e_node].label = e_last;
    }
    nnodes += __popcll(emask);
    n = nsel;
    __syncthreads();
    if (sel) {
      s_node[lane] = e_node; s_par[lane] = e_par; s_last[lane] = e_last; s_depth[lane] = e_depth;
      s_pb[lane] = e_pb; s_pnb[lane] = e_pnb;
      s_hash[lane] = e_hash; s_phash[lane] = e_phash;
    }
    __syncthreads();           // also orders the pool stores before the next frame's walks
  }

  if constexpr (STREAM) {
    if (lane < n) {
      S->node[r + lane] = s_node[lane]; S->par[r + lane] = s_par[lane];
      S->last[r + lane] = s_last[lane]; S->depth[r + lane] = s_depth[lane];
      S->pb[r + lane] = s_pb[lane]; S->pnb[r + lane] = s_pnb[lane];
      S->hash[r + lane] = s_hash[lane]; S->phash[r + lane] = s_phash[lane];
    }
    if (lane == 0) { S->n[b] = n; S->nnodes[b] = nnodes; }
  } else if (lane == 0) {
    const int d = s_depth[0];
    int node = s_node[0];
    int32_t* out = hyps + (long long)b * T;
    for (int k = d - 1; k >= 0; --k) {       // d <= Tb <= T
      const Node nd = pool[node];
      out[k] = nd.label;
      node = nd.parent;
    }
    hyp_lens[b] = d;
    scores[b] = logaddexp_(s_pb[0], s_pnb[0]);
  }
}

__global__ void __launch_bounds__(64) beam_search_kernel(
    const float* __restrict__ logits, long long st, long long sb, int T, int V,
    const int32_t* __restrict__ lens, int blank, int W, const float* __restrict__ lse_in,
    const float* __restrict__ topv, const int32_t* __restrict__ topc, Node* __restrict__ pools,
    int32_t* __restrict__ hyps, int32_t* __restrict__ hyp_lens, float* __restrict__ scores) {
  beam_search_body<false>(logits, st, sb, T, V, lens, blank, W, lse_in, topv, topc, pools,
                          nullptr, hyps, hyp_lens, scores);
}

// ------------------------------------------- the search with a language model
struct LmP : Beam {              // the beam between frames
  // the call
  const float* logits;
  long long st, sb;
  int T, B, V, blank, W;
  int poolT;                     // the frames a row's node pool is sized for (T; a session's max_frames)
  const int32_t* lens;
  float alpha, beta;
  int has_lm;                    // 0: no LM term anywhere, q / h / c are not touched
  LmNet net;                     // the language model; net.V is V
  // workspace
  const float* lse;              // [B][T]
  float* topv;                   // [B][W][W + 1] per parent: lp + alpha q, best first
  int32_t* topc;
};

__device__ __forceinline__ int lm_class(int c, int blank) { return c - (c > blank ? 1 : 0); }

// the root: the empty prefix in slot 0, whose LM state lm_step(t = -1) makes
// from the zero state and <eos>
__global__ void __launch_bounds__(64) lm_init_kernel(LmP p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r = (long long)b * p.W;
  if (lane < p.W) {
    p.tok[r + lane] = lane == 0 ? p.V - 1 : -1;
    p.src[r + lane] = -1;
  }
  if (lane == 0) beam_root(p, b, p.W, p.poolT);
}

// Per beam entry (parent) the W + 1 best non-blank classes by lp_t[c] + alpha
// q_p[c] in the order (value descending, class ascending), as beam_rows_kernel
// ranks a frame.  WAVES waves share one entry; a block is 4 / WAVES entries.
template <int WAVES>
__global__ void __launch_bounds__(256) lm_topk_kernel(int t, LmP p) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int tid = WAVES == 1 ? (threadIdx.x & 63) : threadIdx.x;
  constexpr int NTH = WAVES * 64;
  const long long e = WAVES == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (e >= (long long)p.B * p.W) return;  // the waves of one barrier group leave together
  const int b = (int)(e / p.W), i = (int)(e % p.W);
  if (t >= min(p.lens[b], p.T) || i >= p.n[b]) return;
  const float* x = p.logits + (long long)t * p.st + (long long)b * p.sb;
  const float lse = p.lse[(long long)b * p.T + t];
  const float* q = p.has_lm ? p.q + ((long long)b * 2 * p.W + p.slot[e]) * p.V : nullptr;
  const int K = p.W + 1, V = p.V, blank = p.blank;
  const float alpha = p.alpha;

  float pv = __builtin_huge_valf();
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = neg_inf();
    int bi = INT_MAX;
    for (int v = tid; v < V; v += NTH) {
      if (v == blank) continue;
      float xv = x[v] - lse;
      if (q) xv += alpha * q[lm_class(v, blank)];
      const bool after = xv < pv || (xv == pv && v > pi);   // false for a NaN
      if (after) argmax_pair(bv, bi, xv, v);
    }
    group_argmax<WAVES>(bv, bi, shv, shi);
    const bool none = bi == INT_MAX;        // fewer than K eligible classes
    if (tid == 0) {
      p.topv[e * K + k] = none ? neg_inf() : bv;
      p.topc[e * K + k] = none ? -1 : bi;
    }
    if (none) { pv = neg_inf(); pi = INT_MAX; } else { pv = bv; pi = bi; }
  }
}

// One frame of beam_search_kernel's steps A-E with per-parent class lists and
// the LM / insertion terms on the extension edge.  The beam lives in global
// memory between frames.  Every new entry gets its LM slot: a stay keeps its
// own, an extension takes one that no entry of the previous beam holds (there
// are 2 W, the previous beam holds at most W), so lm_step reads parents' slots
// and writes children's without a copy and without a race.
__global__ void __launch_bounds__(64) lm_select_kernel(int t, LmP p) {
  __shared__ int s_node[kMaxBeam], s_par[kMaxBeam], s_last[kMaxBeam], s_depth[kMaxBeam];
  __shared__ int s_slot[kMaxBeam];
  __shared__ float s_pb[kMaxBeam], s_pnb[kMaxBeam], s_tot[kMaxBeam];
  __shared__ float s_npb[kMaxBeam], s_npnb[kMaxBeam];
  __shared__ unsigned long long s_hash[kMaxBeam], s_phash[kMaxBeam];
  __shared__ int s_used[2 * kMaxBeam], s_free[2 * kMaxBeam];
  __shared__ unsigned long long s_key[kMaxBeam + kMaxBeam * kMaxTop];

  const int b = blockIdx.x, lane = threadIdx.x;
  const int W = p.W, K = W + 1;
  if (t >= min(p.lens[b], p.T)) return;
  Node* pool = p.pools + (long long)b * ((long long)p.poolT * W + 1);
  const long long r = (long long)b * W;
  const int n = p.n[b], nnodes = p.nnodes[b];
  const float* topv = p.topv + r * K;
  const int32_t* topc = p.topc + r * K;
  const float* qb = p.has_lm ? p.q + (long long)b * 2 * W * p.V : nullptr;

  s_used[lane] = 0;
  s_used[lane + 64] = 0;
  if (lane < n) {
    s_node[lane] = p.node[r + lane]; s_par[lane] = p.par[r + lane];
    s_last[lane] = p.last[r + lane]; s_depth[lane] = p.depth[r + lane];
    s_slot[lane] = p.slot[r + lane];
    s_pb[lane] = p.pb[r + lane]; s_pnb[lane] = p.pnb[r + lane];
    s_hash[lane] = p.hash[r + lane]; s_phash[lane] = p.phash[r + lane];
  }
  __syncthreads();
  if (lane < n) s_used[s_slot[lane]] = 1;

  const float* x = p.logits + (long long)t * p.st + (long long)b * p.sb;
  const float lse = p.lse[(long long)b * p.T + t];
  const float lpb = x[p.blank] - lse;

  // A: entry `lane` stays: blank, repeat, and the extension that equals it
  // (which carries ITS parent's LM term and the bonus)
  int mpar = -1, my_last = -1;
  unsigned long long key = 0;
  if (lane < n) {
    my_last = s_last[lane];
    const float pb = s_pb[lane], pnb = s_pnb[lane];
    const float tot = logaddexp_(pb, pnb);
    const float npb = tot + lpb;
    float npnb = neg_inf();
    if (my_last >= 0) {
      const float xl = x[my_last] - lse;
      npnb = pnb + xl;
      const int dep = s_depth[lane] - 1, par = s_par[lane];
      const unsigned long long ph = s_phash[lane];
      for (int j = 0; j < n; ++j) {
        if (s_depth[j] != dep || s_hash[j] != ph) continue;
        if (!same_prefix(pool, s_node[j], par, dep)) continue;
        const float base = s_last[j] == my_last ? s_pb[j] : logaddexp_(s_pb[j], s_pnb[j]);
        float edge = xl;
        if (qb) edge += p.alpha * qb[(long long)s_slot[j] * p.V + lm_class(my_last, p.blank)];
        npnb = logaddexp_(npnb, edge + p.beta + base);
        mpar = j;
        break;                // beam entries are distinct prefixes: at most one
      }
    }
    s_tot[lane] = tot;
    s_npb[lane] = npb;
    s_npnb[lane] = npnb;
    key = make_key(logaddexp_(npb, npnb), lane);
  }
  s_key[lane] = key;
  __syncthreads();

  // the slots no entry of this beam holds, in ascending order
  {
    const bool f0 = lane < 2 * W && !s_used[lane];
    const bool f1 = lane + 64 < 2 * W && !s_used[lane + 64];
    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (f0) s_free[__popcll(m0 & below)] = lane;
    if (f1) s_free[__popcll(m0) + __popcll(m1 & below)] = lane + 64;
  }

  // B: extensions by each parent's W + 1 best non-blank classes
  for (int e = lane; e < n * K; e += 64) {
    const int j = e / K;
    const int c = topc[e];
    const float base = c == s_last[j] ? s_pb[j] : s_tot[j];
    s_key[kMaxBeam + e] = c >= 0 ? make_key(topv[e] + p.beta + base, kMaxBeam + e) : 0ull;
  }
  __syncthreads();
  // C: ... except those counted in A
  if (mpar >= 0)
    for (int k = 0; k < K; ++k)
      if (topc[mpar * K + k] == my_last) s_key[kMaxBeam + mpar * K + k] = 0ull;
  __syncthreads();

  // D: the W best keys, one per round, round r's into lane r
  const int C = kMaxBeam + n * K;
  unsigned long long prev = ~0ull, mine = 0ull;
  int nsel = 0;
  for (int rd = 0; rd < W; ++rd) {
    unsigned long long best = 0ull;
    for (int e = lane; e < C; e += 64) {
      const unsigned long long k = s_key[e];
      if (k < prev && k > best) best = k;
    }
    best = wave_max_u64(best);
    if (best == 0ull) break;
    if (lane == rd) mine = best;
    prev = best;
    ++nsel;
  }

  // E: the new beam, and lm_step's work list
  const bool sel = lane < nsel;
  const int idx = sel ? (int)(0xffffffffu - (unsigned)mine) : 0;
  const bool ext = sel && idx >= kMaxBeam;
  const unsigned long long emask = __ballot(ext);
  if (sel && !ext) {
    p.node[r + lane] = s_node[idx]; p.par[r + lane] = s_par[idx];
    p.last[r + lane] = s_last[idx]; p.depth[r + lane] = s_depth[idx];
    p.slot[r + lane] = s_slot[idx];
    p.pb[r + lane] = s_npb[idx]; p.pnb[r + lane] = s_npnb[idx];
    p.hash[r + lane] = s_hash[idx]; p.phash[r + lane] = s_phash[idx];
  }
  if (ext) {
    const int e = idx - kMaxBeam;
    const int j = e / K;
    const int ord = __popcll(emask & ((1ull << lane) - 1ull));
    const int e_node = nnodes + ord;
    const int e_last = topc[e];
    const unsigned long long e_phash = s_hash[j];
    pool[e_node].parent = s_node[j];
    pool[e_node].label = e_last;
    p.node[r + lane] = e_node; p.par[r + lane] = s_node[j];
    p.last[r + lane] = e_last; p.depth[r + lane] = s_depth[j] + 1;
    p.slot[r + lane] = s_free[ord];
    p.pb[r + lane] = neg_inf(); p.pnb[r + lane] = ord2f((unsigned)(mine >> 32));
    p.hash[r + lane] = hash_push(e_phash, e_last); p.phash[r + lane] = e_phash;
    p.src[r + lane] = s_slot[j];
  }
  if (lane < W) p.tok[r + lane] = ext ? lm_class(topc[idx - kMaxBeam], p.blank) : -1;
  if (lane == 0) {
    p.n[b] = nsel;
    p.nnodes[b] = nnodes + __popcll(emask);
  }
}

// The LM after an extended entry's new token: the stacked LSTM from the
// parent's slot, then the output layer and its f32 log-softmax into the entry's
// row of q.  Entries that stayed (most of them, at most frames) leave at once.
// t = -1: the root.
__global__ void __launch_bounds__(LM_THREADS) lm_step_kernel(int t, LmP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ float red[4];
  const int i = blockIdx.x, b = blockIdx.y;
  if (t >= 0 && (t >= min(p.lens[b], p.T) || i >= p.n[b])) return;
  const long long r = (long long)b * p.W + i;
  const int tok = p.tok[r];
  if (tok < 0) return;
  const int src = p.src[r], dst = p.slot[r], V = p.V;
  const long long LH = (long long)p.net.layers * p.net.H;
  const long long so = ((long long)b * 2 * p.W + dst) * LH;
  const long long sp = ((long long)b * 2 * p.W + max(src, 0)) * LH;
  const float* h = lm_lstm_step(p.net, tok, src >= 0 ? p.h + sp : nullptr,
                                src >= 0 ? p.c + sp : nullptr, p.h + so, p.c + so, sm);
  float* q = p.q + ((long long)b * 2 * p.W + dst) * V;
  float mx, lse;
  lm_output_lse<wave_sum_xor>(p.net, h, q, red, mx, lse);
  for (int v = threadIdx.x; v < V; v += LM_THREADS) q[v] = (q[v] - mx) - lse;
}

// After the last frame: the entries re-ranked by S_T + alpha lp_lm(<eos> | l)
// (ties: the better rank), the best one's labels and that score.
__global__ void __launch_bounds__(64) lm_final_kernel(LmP p, int32_t* __restrict__ hyps,
                                                      int32_t* __restrict__ hyp_lens,
                                                      float* __restrict__ scores) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r = (long long)b * p.W;
  const int n = p.n[b];
  float s = neg_inf();
  unsigned long long key = 0;
  if (lane < n) {
    s = logaddexp_(p.pb[r + lane], p.pnb[r + lane]);
    if (p.has_lm)
      s += p.alpha * p.q[((long long)b * 2 * p.W + p.slot[r + lane]) * p.V + (p.V - 1)];
    key = make_key(s, lane);
  }
  const unsigned long long best = wave_max_u64(key);
  if (lane < n && key == best) {           // keys are distinct: one lane
    const Node* pool = p.pools + (long long)b * ((long long)p.poolT * p.W + 1);
    const int d = p.depth[r + lane];
    int node = p.node[r + lane];
    int32_t* out = hyps + (long long)b * p.T;
    for (int k = d - 1; k >= 0; --k) {     // d <= lens[b] <= T
      const Node nd = pool[node];
      out[k] = nd.label;
      node = nd.parent;
    }
    hyp_lens[b] = d;
    scores[b] = s;
  }
}

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct BeamWs { size_t lse, topv, topc, pool, total; };

inline BeamWs beam_ws(int T, int B, int V, int W) {
  BeamWs w;
  const size_t frames = (size_t)B * T, K = (size_t)W + 1;
  w.lse = 0;
  w.topv = align16(frames * sizeof(float));
  w.topc = w.topv + align16(frames * K * sizeof(float));
  w.pool = w.topc + align16(frames * K * sizeof(int32_t));
  w.total = w.pool + align16((size_t)B * ((size_t)T * W + 1) * sizeof(Node));
  return w;
}

inline bool beam_args_ok(int T, int B, int V, int W) {
  return T > 0 && B > 0 && V >= 2 && W >= 1 && W <= kMaxBeam;
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_ctc_beam_ws_bytes(int T, int B, int V, int beam_width) {
  if (!beam_args_ok(T, B, V, beam_width)) return 0;
  return beam_ws(T, B, V, beam_width).total;
}

// what both searches ask of their arguments, and of the workspace once its size is known
static int beam_args_check(const char* who, bool pointers, int T, int B, int V, int blank,
                           int beam_width) {
  ASR_REQUIRE(pointers, ASR_ERR_ARG, "%s: null pointer", who);
  ASR_REQUIRE(T > 0 && B > 0, ASR_ERR_ARG, "%s: bad shape", who);
  ASR_REQUIRE(V >= 2, ASR_ERR_ARG, "%s: V = %d < 2", who, V);
  ASR_REQUIRE(beam_width >= 1 && beam_width <= kMaxBeam, ASR_ERR_ARG,
              "%s: beam_width = %d outside [1, %d]", who, beam_width, kMaxBeam);
  ASR_REQUIRE(blank >= 0 && blank < V, ASR_ERR_ARG, "%s: blank = %d outside [0, %d)", who, blank, V);
  return ASR_OK;
}

static int beam_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  ASR_REQUIRE(ws_bytes >= need, ASR_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes,
              need);
  ASR_REQUIRE(((uintptr_t)ws & 15) == 0, ASR_ERR_ARG, "%s: workspace not 16-B aligned", who);
  return ASR_OK;
}

// pass 1: the log-sum-exp of every frame and its K best non-blank classes (K == 0: none)
static void launch_rows(const float* logits, long long stride_t, long long stride_b, int T, int B,
                        int V, const int32_t* lens, int blank, int K, int normalize, float* lse,
                        float* topv, int32_t* topc, hipStream_t s) {
  const long long frames = (long long)B * T;
  if (V <= kWaveModeMaxV) {
    hipLaunchKernelGGL(beam_rows_kernel<1>, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s,
                       logits, stride_t, stride_b, T, B, V, lens, blank, K, normalize, lse, topv,
                       topc);
  } else {
    hipLaunchKernelGGL(beam_rows_kernel<4>, dim3((unsigned)frames), dim3(256), 0, s, logits,
                       stride_t, stride_b, T, B, V, lens, blank, K, normalize, lse, topv, topc);
  }
}

static int beam_launch(const float* logits, long long stride_t, long long stride_b, int T, int B,
                       int V, const int32_t* lens, int blank, int beam_width, int normalize,
                       void* ws, size_t ws_bytes, int32_t* hyps, int32_t* hyp_lens, float* scores,
                       bool search, void* stream) {
  const char* who = "ctc_beam_search";
  int rc = beam_args_check(who, logits && lens && ws && (!search || (hyps && hyp_lens && scores)),
                           T, B, V, blank, beam_width);
  if (rc != ASR_OK) return rc;
  const BeamWs w = beam_ws(T, B, V, beam_width);
  if ((rc = beam_ws_check(who, ws, ws_bytes, w.total)) != ASR_OK) return rc;
  char* base = (char*)ws;
  float* lse = (float*)(base + w.lse);
  float* topv = (float*)(base + w.topv);
  int32_t* topc = (int32_t*)(base + w.topc);
  Node* pool = (Node*)(base + w.pool);
  hipStream_t s = (hipStream_t)stream;
  launch_rows(logits, stride_t, stride_b, T, B, V, lens, blank, beam_width + 1, normalize, lse, topv,
              topc, s);
  ASR_LAUNCH_CHECK();
  if (!search) return ASR_OK;
  hipLaunchKernelGGL(beam_search_kernel, dim3(B), dim3(64), 0, s, logits, stride_t, stride_b, T, V,
                     lens, blank, beam_width, lse, topv, topc, pool, hyps, hyp_lens, scores);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_ctc_beam_search(const float* logits, long long stride_t, long long stride_b,
                                   int T, int B, int V, const int32_t* lens, int blank,
                                   int beam_width, int normalize, void* ws, size_t ws_bytes,
                                   int32_t* hyps, int32_t* hyp_lens, float* scores, void* stream) {
  return beam_launch(logits, stride_t, stride_b, T, B, V, lens, blank, beam_width, normalize, ws,
                     ws_bytes, hyps, hyp_lens, scores, true, stream);
}

extern "C" int asr_ctc_beam_rows(const float* logits, long long stride_t, long long stride_b, int T,
                                 int B, int V, const int32_t* lens, int blank, int beam_width,
                                 int normalize, void* ws, size_t ws_bytes, void* stream) {
  return beam_launch(logits, stride_t, stride_b, T, B, V, lens, blank, beam_width, normalize, ws,
                     ws_bytes, nullptr, nullptr, nullptr, false, stream);
}

// ------------------------------------------- the search with a language model
namespace asr {
namespace {

// `bytes` more from the running offset o, the next array 16-B aligned: where they start
inline size_t take(size_t& o, size_t bytes) {
  const size_t at = o;
  o += align16(bytes);
  return at;
}

// Where the arrays of a Beam lie from their base.  The order and the alignment
// are part of a session state's format.
struct BeamLayout {
  size_t n, nnodes, node, par, last, depth, slot, src, tok, pb, pnb, hash, phash, pool, h, c, q;
};

// from the running offset o; layers == 0: no language model, no h / c / q
inline BeamLayout beam_layout(size_t& o, int pool_frames, int B, int V, int W, int layers, int H) {
  BeamLayout w;
  const size_t R = (size_t)B * W;
  w.n = take(o, (size_t)B * sizeof(int32_t));
  w.nnodes = take(o, (size_t)B * sizeof(int32_t));
  w.node = take(o, R * sizeof(int32_t));
  w.par = take(o, R * sizeof(int32_t));
  w.last = take(o, R * sizeof(int32_t));
  w.depth = take(o, R * sizeof(int32_t));
  w.slot = take(o, R * sizeof(int32_t));
  w.src = take(o, R * sizeof(int32_t));
  w.tok = take(o, R * sizeof(int32_t));
  w.pb = take(o, R * sizeof(float));
  w.pnb = take(o, R * sizeof(float));
  w.hash = take(o, R * sizeof(unsigned long long));
  w.phash = take(o, R * sizeof(unsigned long long));
  w.pool = take(o, (size_t)B * ((size_t)pool_frames * W + 1) * sizeof(Node));
  w.h = take(o, 2 * R * (size_t)layers * H * sizeof(float));
  w.c = take(o, 2 * R * (size_t)layers * H * sizeof(float));
  w.q = take(o, layers > 0 ? 2 * R * (size_t)V * sizeof(float) : 0);
  return w;
}

inline void beam_bind(Beam& m, void* mem, const BeamLayout& w) {
  char* base = (char*)mem;
  m.n = (int32_t*)(base + w.n); m.nnodes = (int32_t*)(base + w.nnodes);
  m.node = (int32_t*)(base + w.node); m.par = (int32_t*)(base + w.par);
  m.last = (int32_t*)(base + w.last); m.depth = (int32_t*)(base + w.depth);
  m.slot = (int32_t*)(base + w.slot); m.src = (int32_t*)(base + w.src);
  m.tok = (int32_t*)(base + w.tok);
  m.pb = (float*)(base + w.pb); m.pnb = (float*)(base + w.pnb);
  m.hash = (unsigned long long*)(base + w.hash); m.phash = (unsigned long long*)(base + w.phash);
  m.pools = (Node*)(base + w.pool);
  m.h = (float*)(base + w.h); m.c = (float*)(base + w.c); m.q = (float*)(base + w.q);
}

struct LmBeamWs {
  size_t lse, topv, topc;
  BeamLayout beam;
  size_t total;
};

inline LmBeamWs lm_beam_ws(int T, int B, int V, int W, int layers, int H) {
  LmBeamWs w;
  const size_t frames = (size_t)B * T, K = (size_t)W + 1, R = (size_t)B * W;
  size_t o = 0;
  w.lse = take(o, frames * sizeof(float));
  w.topv = take(o, R * K * sizeof(float));
  w.topc = take(o, R * K * sizeof(int32_t));
  w.beam = beam_layout(o, T, B, V, W, layers, H);
  w.total = o;
  return w;
}

// What the searches with an LM ask of it; on ASR_OK *lm is null where the LM
// term is absent (no LM, or weight 0).
int lm_args_check(const char* who, const asr_att_beam_lm_t** lm, int V, const LmWho& lw) {
  if (!*lm) return ASR_OK;
  ASR_REQUIRE((*lm)->weight >= 0.0 && (*lm)->weight <= 3.0e38, ASR_ERR_ARG,
              "%s: weight = %g is negative or not finite", who, (*lm)->weight);
  const int rc = lm_net_check(*lm, V, lw);
  if (rc != ASR_OK) return rc;
  if ((*lm)->weight == 0.0) *lm = nullptr;
  return ASR_OK;
}

// The frames [0, T) of the search on p's beam, three launches per frame (two
// without an LM): the per-parent class lists, the new beam, the LM's step for
// the entries that were extended.
int lm_launch_frames(const LmP& p, int T, const asr_att_beam_lm_t* lm, hipStream_t s) {
  const size_t lds_step = lm ? lm_cell_lds_floats(lm->Y, lm->H) * 4 : 0;
  const long long entries = (long long)p.B * p.W;
  for (int t = 0; t < T; ++t) {
    if (p.V <= kWaveModeMaxV)
      hipLaunchKernelGGL(lm_topk_kernel<1>, dim3((unsigned)((entries + 3) / 4)), dim3(256), 0, s,
                         t, p);
    else
      hipLaunchKernelGGL(lm_topk_kernel<4>, dim3((unsigned)entries), dim3(256), 0, s, t, p);
    hipLaunchKernelGGL(lm_select_kernel, dim3(p.B), dim3(64), 0, s, t, p);
    if (lm)
      hipLaunchKernelGGL(lm_step_kernel, dim3(p.W, p.B), dim3(LM_THREADS), lds_step, s, t, p);
    ASR_LAUNCH_CHECK();
  }
  return ASR_OK;
}

// the root's LM state, from the zero state and <eos> (lm_step at t = -1)
int lm_launch_root(const LmP& p, const asr_att_beam_lm_t* lm, hipStream_t s) {
  hipLaunchKernelGGL(lm_step_kernel, dim3(1, p.B), dim3(LM_THREADS),
                     lm_cell_lds_floats(lm->Y, lm->H) * 4, s, -1, p);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

constexpr LmWho kLmWho = {"ctc_beam_search_lm", "ctc_beam_search_lm", "LM dims", "CTC head",
                          " (blank included; <eos> takes the blank's place)"};

}  // namespace
}  // namespace asr

extern "C" size_t asr_ctc_beam_lm_ws_bytes(int T, int B, int V, int beam_width, int lm_layers,
                                           int lm_H, int lm_Y) {
  if (!beam_args_ok(T, B, V, beam_width)) return 0;
  if (lm_layers == 0) return lm_beam_ws(T, B, V, beam_width, 0, 0).total;
  if (lm_net_shape_check(lm_layers, lm_H, lm_Y, kLmWho) != ASR_OK) return 0;
  return lm_beam_ws(T, B, V, beam_width, lm_layers, lm_H).total;
}

extern "C" int asr_ctc_beam_search_lm(const float* logits, long long stride_t, long long stride_b,
                                      int T, int B, int V, const int32_t* lens, int blank,
                                      int beam_width, int normalize, const asr_att_beam_lm_t* lm,
                                      double beta, void* ws, size_t ws_bytes, int32_t* hyps,
                                      int32_t* hyp_lens, float* scores, void* stream) {
  const char* who = "ctc_beam_search_lm";
  int rc = beam_args_check(who, logits && lens && ws && hyps && hyp_lens && scores, T, B, V, blank,
                           beam_width);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(beta == beta && fabs(beta) <= 3.0e38, ASR_ERR_ARG,
              "ctc_beam_search_lm: beta = %g is not finite", beta);
  if ((rc = lm_args_check(who, &lm, V, kLmWho)) != ASR_OK) return rc;
  const int W = beam_width;
  const LmBeamWs w = lm_beam_ws(T, B, V, W, lm ? lm->layers : 0, lm ? lm->H : 0);
  if ((rc = beam_ws_check(who, ws, ws_bytes, w.total)) != ASR_OK) return rc;
  char* base = (char*)ws;
  LmP p = {};
  p.logits = logits; p.st = stride_t; p.sb = stride_b;
  p.T = T; p.B = B; p.V = V; p.blank = blank; p.W = W; p.poolT = T; p.lens = lens;
  p.alpha = lm ? (float)lm->weight : 0.f;
  p.beta = (float)beta;
  p.has_lm = lm ? 1 : 0;
  if (lm) p.net = lm_net_from(lm);
  float* lse = (float*)(base + w.lse);
  p.lse = lse;
  p.topv = (float*)(base + w.topv); p.topc = (int32_t*)(base + w.topc);
  beam_bind(p, base, w.beam);

  hipStream_t s = (hipStream_t)stream;
  // the acoustic log-sum-exp of every frame, once (K = 0: no class ranking)
  launch_rows(logits, stride_t, stride_b, T, B, V, lens, blank, 0, normalize, lse, nullptr, nullptr,
              s);
  ASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(lm_init_kernel, dim3(B), dim3(64), 0, s, p);
  ASR_LAUNCH_CHECK();
  if (lm && (rc = lm_launch_root(p, lm, s)) != ASR_OK) return rc;
  if ((rc = lm_launch_frames(p, T, lm, s)) != ASR_OK) return rc;
  hipLaunchKernelGGL(lm_final_kernel, dim3(B), dim3(64), 0, s, p, hyps, hyp_lens, scores);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

// ------------------------------------------------- the search, chunk by chunk
// asr_ctc_beam_stream_*: the two searches above with their state kept between
// calls, so that a call costs O(chunk).  The result of the call that carries a
// row's `final` flag equals, bit for bit, the whole-utterance search on the
// concatenated frames, for any chunking:
//   * pass 1 (log-sum-exp, class lists) is per frame;
//   * a frame of the search is the same f32 operations in the same order, on
//     the previous beam in rank order (the state holds it in rank order, with
//     both hashes, the depths, the LM slots and the pool's node numbering);
//   * the order on equal scores depends on the previous beam's rank order and
//     the frame's lists only.
// Plain search (no LM, beta == 0): beam_stream_prep_kernel, pass 1 of the chunk,
// beam_stream_kernel (beam_search_kernel's frame loop between a load and a
// store of the state), beam_stream_out_kernel.  Otherwise: prep, the chunk's
// log-sum-exps, per chunk frame lm_topk / lm_select / lm_step on the state's
// arrays (the kernels above, unchanged), out.
namespace asr {
namespace {

constexpr int kStreamFull = 1;       // status: frames were dropped at max_frames
constexpr int kStreamInvalid = 2;    // status: the row's state is not one reset / feed left

// the state buffer: the frame counts, the status words, the beam
struct StreamLayout {
  size_t frames, status;
  BeamLayout beam;
  size_t total;
};

inline StreamLayout stream_layout(int max_frames, int B, int V, int W, int layers, int H) {
  StreamLayout w;
  size_t o = 0;
  w.frames = take(o, (size_t)B * sizeof(int32_t));
  w.status = take(o, (size_t)B * sizeof(int32_t));
  w.beam = beam_layout(o, max_frames, B, V, W, layers, H);
  w.total = o;
  return w;
}

// the per-frame kernels' view of a session: the beam is the state's
inline LmP stream_lmp(const BeamState& S, int B, int V, int blank, int W,
                      const asr_att_beam_lm_t* lm, double beta) {
  LmP p = {};
  static_cast<Beam&>(p) = S;
  p.B = B; p.V = V; p.blank = blank; p.W = W; p.poolT = S.max_frames;
  p.alpha = lm ? (float)lm->weight : 0.f;
  p.beta = (float)beta;
  p.has_lm = lm ? 1 : 0;
  if (lm) p.net = lm_net_from(lm);
  return p;
}

struct StreamWs { size_t lens, lse, topv, topc, total; };

// the class lists of the plain search ([B][Tc][W + 1]) and of the LM search
// ([B][W][W + 1]) share one region
inline StreamWs stream_ws(int Tc, int B, int V, int W) {
  StreamWs w;
  const size_t K = (size_t)W + 1;
  const size_t lists = (size_t)B * ((size_t)Tc > (size_t)W ? (size_t)Tc : (size_t)W) * K;
  w.lens = 0;
  w.lse = align16((size_t)B * sizeof(int32_t));
  w.topv = w.lse + align16((size_t)B * Tc * sizeof(float));
  w.topc = w.topv + align16(lists * sizeof(float));
  w.total = w.topc + align16(lists * sizeof(int32_t));
  return w;
}

inline bool stream_args_ok(int max_frames, int B, int V, int W) {
  return max_frames > 0 && max_frames <= (INT_MAX - 1) / kMaxBeam && beam_args_ok(1, B, V, W);
}

// The rows of `rows` (null: all) at the empty prefix; with an LM, lm_step(t =
// -1) then makes the root's LM state from the zero state and <eos>.  tok is the
// work list of that step: no token for the rows left alone.
__global__ void __launch_bounds__(64) beam_stream_reset_kernel(BeamState S, int W, int V,
                                                               const int32_t* __restrict__ rows) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r = (long long)b * W;
  const bool sel = !rows || rows[b] != 0;
  if (lane < W) {
    S.tok[r + lane] = sel && lane == 0 ? V - 1 : -1;
    S.src[r + lane] = -1;
  }
  if (sel && lane == 0) {
    S.frames[b] = 0; S.status[b] = 0;
    beam_root(S, b, W, S.max_frames);
  }
}

// Per row the frames this call consumes: lens[b] clipped to the chunk and to
// what max_frames leaves (status |= kStreamFull where that drops frames), 0 for
// a row whose counters are not ones a reset or a feed can have left (status |=
// kStreamInvalid: an uninitialised state must not index the pool).
__global__ void __launch_bounds__(256) beam_stream_prep_kernel(BeamState S, int B, int W, int Tc,
                                                               const int32_t* __restrict__ lens,
                                                               int32_t* __restrict__ eff_lens) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int frames = S.frames[b], n = S.n[b], nnodes = S.nnodes[b];
  int eff = max(0, min(lens[b], Tc));
  const bool ok = frames >= 0 && frames <= S.max_frames && n >= 1 && n <= W && nnodes >= 1 &&
                  (long long)nnodes <= (long long)frames * W + 1;
  if (!ok) {
    S.status[b] |= kStreamInvalid;
    eff = 0;
  } else if (eff > S.max_frames - frames) {
    eff = S.max_frames - frames;
    S.status[b] |= kStreamFull;
  }
  eff_lens[b] = eff;
  if (eff > 0) S.frames[b] = frames + eff;
}

__global__ void __launch_bounds__(64) beam_stream_kernel(
    const float* __restrict__ logits, long long st, long long sb, int T, int V,
    const int32_t* __restrict__ lens, int blank, int W, const float* __restrict__ lse_in,
    const float* __restrict__ topv, const int32_t* __restrict__ topc, BeamState S) {
  beam_search_body<true>(logits, st, sb, T, V, lens, blank, W, lse_in, topv, topc, S.pools,
                         &S, nullptr, nullptr, nullptr);
}

// One wave per row, entry i in lane i.  The best entry's labels and score: rank
// 0 and S_t, or for a row whose `final` flag is set lm_final_kernel's choice
// and value (the entries re-ranked with alpha lp_lm(<eos> | l) added; the state
// is only read).  stable_lens (nullable): the length of the longest common
// prefix of the n entries' label sequences -- every later hypothesis descends
// from a beam entry, so these labels are final.  The chains are first brought
// to the smallest depth, then walked up in lock step: a level at which all
// lanes hold one node ends the walk (the prefixes below are one prefix); a
// level at which the labels differ caps the length below it.  Labels are
// compared, not node ids: two ids can denote the same prefix.
__global__ void __launch_bounds__(64) beam_stream_out_kernel(
    BeamState S, int W, int V, int has_lm, float alpha, const int32_t* __restrict__ final,
    int32_t* __restrict__ hyps, int ld, int32_t* __restrict__ hyp_lens,
    float* __restrict__ scores, int32_t* __restrict__ stable_lens) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r = (long long)b * W;
  const int n = S.n[b];
  if ((S.status[b] & kStreamInvalid) || n < 1 || n > W) {
    if (lane == 0) {
      hyp_lens[b] = 0;
      scores[b] = neg_inf();
      if (stable_lens) stable_lens[b] = 0;
    }
    return;
  }
  const Node* pool = S.pools + (long long)b * ((long long)S.max_frames * W + 1);
  const bool fin = final && final[b] != 0;
  const bool act = lane < n;
  int node = 0, d = INT_MAX;
  float s = neg_inf();
  unsigned long long key = 0;
  if (act) {
    node = S.node[r + lane];
    d = S.depth[r + lane];
    s = logaddexp_(S.pb[r + lane], S.pnb[r + lane]);
    if (fin && has_lm) s += alpha * S.q[((long long)b * 2 * W + S.slot[r + lane]) * V + (V - 1)];
    key = make_key(s, lane);
  }
  const unsigned long long best = fin ? wave_max_u64(key) : 0ull;
  const bool win = act && (fin ? key == best : lane == 0);   // keys are distinct: one lane
  if (win) {
    int nd_ = node;
    int32_t* out = hyps + (long long)b * ld;
    for (int k = d - 1; k >= 0; --k) {       // d <= frames <= max_frames <= ld
      const Node nd = pool[nd_];
      out[k] = nd.label;
      nd_ = nd.parent;
    }
    hyp_lens[b] = d;
    scores[b] = s;
    if (stable_lens && fin) stable_lens[b] = d;
  }
  if (!stable_lens || fin) return;

  int dmin = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dmin = min(dmin, __shfl_xor(dmin, o, 64));
  if (act)
    for (int k = d; k > dmin; --k) node = pool[node].parent;
  int L = dmin;
  for (int lev = dmin; lev > 0; --lev) {
    const int node0 = __shfl(node, 0, 64);
    if (__ballot(act && node != node0) == 0ull) break;
    const Node nd = act ? pool[node] : Node{0, 0};
    const int lab0 = __shfl(nd.label, 0, 64);
    if (__ballot(act && nd.label != lab0) != 0ull) L = lev - 1;
    node = nd.parent;
  }
  if (lane == 0) stable_lens[b] = L;
}

// every entry of the beam in rank order: labels, length, S_t
__global__ void __launch_bounds__(64) beam_stream_nbest_kernel(
    BeamState S, int W, int32_t* __restrict__ hyps, int ld, int32_t* __restrict__ lens,
    float* __restrict__ scores, int32_t* __restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r = (long long)b * W;
  int n = S.n[b];
  if ((S.status[b] & kStreamInvalid) || n < 1 || n > W) n = 0;
  if (lane == 0) counts[b] = n;
  if (lane >= W) return;
  if (lane >= n) {
    lens[r + lane] = 0;
    scores[r + lane] = neg_inf();
    return;
  }
  const Node* pool = S.pools + (long long)b * ((long long)S.max_frames * W + 1);
  const int d = S.depth[r + lane];
  int node = S.node[r + lane];
  int32_t* out = hyps + (r + lane) * ld;
  for (int k = d - 1; k >= 0; --k) {         // d <= max_frames <= ld
    const Node nd = pool[node];
    out[k] = nd.label;
    node = nd.parent;
  }
  lens[r + lane] = d;
  scores[r + lane] = logaddexp_(S.pb[r + lane], S.pnb[r + lane]);
}

constexpr LmWho kStreamLmWho = {"ctc_beam_stream", "ctc_beam_stream", "LM dims", "CTC head",
                                " (blank included; <eos> takes the blank's place)"};

}  // namespace
}  // namespace asr

extern "C" size_t asr_ctc_beam_stream_state_bytes(int max_frames, int B, int V, int beam_width,
                                                  int lm_layers, int lm_H, int lm_Y) {
  if (!stream_args_ok(max_frames, B, V, beam_width)) return 0;
  if (lm_layers == 0) return stream_layout(max_frames, B, V, beam_width, 0, 0).total;
  if (lm_net_shape_check(lm_layers, lm_H, lm_Y, kStreamLmWho) != ASR_OK) return 0;
  return stream_layout(max_frames, B, V, beam_width, lm_layers, lm_H).total;
}

extern "C" size_t asr_ctc_beam_stream_ws_bytes(int Tc, int B, int V, int beam_width) {
  if (!beam_args_ok(Tc, B, V, beam_width)) return 0;
  return stream_ws(Tc, B, V, beam_width).total;
}

// What every session call asks of max_frames and of the state buffer of a
// session with (layers, H) of LM state per slot; on ASR_OK S is the state's view.
static int stream_state_check(const char* who, int max_frames, int B, int V, int beam_width,
                              int layers, int H, const void* state, size_t state_bytes,
                              BeamState* S) {
  ASR_REQUIRE(stream_args_ok(max_frames, B, V, beam_width), ASR_ERR_ARG,
              "%s: max_frames = %d outside [1, %d]", who, max_frames, (INT_MAX - 1) / kMaxBeam);
  const StreamLayout w = stream_layout(max_frames, B, V, beam_width, layers, H);
  ASR_REQUIRE(state_bytes >= w.total, ASR_ERR_WORKSPACE, "%s: state %zu < %zu bytes", who,
              state_bytes, w.total);
  ASR_REQUIRE(((uintptr_t)state & 15) == 0, ASR_ERR_ARG, "%s: state not 16-B aligned", who);
  char* base = (char*)state;
  S->frames = (int32_t*)(base + w.frames);
  S->status = (int32_t*)(base + w.status);
  S->max_frames = max_frames;
  beam_bind(*S, base, w.beam);
  return ASR_OK;
}

// What reset and feed ask of the session's shape, its LM and its state; on
// ASR_OK *lm is null where the LM term is absent and S is the state's view.
static int stream_check(const char* who, bool pointers, int max_frames, int B, int V, int blank,
                        int beam_width, const asr_att_beam_lm_t** lm, const void* state,
                        size_t state_bytes, BeamState* S) {
  int rc = beam_args_check(who, pointers && state, 1, B, V, blank, beam_width);
  if (rc != ASR_OK) return rc;
  if ((rc = lm_args_check(who, lm, V, kStreamLmWho)) != ASR_OK) return rc;
  return stream_state_check(who, max_frames, B, V, beam_width, *lm ? (*lm)->layers : 0,
                            *lm ? (*lm)->H : 0, state, state_bytes, S);
}

extern "C" int asr_ctc_beam_stream_reset(void* state, size_t state_bytes, int max_frames, int B,
                                         int V, int beam_width, const asr_att_beam_lm_t* lm,
                                         const int32_t* rows, void* stream) {
  BeamState S;
  const int rc = stream_check("ctc_beam_stream_reset", true, max_frames, B, V, 0, beam_width, &lm,
                              state, state_bytes, &S);
  if (rc != ASR_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_stream_reset_kernel, dim3(B), dim3(64), 0, s, S, beam_width, V, rows);
  ASR_LAUNCH_CHECK();
  return lm ? lm_launch_root(stream_lmp(S, B, V, 0, beam_width, lm, 0.0), lm, s) : ASR_OK;
}

extern "C" int asr_ctc_beam_stream_feed(const float* logits, long long stride_t, long long stride_b,
                                        int Tc, int B, int V, const int32_t* lens, int blank,
                                        int beam_width, int normalize, const asr_att_beam_lm_t* lm,
                                        double beta, const int32_t* final, void* state,
                                        size_t state_bytes, int max_frames, void* ws,
                                        size_t ws_bytes, int32_t* hyps, int ld_hyp,
                                        int32_t* hyp_lens, float* scores, int32_t* stable_lens,
                                        void* stream) {
  const char* who = "ctc_beam_stream_feed";
  int rc = beam_args_check(who, logits && lens && ws && hyps && hyp_lens && scores, Tc, B, V, blank,
                           beam_width);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(beta == beta && fabs(beta) <= 3.0e38, ASR_ERR_ARG, "%s: beta = %g is not finite", who,
              beta);
  BeamState S;
  if ((rc = stream_check(who, true, max_frames, B, V, blank, beam_width, &lm, state, state_bytes,
                         &S)) != ASR_OK)
    return rc;
  ASR_REQUIRE(ld_hyp >= max_frames, ASR_ERR_ARG, "%s: ld_hyp = %d < max_frames = %d", who, ld_hyp,
              max_frames);
  const int W = beam_width;
  const StreamWs w = stream_ws(Tc, B, V, W);
  if ((rc = beam_ws_check(who, ws, ws_bytes, w.total)) != ASR_OK) return rc;
  char* base = (char*)ws;
  int32_t* eff = (int32_t*)(base + w.lens);
  float* lse = (float*)(base + w.lse);
  float* topv = (float*)(base + w.topv);
  int32_t* topc = (int32_t*)(base + w.topc);

  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_stream_prep_kernel, dim3((B + 255) / 256), dim3(256), 0, s, S, B, W, Tc,
                     lens, eff);
  ASR_LAUNCH_CHECK();
  const bool plain = !lm && beta == 0.0;
  if (plain) {
    launch_rows(logits, stride_t, stride_b, Tc, B, V, eff, blank, W + 1, normalize, lse, topv, topc,
                s);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_stream_kernel, dim3(B), dim3(64), 0, s, logits, stride_t, stride_b, Tc,
                       V, eff, blank, W, lse, topv, topc, S);
    ASR_LAUNCH_CHECK();
  } else {
    LmP p = stream_lmp(S, B, V, blank, W, lm, beta);
    p.logits = logits; p.st = stride_t; p.sb = stride_b;
    p.T = Tc; p.lens = eff; p.lse = lse; p.topv = topv; p.topc = topc;
    launch_rows(logits, stride_t, stride_b, Tc, B, V, eff, blank, 0, normalize, lse, nullptr,
                nullptr, s);
    ASR_LAUNCH_CHECK();
    if ((rc = lm_launch_frames(p, Tc, lm, s)) != ASR_OK) return rc;
  }
  hipLaunchKernelGGL(beam_stream_out_kernel, dim3(B), dim3(64), 0, s, S, W, V, lm ? 1 : 0,
                     lm ? (float)lm->weight : 0.f, final, hyps, ld_hyp, hyp_lens, scores,
                     stable_lens);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_ctc_beam_stream_nbest(const void* state, size_t state_bytes, int max_frames,
                                         int B, int V, int beam_width, int lm_layers, int lm_H,
                                         int32_t* hyps, int ld_hyp, int32_t* lens, float* scores,
                                         int32_t* counts, void* stream) {
  const char* who = "ctc_beam_stream_nbest";
  int rc = beam_args_check(who, state && hyps && lens && scores && counts, 1, B, V, 0, beam_width);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(lm_layers >= 0 && lm_H >= 0, ASR_ERR_ARG, "%s: bad LM dims", who);
  ASR_REQUIRE(ld_hyp >= max_frames, ASR_ERR_ARG, "%s: ld_hyp = %d < max_frames = %d", who, ld_hyp,
              max_frames);
  BeamState S;
  if ((rc = stream_state_check(who, max_frames, B, V, beam_width, lm_layers, lm_H, state,
                               state_bytes, &S)) != ASR_OK)
    return rc;
  hipLaunchKernelGGL(beam_stream_nbest_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, S,
                     beam_width, hyps, ld_hyp, lens, scores, counts);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_ctc_beam_stream_status(const void* state, int B, int32_t* status, void* stream) {
  ASR_REQUIRE(state && status && B > 0, ASR_ERR_ARG, "ctc_beam_stream_status: bad argument");
  // (frames and status lead the state: their offsets depend on B alone)
  const char* at = (const char*)state + stream_layout(1, B, 2, 1, 0, 0).status;
  ASR_CHECK_HIP(hipMemcpyAsync(status, at, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
  return ASR_OK;
}
