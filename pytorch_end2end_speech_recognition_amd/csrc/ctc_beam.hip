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
#include <limits.h>

#include "common.h"

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

template <int WAVES>
__device__ __forceinline__ float group_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
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

__global__ void __launch_bounds__(64) beam_search_kernel(
    const float* __restrict__ logits, long long st, long long sb, int T, int V,
    const int32_t* __restrict__ lens, int blank, int W, const float* __restrict__ lse_in,
    const float* __restrict__ topv, const int32_t* __restrict__ topc, Node* __restrict__ pools,
    int32_t* __restrict__ hyps, int32_t* __restrict__ hyp_lens, float* __restrict__ scores) {
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
  Node* pool = pools + (long long)b * ((long long)T * W + 1);

  if (lane == 0) {
    pool[0].parent = 0;
    pool[0].label = -1;
    s_node[0] = 0; s_par[0] = 0; s_last[0] = -1; s_depth[0] = 0;
    s_pb[0] = 0.f; s_pnb[0] = neg_inf();
    s_hash[0] = 0; s_phash[0] = 0;
  }
  int n = 1, nnodes = 1;
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

  if (lane == 0) {
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

static int beam_launch(const float* logits, long long stride_t, long long stride_b, int T, int B,
                       int V, const int32_t* lens, int blank, int beam_width, int normalize,
                       void* ws, size_t ws_bytes, int32_t* hyps, int32_t* hyp_lens, float* scores,
                       bool search, void* stream) {
  ASR_REQUIRE(logits && lens && ws && (!search || (hyps && hyp_lens && scores)), ASR_ERR_ARG,
              "ctc_beam_search: null pointer");
  ASR_REQUIRE(T > 0 && B > 0, ASR_ERR_ARG, "ctc_beam_search: bad shape");
  ASR_REQUIRE(V >= 2, ASR_ERR_ARG, "ctc_beam_search: V = %d < 2", V);
  ASR_REQUIRE(beam_width >= 1 && beam_width <= kMaxBeam, ASR_ERR_ARG,
              "ctc_beam_search: beam_width = %d outside [1, %d]", beam_width, kMaxBeam);
  ASR_REQUIRE(blank >= 0 && blank < V, ASR_ERR_ARG, "ctc_beam_search: blank = %d outside [0, %d)",
              blank, V);
  const BeamWs w = beam_ws(T, B, V, beam_width);
  ASR_REQUIRE(ws_bytes >= w.total, ASR_ERR_WORKSPACE, "ctc_beam_search: workspace %zu < %zu bytes",
              ws_bytes, w.total);
  ASR_REQUIRE(((uintptr_t)ws & 15) == 0, ASR_ERR_ARG, "ctc_beam_search: workspace not 16-B aligned");
  char* base = (char*)ws;
  float* lse = (float*)(base + w.lse);
  float* topv = (float*)(base + w.topv);
  int32_t* topc = (int32_t*)(base + w.topc);
  Node* pool = (Node*)(base + w.pool);
  const long long frames = (long long)B * T;
  const int K = beam_width + 1;
  hipStream_t s = (hipStream_t)stream;
  if (V <= kWaveModeMaxV) {
    hipLaunchKernelGGL(beam_rows_kernel<1>, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s,
                       logits, stride_t, stride_b, T, B, V, lens, blank, K, normalize, lse, topv,
                       topc);
  } else {
    hipLaunchKernelGGL(beam_rows_kernel<4>, dim3((unsigned)frames), dim3(256), 0, s, logits,
                       stride_t, stride_b, T, B, V, lens, blank, K, normalize, lse, topv, topc);
  }
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
