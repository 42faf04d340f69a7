// CTC forced alignment on gfx950: the Viterbi (max-plus) path of a known label
// sequence through the blank-interleaved lattice, the class of every frame and
// the first / last frame of every label (include/asr_hip.h, asr_ctc_align).
//
// The path is chosen on the RAW logits: subtracting a frame's log-sum-exp from
// every state of that frame cannot change an argmax, so the recurrence is
// float32 adds and compares only and a float32 host restatement is bit-exact,
// ties included (first predecessor in the order s, s-1, s-2).
//
// Kernels (all stream-ordered, no host sync):
//   ctc_align_prep    1 thread: exclusive scan of label_lens -> label offsets.
//   ctc_align_gather  one wave per (b,t) row: g[b][t][s] = x[b,t,class(s)] for
//                     the row's S states (-inf up to Spad = 64 K), stored
//                     lattice-contiguous as ctc_emit stores its rows; with
//                     `normalize` also the row's log-sum-exp (one read of the
//                     row, the accumulator of ctc_emit).
//   ctc_viterbi<K>    one work-group of two waves per utterance.  Wave 0 runs
//                     the lattice (lane l owns states l K .. l K + K - 1 in
//                     registers, neighbours through DPP wave shifts, no global
//                     load inside its loop); wave 1 streams the gathered rows
//                     into a two-chunk LDS ring, as in ctc_lattice.  Per frame
//                     each lane packs its K two-bit backpointers into one u32
//                     (256 B per frame).  Then wave 0 walks the path back and
//                     writes ali / starts / ends / scores (below).
#include "common.h"
#include "ctc_lattice.h"

namespace asr {
namespace {

// Backpointer words of frames t < kAliLds never leave LDS; later frames' words
// go to the workspace and come back kAliChunk frames at a time.  kAliLds is a
// multiple of kAliChunk, so a chunk is entirely on one side.
constexpr int kAliChunk = 64;
constexpr int kAliLds = 256;
static_assert(kAliLds % kAliChunk == 0, "a chunk is LDS-resident or staged as a whole");

struct AliWs {
  float* g;        // [B*T*Spad]
  float* lse;      // [B*T]
  uint32_t* bp;    // [B*max(T - kAliLds, 0)*64]
  int32_t* offs;   // [B]
};

inline size_t ali_layout(int T, int B, int max_label_len, AliWs* ws, char* base) {
  const int Spad = 64 * pick_k(max_label_len);
  const int Tg = T > kAliLds ? T - kAliLds : 0;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align256(off + bytes); return base + o; };
  char* p;
  p = take(sizeof(float) * (size_t)B * T * Spad);        if (ws) ws->g = (float*)p;
  p = take(sizeof(float) * (size_t)B * T);               if (ws) ws->lse = (float*)p;
  p = take(sizeof(uint32_t) * (size_t)B * Tg * 64);      if (ws) ws->bp = (uint32_t*)p;
  p = take(sizeof(int32_t) * (size_t)B);                 if (ws) ws->offs = (int32_t*)p;
  return off;
}

__global__ void ctc_align_prep(const int32_t* __restrict__ label_lens, int B,
                               int32_t* __restrict__ offs) {
  // single thread scan, as ctc_prep's (the labels are range-checked per row
  // by the row's own work-group in ctc_viterbi)
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int acc = 0;
    for (int b = 0; b < B; ++b) {
      offs[b] = acc;
      const int L = label_lens[b];
      acc += L < 0 ? 0 : L;
    }
  }
}

// A row whose label_len is outside [0, max_label_len] is infeasible and its
// labels are never read.
__device__ __forceinline__ int row_labels(int Lraw, int max_label_len) {
  return (Lraw < 0 || Lraw > max_label_len) ? -1 : Lraw;
}

__global__ void __launch_bounds__(256) ctc_align_gather(
    const float* __restrict__ acts, long long st, long long sb, int T, int B, int V,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ label_lens,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ offs, int blank,
    int max_label_len, int Spad, int normalize, float* __restrict__ lse_out,
    float* __restrict__ g) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= (long long)B * T) return;
  const int b = (int)(row / T), t = (int)(row % T);
  if (t >= act_lens[b]) return;
  const float* x = acts + (long long)t * st + (long long)b * sb;
  if (normalize) {
    float m = neg_inf(), s = 0.f;
    const int h = min(head_elems(x), V);
    if (lane < h) lse_acc1(m, s, x[lane]);
    const int n4 = (V - h) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + h);
    int i = lane;
    for (; i + 192 < n4; i += 256) {
      const float4 v0 = x4[i], v1 = x4[i + 64], v2 = x4[i + 128], v3 = x4[i + 192];
      lse_acc4(m, s, v0); lse_acc4(m, s, v1); lse_acc4(m, s, v2); lse_acc4(m, s, v3);
    }
    for (; i < n4; i += 64) lse_acc4(m, s, x4[i]);
    for (int v = h + 4 * n4 + lane; v < V; v += 64) lse_acc1(m, s, x[v]);
    const float M = wave_max(m);
    const float tot = wave_sum(m == neg_inf() ? 0.f : s * __expf(m - M));
    if (lane == 0) lse_out[row] = M + __logf(tot);
  }
  const int L = max(row_labels(label_lens[b], max_label_len), 0);
  const int S = 2 * L + 1;
  const int32_t* lab = labels + offs[b];
  float* e = g + row * Spad;
  for (int st_ = lane; st_ < Spad; st_ += 64) {
    float v = neg_inf();
    if (st_ < S) {
      int c = (st_ & 1) ? lab[st_ >> 1] : blank;
      c = c < 0 ? 0 : (c >= V ? V - 1 : c);   // a bad label: the row is infeasible anyway
      v = x[c];                                // raw: no normaliser on the argmax path
    }
    e[st_] = v;
  }
}

// Orders one wave's LDS traffic (the backtrace runs in wave 0 alone: lanes
// exchange data through LDS with no other wave to wait for).
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

struct AliOut {
  int32_t* ali;     // [B][T]
  int32_t* starts;  // [B][max_label_len] or null
  int32_t* ends;
  float* scores;    // [B]
};

// The outputs of a row without a path (infeasible, or no frames).
__device__ __forceinline__ void write_no_path(const AliOut& o, int b, int T, int max_label_len,
                                              float score, int tid, int nthreads) {
  for (int t = tid; t < T; t += nthreads) o.ali[(size_t)b * T + t] = -1;
  for (int j = tid; j < max_label_len; j += nthreads) {
    if (o.starts) o.starts[(size_t)b * max_label_len + j] = -1;
    if (o.ends) o.ends[(size_t)b * max_label_len + j] = -1;
  }
  if (tid == 0) o.scores[b] = score;
}

template <int K>
__global__ void __launch_bounds__(128) ctc_viterbi(
    int T, int V, int max_label_len, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ label_lens, const int32_t* __restrict__ act_lens,
    const int32_t* __restrict__ offs, int blank, int normalize, const float* __restrict__ g,
    const float* __restrict__ lse, uint32_t* __restrict__ bpg, AliOut out) {
  constexpr int Spad = 64 * K;
  constexpr int C = K <= 4 ? 16 : (K == 8 ? 8 : 4);  // rows per chunk (LDS ring 2*C*Spad*4 B)
  constexpr int LOGK = K == 1 ? 0 : K == 2 ? 1 : K == 4 ? 2 : K == 8 ? 3 : 4;
  __shared__ __attribute__((aligned(16))) float ring[2][C][Spad];   // 32 KB
  // rows [0, kAliLds): the resident frames' words; the kAliChunk rows after
  // them: the staging area of a chunk that comes back from the workspace
  __shared__ uint32_t bpl[kAliLds + kAliChunk][64];                 // 80 KB
  __shared__ int32_t cls[Spad / 2];       // class of label j
  __shared__ int32_t sp_start[Spad / 2], sp_end[Spad / 2];
  __shared__ int32_t path[kAliChunk];     // state of each frame of the chunk being walked
  __shared__ int s_bad;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Tb = max(min(act_lens[b], T), 0);
  const int Lrow = row_labels(label_lens[b], max_label_len);
  const int L = max(Lrow, 0);
  const int S = 2 * L + 1;
  const int32_t* lab = labels + offs[b];
  const float NEG = neg_inf();

  if (tid == 0) s_bad = Lrow < 0;
  for (int j = tid; j < Spad / 2; j += 128) { sp_start[j] = -1; sp_end[j] = -1; }
  __syncthreads();
  for (int j = tid; j < L; j += 128) {
    const int c = lab[j];
    cls[j] = c;
    if (c < 0 || c >= V || c == blank) s_bad = 1;
  }
  __syncthreads();
  if (s_bad || Tb == 0) {
    write_no_path(out, b, T, max_label_len, (!s_bad && L == 0) ? 0.f : NEG, tid, 128);
    return;
  }
  const int N = Tb - 1;               // lattice steps after the initial row
  const int nch = (N + C - 1) / C;
  // row of the n-th step (clamped: the loader's overrun rows are harmless)
  auto row_of = [&](int n) { return 1 + min(n, N - 1); };
  const float* E = g + (size_t)b * T * Spad + lane * K;

  if (wave == 1) {
    // ---------------- loader (ctc_lattice's) ----------------
    float r[C][K];
    if (nch > 0) {
#pragma unroll
      for (int j = 0; j < C; ++j) load_k<K>(r[j], E + (size_t)row_of(j) * Spad);
#pragma unroll
      for (int j = 0; j < C; ++j) store_k<K>(&ring[0][j][lane * K], r[j]);
      if (nch > 1) {
#pragma unroll
        for (int j = 0; j < C; ++j) load_k<K>(r[j], E + (size_t)row_of(C + j) * Spad);
      }
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      if (c + 1 < nch) {
#pragma unroll
        for (int j = 0; j < C; ++j) store_k<K>(&ring[(c + 1) & 1][j][lane * K], r[j]);
        if (c + 2 < nch) {
#pragma unroll
          for (int j = 0; j < C; ++j)
            load_k<K>(r[j], E + (size_t)row_of((c + 2) * C + j) * Spad);
        }
      }
      lds_barrier();
    }
    return;
  }

  // ---------------- max-plus lattice ----------------
  bool valid[K], skip[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = lane * K + k;
    valid[k] = s < S;
    // transition s-2 -> s allowed (s odd label state, label differs)
    skip[k] = (s & 1) && s >= 3 && s < S && cls[s >> 1] != cls[(s >> 1) - 1];
  }
  const int Tg = T > kAliLds ? T - kAliLds : 0;
  uint32_t* BP = bpg + (size_t)b * Tg * 64 + lane;
  float a[K];
  {
    float e0[K];
    load_k<K>(e0, E);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int s = lane * K + k;
      a[k] = (s < 2 && valid[k]) ? e0[k] : NEG;
    }
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    float ec[C][K];
#pragma unroll
    for (int j = 0; j < C; ++j) load_k<K>(ec[j], &ring[c & 1][j][lane * K]);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const int n = c * C + j;
      if (n < N) {
        const float (&e)[K] = ec[j];
        float p1 = from_lower_lane(a[K - 1]);
        float p2 = (K >= 2) ? from_lower_lane(a[K >= 2 ? K - 2 : 0]) : from_lower_lane(p1);
        if (lane == 0) { p1 = NEG; p2 = NEG; }
        if (K == 1 && lane == 1) p2 = NEG;
        float nx[K];
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float a1 = (k >= 1) ? a[k >= 1 ? k - 1 : 0] : p1;
          const float a2 = (k >= 2) ? a[k >= 2 ? k - 2 : 0] : ((k == 1) ? p1 : p2);
          // first predecessor in the order s, s-1, s-2 that attains the max
          float m = a[k];
          uint32_t bp = 0;
          if (a1 > m) { m = a1; bp = 1; }
          // K even: state parity = k parity, and blank (even) states never skip
          if (!((K % 2 == 0) && (k % 2 == 0)) && skip[k] && a2 > m) { m = a2; bp = 2; }
          nx[k] = valid[k] ? m + e[k] : NEG;
          w |= bp << (2 * k);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = nx[k];
        const int t = 1 + n;
        if (t < kAliLds) bpl[t][lane] = w;
        else BP[(size_t)(t - kAliLds) * 64] = w;
      }
    }
    lds_barrier();
  }

  // ---------------- end state ----------------
  float v1 = NEG, v2 = NEG;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = lane * K + k;
    if (s == S - 1) v1 = a[k];
    if (s == S - 2) v2 = a[k];
  }
  v1 = wave_max(v1);   // one lane holds the value, the others the identity
  v2 = wave_max(v2);
  const bool last = L == 0 || v1 >= v2;
  const float endv = last ? v1 : v2;
  if (!(endv > NEG)) {
    write_no_path(out, b, T, max_label_len, NEG, lane, 64);
    return;
  }

  // ---------------- backtrace (this wave alone) ----------------
  // The words of frames >= kAliLds were stored by this wave: once its own
  // stores have completed it may load them back.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int s = last ? S - 1 : S - 2;
  if (lane == 0 && (s & 1)) sp_end[s >> 1] = Tb - 1;
  float score = 0.f;
  for (int c = (Tb - 1) / kAliChunk; c >= 0; --c) {
    const int lo = c * kAliChunk, hi = min(Tb, lo + kAliChunk) - 1;
    int r0 = lo;   // bpl row of frame lo
    if (lo >= kAliLds) {
      // whole-wave 256-B row loads, sixteen in flight
      const uint32_t* src = BP + (size_t)(lo - kAliLds) * 64;
      for (int j0 = 0; j0 <= hi - lo; j0 += 16) {
        uint32_t r[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = j0 + q <= hi - lo ? src[(size_t)(j0 + q) * 64] : 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) bpl[kAliLds + j0 + q][lane] = r[q];
      }
      r0 = kAliLds;
    }
    wave_lds_sync();
    for (int t = hi; t >= lo; --t) {
      if (lane == 0) path[t - lo] = s;
      if (t > 0) {
        const uint32_t w = bpl[r0 + t - lo][s >> LOGK];
        const int ns = s - (int)((w >> (2 * (s & (K - 1)))) & 3u);
        if (ns != s && lane == 0) {
          if (s & 1) sp_start[s >> 1] = t;
          if (ns & 1) sp_end[ns >> 1] = t - 1;
        }
        s = ns;
      }
    }
    wave_lds_sync();
    // the chunk's frames in parallel: class, and the path's log-probability term
    const int t = lo + lane;
    float term = 0.f;
    if (t <= hi) {
      const int sv = path[lane];
      out.ali[(size_t)b * T + t] = (sv & 1) ? cls[sv >> 1] : blank;
      if (normalize)
        term = g[((size_t)b * T + t) * Spad + sv] - lse[(size_t)b * T + t];
    }
    // fixed order: the DPP tree over the chunk's 64 frames, chunks from the
    // last to the first
    if (normalize) score += wave_sum(term);
    wave_lds_sync();
  }
  if (lane == 0 && (s & 1)) sp_start[s >> 1] = 0;
  wave_lds_sync();
  for (int t = Tb + lane; t < T; t += 64) out.ali[(size_t)b * T + t] = -1;
  for (int j = lane; j < max_label_len; j += 64) {
    if (out.starts) out.starts[(size_t)b * max_label_len + j] = j < L ? sp_start[j] : -1;
    if (out.ends) out.ends[(size_t)b * max_label_len + j] = j < L ? sp_end[j] : -1;
  }
  if (lane == 0) out.scores[b] = normalize ? score : endv;
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_ctc_align_limits(int* chunk_frames, int* lds_frames) {
  ASR_REQUIRE(chunk_frames && lds_frames, ASR_ERR_ARG, "ctc_align_limits: null pointer");
  *chunk_frames = kAliChunk;
  *lds_frames = kAliLds;
  return ASR_OK;
}

extern "C" size_t asr_ctc_align_ws_bytes(int T, int B, int V, int max_label_len) {
  (void)V;
  if (T <= 0 || B <= 0 || max_label_len < 0 || 2 * max_label_len + 1 > 64 * kMaxK) return 0;
  return ali_layout(T, B, max_label_len, nullptr, nullptr);
}

extern "C" int asr_ctc_align(const float* logits, long long stride_t, long long stride_b, int T,
                             int B, int V, const int32_t* labels_flat, const int32_t* label_lens,
                             const int32_t* act_lens, int max_label_len, int blank, int normalize,
                             int32_t* ali, int32_t* starts, int32_t* ends, float* scores,
                             void* workspace, size_t ws_bytes, void* stream) {
  ASR_REQUIRE(logits && label_lens && act_lens && ali && scores && workspace, ASR_ERR_ARG,
              "ctc_align: null pointer argument");
  ASR_REQUIRE(T > 0 && B > 0 && V > 1 && stride_t > 0 && stride_b > 0, ASR_ERR_ARG,
              "ctc_align: bad shape T=%d B=%d V=%d strides %lld / %lld", T, B, V, stride_t,
              stride_b);
  ASR_REQUIRE(blank >= 0 && blank < V, ASR_ERR_ARG, "ctc_align: blank %d out of range", blank);
  ASR_REQUIRE(max_label_len >= 0, ASR_ERR_ARG, "ctc_align: max_label_len %d", max_label_len);
  ASR_REQUIRE(labels_flat || max_label_len == 0, ASR_ERR_ARG, "ctc_align: labels is null");
  ASR_REQUIRE(2 * max_label_len + 1 <= 64 * kMaxK, ASR_ERR_UNSUPPORTED,
              "ctc_align: max_label_len %d exceeds %d", max_label_len, (64 * kMaxK - 1) / 2);
  const long long two_gib = 1ll << 31;
  const long long extent = (long long)(T - 1) * stride_t + (long long)(B - 1) * stride_b + V;
  ASR_REQUIRE(extent * 4 < two_gib && (long long)B * T * 4 < two_gib &&
                  (long long)B * max_label_len * 4 < two_gib,
              ASR_ERR_UNSUPPORTED, "ctc_align: an operand of 2 GiB or more");
  const size_t need = asr_ctc_align_ws_bytes(T, B, V, max_label_len);
  ASR_REQUIRE(ws_bytes >= need, ASR_ERR_WORKSPACE, "ctc_align: workspace %zu < %zu", ws_bytes,
              need);
  ASR_REQUIRE(((uintptr_t)workspace & 15) == 0, ASR_ERR_ARG,
              "ctc_align: workspace not 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  AliWs ws;
  ali_layout(T, B, max_label_len, &ws, (char*)workspace);
  const int K = pick_k(max_label_len);
  const int Spad = 64 * K;
  hipLaunchKernelGGL(ctc_align_prep, dim3(1), dim3(64), 0, s, label_lens, B, ws.offs);
  ASR_LAUNCH_CHECK();
  const long long rows = (long long)B * T;
  hipLaunchKernelGGL(ctc_align_gather, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits,
                     stride_t, stride_b, T, B, V, labels_flat, label_lens, act_lens, ws.offs, blank,
                     max_label_len, Spad, normalize, ws.lse, ws.g);
  ASR_LAUNCH_CHECK();
  const AliOut out = {ali, starts, ends, scores};
  auto viterbi = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B), dim3(128), 0, s, T, V, max_label_len, labels_flat,
                       label_lens, act_lens, ws.offs, blank, normalize, ws.g, ws.lse, ws.bp, out);
  };
  switch (K) {
    case 1: viterbi(ctc_viterbi<1>); break;
    case 2: viterbi(ctc_viterbi<2>); break;
    case 4: viterbi(ctc_viterbi<4>); break;
    case 8: viterbi(ctc_viterbi<8>); break;
    case 16: viterbi(ctc_viterbi<16>); break;
    default: set_error("ctc_align: unsupported K=%d", K); return ASR_ERR_UNSUPPORTED;
  }
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
