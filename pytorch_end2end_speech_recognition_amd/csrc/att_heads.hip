// One attention step over all heads: AttentionMechanism.forward
// (attention_layer.py:141-251) for additive (location / content) and
// dot-product energies with H >= 1 heads.  The contract is include/asr_hip.h,
// "multi-head attention step".  f32 arithmetic whatever the compute mode.
//
// Forward: one launch, one work-group per (head, utterance).  The group forms
// W_dec_h dec[b] once, then walks the frames in chunks of AH_FCH: the conv
// features of a chunk go to LDS (one (frame, channel) item per thread), the
// energies of the chunk are formed a wave per frame with the lanes over the
// attention channels (coalesced enc_a rows, one wave reduction per frame).
// Mask, sharpening and softmax / sigmoid run over the T energies kept in LDS,
// and the context is a thread per encoder channel over the T weights.
//
// Backward: one launch, one work-group per utterance, which walks the heads
// in order h = 0 .. H-1.  d_dec[b] is the only output that sums over heads;
// each of its elements is owned by one thread, which adds head h's
// contribution after head h-1's: a fixed order, no atomics, run-to-run
// bitwise.  Everything else is per head.  The conv features f [T][C] of the
// head, and then dF over them, live in the workspace row of the utterance
// (written and read by this group only, between barriers).
//
// Plain data-parallel kernels: no spin-waits, no hand-offs between groups.
// Every frame loop is bounded by T and every channel loop by its extent.
#include <string.h>

#include "common.h"

namespace asr {
namespace {

constexpr int AH_FTHREADS = 256;   // forward: 4 waves
constexpr int AH_BTHREADS = 512;   // backward: 8 waves
constexpr int AH_FCH = 64;         // frames per forward chunk
constexpr int AH_CMAX = ASR_ATT_HEADS_MAX_C;
constexpr size_t AH_LDS_BUDGET = 64 * 1024;

struct AhP {
  int B, T, E, A, C, K, D, H, kind, sigmoid;
  float sharpen;
  const float* w_dec[ASR_ATT_HEADS_MAX];
  const float* w_conv[ASR_ATT_HEADS_MAX];
  const float* conv_w[ASR_ATT_HEADS_MAX];
  const float* v[ASR_ATT_HEADS_MAX];
};

// Sum / max over the work-group in a fixed order: wave totals, then the NW
// totals added by every thread in index order.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) s += red[i];
  __syncthreads();
  return s;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) s = fmaxf(s, red[i]);
  __syncthreads();
  return s;
}

// LDS floats of the two kernels (host and device agree through these).
__host__ __device__ inline size_t fwd_lds_floats(int T, int A, int C, int K, int D, int kind) {
  size_t n = (size_t)T + 16;                                  // energies / weights, reductions
  if (kind == ASR_ATT_HEADS_DOT) return n + D;
  n += 2 * (size_t)A + (size_t)A * C + (size_t)C * K;         // wd, v, W_conv, conv kernel
  if (C > 0) n += (size_t)T + 2 * (K / 2) + (size_t)AH_FCH * C;   // aw_prev with halo, chunk f
  return n;
}
__host__ __device__ inline size_t bwd_lds_floats(int T, int E, int A, int C, int K, int D,
                                                 int kind) {
  size_t n = (size_t)D + T + E + 16;                          // d_dec, de, d_ctx_h, reductions
  if (kind == ASR_ATT_HEADS_DOT) return n + D;
  n += 3 * (size_t)A + (size_t)A * C + (size_t)C * K;         // wd, v, dwd, W_conv, conv kernel
  if (C > 0) n += (size_t)T + 2 * (K / 2);
  return n;
}

__global__ __launch_bounds__(AH_FTHREADS) void att_heads_fwd(
    AhP p, const float* __restrict__ enc, const float* __restrict__ enc_a,
    const int32_t* __restrict__ lens, const float* __restrict__ dec,
    const float* __restrict__ aw_prev, float* __restrict__ ctx_out, float* __restrict__ aw_out) {
  extern __shared__ float sm[];
  constexpr int NW = AH_FTHREADS / 64;
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = p.T, A = p.A, C = p.C, K = p.K, D = p.D, E = p.E, pad = K / 2;
  float* e_s = sm;          // [T] energies, then weights
  float* red = e_s + T;     // [16]
  float* x = red + 16;
  const float* ea = enc_a + ((size_t)h * p.B + b) * T * A;
  const float* decb = dec + (size_t)b * D;
  int len = lens[b];
  len = len < 0 ? 0 : (len > T ? T : len);

  if (p.kind == ASR_ATT_HEADS_DOT) {   // A == D
    float* dec_s = x;
    for (int d = tid; d < D; d += AH_FTHREADS) dec_s[d] = decb[d];
    __syncthreads();
    for (int t = wv; t < T; t += NW) {
      float s = 0.f;
      for (int a = lane; a < D; a += 64) s += ea[(size_t)t * D + a] * dec_s[a];
      s = wave_sum(s);
      if (lane == 0) e_s[t] = s;
    }
  } else {
    float* wd = x; x += A;
    float* v_s = x; x += A;
    float* wc_s = x; x += (size_t)A * C;
    float* cw_s = x; x += (size_t)C * K;
    float* awp_s = x; x += C > 0 ? T + 2 * pad : 0;
    float* f_s = x;
    const float* wdec = p.w_dec[h];
    for (int a = tid; a < A; a += AH_FTHREADS) v_s[a] = p.v[h][a];
    for (int i = tid; i < A * C; i += AH_FTHREADS) wc_s[i] = p.w_conv[h][i];
    for (int i = tid; i < C * K; i += AH_FTHREADS) cw_s[i] = p.conv_w[h][i];
    if (C > 0) {
      const float* awp = aw_prev + ((size_t)b * p.H + h) * T;
      for (int j = tid; j < T + 2 * pad; j += AH_FTHREADS) {
        const int t = j - pad;
        awp_s[j] = (t >= 0 && t < T) ? awp[t] : 0.f;
      }
    }
    for (int a = wv; a < A; a += NW) {   // wd = W_dec_h dec[b]
      float s = 0.f;
      for (int d = lane; d < D; d += 64) s += wdec[(size_t)a * D + d] * decb[d];
      s = wave_sum(s);
      if (lane == 0) wd[a] = s;
    }
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += AH_FCH) {
      for (int i = tid; i < AH_FCH * C; i += AH_FTHREADS) {
        const int tt = i & (AH_FCH - 1), c = i / AH_FCH, t = t0 + tt;
        float s = 0.f;
        if (t < T)
          for (int k = 0; k < K; ++k) s += cw_s[c * K + k] * awp_s[t + k];
        f_s[tt * C + c] = s;
      }
      __syncthreads();
      for (int tt = wv; tt < AH_FCH && t0 + tt < T; tt += NW) {
        const int t = t0 + tt;
        float s = 0.f;
        for (int a = lane; a < A; a += 64) {
          float cv = 0.f;
          for (int c = 0; c < C; ++c) cv += wc_s[a * C + c] * f_s[tt * C + c];
          s += v_s[a] * tanhf_(ea[(size_t)t * A + a] + wd[a] + cv);
        }
        s = wave_sum(s);
        if (lane == 0) e_s[t] = s;
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // multiplicative mask (a padded frame keeps energy 0), sharpening, weights
  float* awo = aw_out + ((size_t)b * p.H + h) * T;
  if (p.sigmoid) {
    for (int t = tid; t < T; t += AH_FTHREADS) {
      const float ev = e_s[t] * (t < len ? 1.f : 0.f) * p.sharpen;
      const float w = 1.f / (1.f + expf(-ev));
      e_s[t] = w;
      awo[t] = w;
    }
  } else {
    float m = neg_inf();
    for (int t = tid; t < T; t += AH_FTHREADS) {
      const float ev = e_s[t] * (t < len ? 1.f : 0.f) * p.sharpen;
      e_s[t] = ev;
      m = fmaxf(m, ev);
    }
    m = block_max<NW>(m, red);
    float s = 0.f;
    for (int t = tid; t < T; t += AH_FTHREADS) {
      const float ex = expf(e_s[t] - m);
      e_s[t] = ex;
      s += ex;
    }
    s = block_sum<NW>(s, red);
    for (int t = tid; t < T; t += AH_FTHREADS) {
      const float w = e_s[t] / s;
      e_s[t] = w;
      awo[t] = w;
    }
  }
  __syncthreads();

  // ctx_h[b] = sum_t aw[t] enc[b, t, :]; four interleaved partial sums
  const float* encb = enc + (size_t)b * T * E;
  float* co = ctx_out + ((size_t)b * p.H + h) * E;
  for (int e = tid; e < E; e += AH_FTHREADS) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int t = 0;
    for (; t + 3 < T; t += 4) {
      s0 += e_s[t] * encb[(size_t)t * E + e];
      s1 += e_s[t + 1] * encb[(size_t)(t + 1) * E + e];
      s2 += e_s[t + 2] * encb[(size_t)(t + 2) * E + e];
      s3 += e_s[t + 3] * encb[(size_t)(t + 3) * E + e];
    }
    for (; t < T; ++t) s0 += e_s[t] * encb[(size_t)t * E + e];
    co[e] = (s0 + s1) + (s2 + s3);
  }
}

__global__ __launch_bounds__(AH_BTHREADS) void att_heads_bwd(
    AhP p, const float* __restrict__ enc, const float* __restrict__ enc_a,
    const int32_t* __restrict__ lens, const float* __restrict__ dec,
    const float* __restrict__ aw_prev, const float* __restrict__ aw_out,
    const float* __restrict__ d_ctx, const float* __restrict__ d_aw, float* d_enc_a,
    float* __restrict__ d_dec, float* __restrict__ d_aw_prev, float* __restrict__ dctx_tot,
    float* __restrict__ dwd, float* __restrict__ dv_part, float* __restrict__ dwc_part,
    float* __restrict__ dcw_part, float* fws) {
  extern __shared__ float sm[];
  constexpr int NW = AH_BTHREADS / 64, NT = AH_BTHREADS;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = p.T, A = p.A, C = p.C, K = p.K, D = p.D, E = p.E, H = p.H, pad = K / 2;
  const bool dot = p.kind == ASR_ATT_HEADS_DOT;
  float* ddec_s = sm;            // [D] element d owned by thread d % NT
  float* de_s = ddec_s + D;      // [T]
  float* dctx_s = de_s + T;      // [E]
  float* red = dctx_s + E;       // [16]
  float* x = red + 16;
  float* dec_s = x;              // dot: [D]
  float* wd = x; x += A;         // additive
  float* v_s = x; x += A;
  float* dwd_s = x; x += A;
  float* wc_s = x; x += (size_t)A * C;
  float* cw_s = x; x += (size_t)C * K;
  float* awp_s = x;
  const float* decb = dec + (size_t)b * D;
  const float* encb = enc + (size_t)b * T * E;
  float* fb = fws + (size_t)b * T * (C > 0 ? C : 1);   // f, then dF: [T][C]
  int len = lens[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  for (int d = tid; d < D; d += NT) ddec_s[d] = 0.f;
  if (dot) {
    for (int d = tid; d < D; d += NT) dec_s[d] = decb[d];
  }

  for (int h = 0; h < H; ++h) {
    const size_t bh = (size_t)b * H + h, hb = (size_t)h * p.B + b;
    const float* ea = enc_a + hb * T * A;
    float* dea = d_enc_a + hb * T * A;
    const float* awo = aw_out + bh * T;
    __syncthreads();   // the previous head's LDS reads are over
    for (int e = tid; e < E; e += NT) {
      const float g = d_ctx[bh * E + e];
      dctx_s[e] = g;
      dctx_tot[bh * E + e] = g;
    }
    if (!dot) {
      const float* wdec = p.w_dec[h];
      for (int a = tid; a < A; a += NT) v_s[a] = p.v[h][a];
      for (int i = tid; i < A * C; i += NT) wc_s[i] = p.w_conv[h][i];
      for (int i = tid; i < C * K; i += NT) cw_s[i] = p.conv_w[h][i];
      if (C > 0) {
        const float* awp = aw_prev + bh * T;
        for (int j = tid; j < T + 2 * pad; j += NT) {
          const int t = j - pad;
          awp_s[j] = (t >= 0 && t < T) ? awp[t] : 0.f;
        }
      }
      for (int a = wv; a < A; a += NW) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += wdec[(size_t)a * D + d] * decb[d];
        s = wave_sum(s);
        if (lane == 0) wd[a] = s;
      }
    }
    __syncthreads();
    // d aw[t] = d_aw[t] + d_ctx_h . enc[b, t, :]
    for (int t = wv; t < T; t += NW) {
      float s = 0.f;
      for (int e = lane; e < E; e += 64) s += dctx_s[e] * encb[(size_t)t * E + e];
      s = wave_sum(s);
      if (lane == 0) de_s[t] = s + (d_aw ? d_aw[bh * T + t] : 0.f);
    }
    __syncthreads();
    // through softmax / sigmoid, sharpening and the mask: de[t]
    if (p.sigmoid) {
      for (int t = tid; t < T; t += NT) {
        const float w = awo[t];
        de_s[t] = de_s[t] * w * (1.f - w) * p.sharpen * (t < len ? 1.f : 0.f);
      }
    } else {
      float s = 0.f;
      for (int t = tid; t < T; t += NT) s += awo[t] * de_s[t];
      s = block_sum<NW>(s, red);
      for (int t = tid; t < T; t += NT)
        de_s[t] = awo[t] * (de_s[t] - s) * p.sharpen * (t < len ? 1.f : 0.f);
    }
    __syncthreads();

    if (dot) {
      // d enc_a_h = de (x) dec;  d dec += sum_t de[t] enc_a_h[t, :]
      for (size_t i = tid; i < (size_t)T * D; i += NT) {
        const int t = (int)(i / D), d = (int)(i % D);
        dea[i] = de_s[t] * dec_s[d];
      }
      for (int d = tid; d < D; d += NT) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += de_s[t] * ea[(size_t)t * D + d];
        ddec_s[d] += s;
      }
      for (int t = tid; t < T; t += NT) d_aw_prev[bh * T + t] = 0.f;
      continue;
    }

    // conv features of this head: f[t][c]
    for (int i = tid; i < T * C; i += NT) {
      const int t = i % T, c = i / T;
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += cw_s[c * K + k] * awp_s[t + k];
      fb[(size_t)t * C + c] = s;
    }
    __syncthreads();
    // a thread per attention channel over the frames: g = d pre-activation
    for (int a = tid; a < A; a += NT) {
      float dv = 0.f, dw = 0.f, dwc[AH_CMAX];
#pragma unroll
      for (int c = 0; c < AH_CMAX; ++c) dwc[c] = 0.f;
      const float wda = wd[a], va = v_s[a];
      for (int t = 0; t < T; ++t) {
        float cv = 0.f;
        for (int c = 0; c < C; ++c) cv += wc_s[a * C + c] * fb[(size_t)t * C + c];
        const float pt = tanhf_(ea[(size_t)t * A + a] + wda + cv);
        const float g = de_s[t] * va * (1.f - pt * pt);
        dv += de_s[t] * pt;
        dw += g;
#pragma unroll
        for (int c = 0; c < AH_CMAX; ++c)
          if (c < C) dwc[c] += g * fb[(size_t)t * C + c];
        dea[(size_t)t * A + a] = g;
      }
      dv_part[hb * A + a] = dv;
      dwd[hb * A + a] = dw;
      dwd_s[a] = dw;
#pragma unroll
      for (int c = 0; c < AH_CMAX; ++c)
        if (c < C) dwc_part[(hb * A + a) * C + c] = dwc[c];
    }
    __syncthreads();   // f is read, g (in d_enc_a) and dwd_s are written
    // d dec += W_dec_h^T dwd_h
    {
      const float* wdec = p.w_dec[h];
      for (int d = tid; d < D; d += NT) {
        float s = 0.f;
        for (int a = 0; a < A; ++a) s += wdec[(size_t)a * D + d] * dwd_s[a];
        ddec_s[d] += s;
      }
    }
    if (C == 0) {
      for (int t = tid; t < T; t += NT) d_aw_prev[bh * T + t] = 0.f;
      continue;
    }
    // dF[t][c] = sum_a g[t][a] W_conv[a][c]: a wave per frame, over f's row
    for (int t = wv; t < T; t += NW) {
      float acc[AH_CMAX];
#pragma unroll
      for (int c = 0; c < AH_CMAX; ++c) acc[c] = 0.f;
      for (int a = lane; a < A; a += 64) {
        const float g = dea[(size_t)t * A + a];
#pragma unroll
        for (int c = 0; c < AH_CMAX; ++c)
          if (c < C) acc[c] += g * wc_s[a * C + c];
      }
#pragma unroll
      for (int c = 0; c < AH_CMAX; ++c) {
        if (c < C) {
          const float s = wave_sum(acc[c]);
          if (lane == 0) fb[(size_t)t * C + c] = s;
        }
      }
    }
    __syncthreads();
    // d conv kernel[c][k] = sum_t dF[t][c] aw_prev[t + k - pad]
    for (int i = tid; i < C * K; i += NT) {
      const int c = i / K, k = i % K;
      float s = 0.f;
      for (int t = 0; t < T; ++t) s += fb[(size_t)t * C + c] * awp_s[t + k];
      dcw_part[hb * C * K + i] = s;
    }
    // d aw_prev[j] = sum_c sum_k dF[j + pad - k][c] kernel[c][k]
    for (int j = tid; j < T; j += NT) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) {
        for (int k = 0; k < K; ++k) {
          const int t = j + pad - k;
          if (t >= 0 && t < T) s += fb[(size_t)t * C + c] * cw_s[c * K + k];
        }
      }
      d_aw_prev[bh * T + j] = s;
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += NT) d_dec[(size_t)b * D + d] = ddec_s[d];
}

// Shapes the kernels take; nullptr when they do, else why not.
const char* refusal(const asr_att_heads_t& q) {
  if (q.kind != ASR_ATT_HEADS_ADDITIVE && q.kind != ASR_ATT_HEADS_DOT) return "unknown kind";
  if (q.B < 1 || q.T < 1 || q.E < 1 || q.A < 1 || q.D < 1 || q.H < 1) return "empty dimension";
  if (q.H > ASR_ATT_HEADS_MAX) return "more than ASR_ATT_HEADS_MAX heads";
  if (q.B > 65535) return "more than 65535 utterances";
  const bool dot = q.kind == ASR_ATT_HEADS_DOT;
  if (dot && (q.A != q.D || q.C != 0)) return "dot: A must equal D and C be 0";
  if (q.C < 0 || q.C > ASR_ATT_HEADS_MAX_C) return "more than ASR_ATT_HEADS_MAX_C conv channels";
  if (q.C > 0 && (q.K < 1 || q.K % 2 == 0)) return "conv width must be odd";
  const unsigned long long lim = 1ull << 31;
  const unsigned long long bt = (unsigned long long)q.B * q.T;
  if (bt * q.E * 4 >= lim || bt * q.A * q.H * 4 >= lim || bt * q.H * 4 >= lim ||
      (unsigned long long)q.B * q.H * q.E * 4 >= lim ||
      (unsigned long long)q.B * q.H * q.A * (q.C > 0 ? q.C : 1) * 4 >= lim ||
      bt * (q.C > 0 ? q.C : 1) * 4 >= lim ||
      (unsigned long long)q.B * q.H * (q.C > 0 ? q.C : 1) * (q.K > 0 ? q.K : 1) * 4 >= lim)
    return "an operand of 2 GiB or more";
  const int K = q.C > 0 ? q.K : 1;
  const size_t f = fwd_lds_floats(q.T, q.A, q.C, K, q.D, q.kind) * 4;
  const size_t g = bwd_lds_floats(q.T, q.E, q.A, q.C, K, q.D, q.kind) * 4;
  if (f > AH_LDS_BUDGET || g > AH_LDS_BUDGET) return "LDS need over the 64 KiB budget";
  return nullptr;
}

AhP to_p(const asr_att_heads_t& q) {
  AhP p;
  memset(&p, 0, sizeof(p));
  p.B = q.B; p.T = q.T; p.E = q.E; p.A = q.A; p.C = q.C; p.K = q.C > 0 ? q.K : 1; p.D = q.D;
  p.H = q.H; p.kind = q.kind; p.sigmoid = q.sigmoid_smoothing != 0; p.sharpen = q.sharpening;
  for (int h = 0; h < q.H; ++h) {
    p.w_dec[h] = q.w_dec[h];
    p.w_conv[h] = q.w_conv[h];
    p.conv_w[h] = q.conv_w[h];
    p.v[h] = q.v[h];
  }
  return p;
}

int check_heads(const asr_att_heads_t* q, const char* who) {
  ASR_REQUIRE(q, ASR_ERR_ARG, "%s: params is null", who);
  const char* why = refusal(*q);
  ASR_REQUIRE(!why, ASR_ERR_UNSUPPORTED, "%s: %s", who, why);
  if (q->kind == ASR_ATT_HEADS_ADDITIVE) {
    for (int h = 0; h < q->H; ++h)
      ASR_REQUIRE(q->w_dec[h] && q->v[h] && (q->C == 0 || (q->w_conv[h] && q->conv_w[h])),
                  ASR_ERR_ARG, "%s: null weight pointer of head %d", who, h);
  }
  return ASR_OK;
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_att_heads_workspace_bytes(const asr_att_heads_t* q, int backward) {
  if (!q || refusal(*q)) return 0;
  if (!backward || q->kind == ASR_ATT_HEADS_DOT || q->C == 0) return 0;
  return (size_t)q->B * q->T * q->C * 4;
}

extern "C" int asr_att_heads_forward(const asr_att_heads_t* q, const float* enc,
                                     const float* enc_a, const int32_t* lens,
                                     const float* dec_out, const float* aw_prev, float* ctx_out,
                                     float* aw_out, void* workspace, size_t ws_bytes,
                                     void* stream) {
  int rc = check_heads(q, "att_heads_forward");
  if (rc) return rc;
  ASR_REQUIRE(enc && enc_a && lens && dec_out && ctx_out && aw_out && (q->C == 0 || aw_prev),
              ASR_ERR_ARG, "att_heads_forward: null pointer");
  (void)workspace;
  (void)ws_bytes;
  const AhP p = to_p(*q);
  const size_t lds = fwd_lds_floats(p.T, p.A, p.C, p.K, p.D, p.kind) * 4;
  hipLaunchKernelGGL(att_heads_fwd, dim3(p.H, p.B), dim3(AH_FTHREADS), lds, (hipStream_t)stream,
                     p, enc, enc_a, lens, dec_out, aw_prev, ctx_out, aw_out);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_att_heads_backward(const asr_att_heads_t* q, const float* enc,
                                      const float* enc_a, const int32_t* lens,
                                      const float* dec_out, const float* aw_prev,
                                      const float* aw_out, const float* d_ctx,
                                      const float* d_aw_out, float* d_enc_a, float* d_dec,
                                      float* d_aw_prev, float* dctx_tot, float* dwd,
                                      float* dv_part, float* dwc_part, float* dcw_part,
                                      void* workspace, size_t ws_bytes, void* stream) {
  int rc = check_heads(q, "att_heads_backward");
  if (rc) return rc;
  const bool add = q->kind == ASR_ATT_HEADS_ADDITIVE;
  ASR_REQUIRE(enc && enc_a && lens && dec_out && aw_out && d_ctx && d_enc_a && d_dec &&
                  d_aw_prev && dctx_tot && (q->C == 0 || aw_prev),
              ASR_ERR_ARG, "att_heads_backward: null pointer");
  ASR_REQUIRE(!add || (dwd && dv_part && (q->C == 0 || (dwc_part && dcw_part))), ASR_ERR_ARG,
              "att_heads_backward: null partial pointer");
  const size_t need = asr_att_heads_workspace_bytes(q, 1);
  ASR_REQUIRE(need == 0 || (workspace && ws_bytes >= need), ASR_ERR_WORKSPACE,
              "att_heads_backward: workspace too small");
  const AhP p = to_p(*q);
  const size_t lds = bwd_lds_floats(p.T, p.E, p.A, p.C, p.K, p.D, p.kind) * 4;
  hipLaunchKernelGGL(att_heads_bwd, dim3(p.B), dim3(AH_BTHREADS), lds, (hipStream_t)stream, p,
                     enc, enc_a, lens, dec_out, aw_prev, aw_out, d_ctx, d_aw_out, d_enc_a, d_dec,
                     d_aw_prev, dctx_tot, dwd, dv_part, dwc_part, dcw_part, (float*)workspace);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
