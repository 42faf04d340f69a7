// Activation -> max-pool -> BatchNorm2d -> dropout block of a CNNEncoder layer
// (encoders/cnn.py:78-111) for the activations the ReLU block of cnn.hip does
// not take: PReLU (one learnable slope) and hard-tanh(0, 20); ReLU is accepted
// too.  The pool keeps the true maximum of the activated values in its window
// (PReLU outputs can be negative, so a partial ceil-mode window or a window of
// negative values must not be floored at 0 as the ReLU block may do).
//
// Layouts as in cnn.hip: z / dz [B][T+2][F+2][C] (zero halo, interior used),
// P [B][To][Fo][C] f32 (pooled activations), slot uint8 (argmax within the
// window, df * pt + dt, first maximum in torch's scan order), out either the
// next layer's haloed operand (f32 / bf16) or flat [B][To][Fo][C] f32.
// Every per-channel sum (BN moments, BN backward sums, conv bias gradient,
// PReLU slope gradient) is taken per 128-pixel chunk by one thread per channel
// and the chunks are then added in order: bitwise reproducible.
#include "common.h"

namespace asr {
namespace {

constexpr int ACT_CHUNK = 128;

struct ActDims {
  int B, T, F, C, pt, pf, To, Fo;
};

__device__ __forceinline__ float act_fwd(float z, int act, float slope) {
  if (act == ASR_ACT_PRELU) return z > 0.f ? z : slope * z;
  if (act == ASR_ACT_HARDTANH) return fminf(fmaxf(z, 0.f), 20.f);
  return fmaxf(z, 0.f);
}

__device__ __forceinline__ long long pad_px(int b, int t, int f, int T, int F) {
  return ((long long)b * (T + 2) + t + 1) * (F + 2) + f + 1;
}

// P[q][c] = max over the window of act(z); slot = first argmax
__global__ void __launch_bounds__(256) act_pool(const float* __restrict__ z, ActDims d, int act,
                                                const float* __restrict__ slope_p,
                                                float* __restrict__ P, uint8_t* __restrict__ slot) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)d.B * d.To * d.Fo * d.C;
  if (i >= n) return;
  const float slope = act == ASR_ACT_PRELU ? *slope_p : 0.f;
  const int c = (int)(i % d.C);
  long long q = i / d.C;
  const int fo = (int)(q % d.Fo);
  q /= d.Fo;
  const int to = (int)(q % d.To), b = (int)(q / d.To);
  if (!d.pt) {
    P[i] = act_fwd(z[pad_px(b, to, fo, d.T, d.F) * d.C + c], act, slope);
    return;
  }
  float best = -__builtin_huge_valf();
  int bs = 0;
  for (int df = 0; df < d.pf; ++df) {
    const int f = fo * d.pf + df;
    if (f >= d.F) break;
    for (int dt = 0; dt < d.pt; ++dt) {
      const int t = to * d.pt + dt;
      if (t >= d.T) break;
      const float v = act_fwd(z[pad_px(b, t, f, d.T, d.F) * d.C + c], act, slope);
      if (v > best || (df == 0 && dt == 0)) { best = v; bs = df * d.pt + dt; }
    }
  }
  P[i] = best;
  slot[i] = (uint8_t)bs;
}

// part[chunk][c] = sum over the chunk's pixels of (P - sub[c])^pw (sub nullable)
__global__ void __launch_bounds__(256) act_moment(const float* __restrict__ P, long long npx, int C,
                                                  const float* __restrict__ sub, int square,
                                                  float* __restrict__ part) {
  const long long p0 = (long long)blockIdx.x * ACT_CHUNK;
  const int np = (int)min((long long)ACT_CHUNK, npx - p0);
  for (int c = threadIdx.x; c < C; c += 256) {
    const float m = sub ? sub[c] : 0.f;
    float s = 0.f;
    for (int p = 0; p < np; ++p) {
      const float v = P[(p0 + p) * C + c] - m;
      s += square ? v * v : v;
    }
    part[(long long)blockIdx.x * C + c] = s;
  }
}

// mode 0: mean[c] = sum / n.  mode 1: var = sum / n -> rstd, running stats.
__global__ void __launch_bounds__(256) act_moment_finish(const float* __restrict__ part, int nchunk,
                                                         int C, long long npx, int mode,
                                                         float* __restrict__ mean,
                                                         float* __restrict__ rstd, float eps,
                                                         float momentum, float* __restrict__ run_mean,
                                                         float* __restrict__ run_var) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int k = 0; k < nchunk; ++k) s += part[(long long)k * C + c];
  if (mode == 0) {
    mean[c] = s / (float)npx;
    return;
  }
  const float var = s / (float)npx;
  rstd[c] = 1.f / sqrtf(var + eps);
  if (run_mean) {
    const float unb = npx > 1 ? s / (float)(npx - 1) : var;
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean[c];
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

__global__ void __launch_bounds__(256) act_eval_stats(const float* __restrict__ run_mean,
                                                      const float* __restrict__ run_var, float eps,
                                                      int C, float* __restrict__ mean,
                                                      float* __restrict__ rstd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  mean[c] = run_mean[c];
  rstd[c] = 1.f / sqrtf(run_var[c] + eps);
}

// out = dropout(BN(P))
__global__ void __launch_bounds__(256) act_apply(const float* __restrict__ P, ActDims d,
                                                 const float* __restrict__ mean,
                                                 const float* __restrict__ rstd,
                                                 const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float drop,
                                                 unsigned long long seed, void* __restrict__ out,
                                                 int out_bf16, int flat) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)d.B * d.To * d.Fo * d.C;
  if (i >= n) return;
  const int c = (int)(i % d.C);
  float v = P[i];
  if (mean) v = (v - mean[c]) * rstd[c] * gamma[c] + beta[c];
  if (drop > 0.f) v *= drop_scale(drop, seed, (unsigned long long)i);
  long long o = i;
  if (!flat) {
    long long q = i / d.C;
    const int fo = (int)(q % d.Fo);
    q /= d.Fo;
    const int to = (int)(q % d.To), b = (int)(q / d.To);
    o = pad_px(b, to, fo, d.To, d.Fo) * d.C + c;
  }
  if (out_bf16)
    static_cast<uint16_t*>(out)[o] = f2bf(v);
  else
    static_cast<float*>(out)[o] = v;
}

// dy(q, c): the incoming gradient at pooled pixel q with the dropout mask applied
__device__ __forceinline__ float dy_at(const float* __restrict__ dnext, int flat, const ActDims& d,
                                       long long q, int c, float drop, unsigned long long seed) {
  long long o = q * d.C + c;
  if (!flat) {
    long long r = q;
    const int fo = (int)(r % d.Fo);
    r /= d.Fo;
    const int to = (int)(r % d.To), b = (int)(r / d.To);
    o = pad_px(b, to, fo, d.To, d.Fo) * d.C + c;
  }
  float g = dnext[o];
  if (drop > 0.f) g *= drop_scale(drop, seed, (unsigned long long)(q * d.C + c));
  return g;
}

// part1[chunk][c] = sum dy, part2[chunk][c] = sum dy * xhat
__global__ void __launch_bounds__(256) act_bn_bwd_sums(const float* __restrict__ dnext, int flat,
                                                       const float* __restrict__ P, ActDims d,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, float drop,
                                                       unsigned long long seed,
                                                       float* __restrict__ part1,
                                                       float* __restrict__ part2) {
  const long long npx = (long long)d.B * d.To * d.Fo;
  const long long p0 = (long long)blockIdx.x * ACT_CHUNK;
  const int np = (int)min((long long)ACT_CHUNK, npx - p0);
  for (int c = threadIdx.x; c < d.C; c += 256) {
    const float m = mean[c], rs = rstd[c];
    float s1 = 0.f, s2 = 0.f;
    for (int p = 0; p < np; ++p) {
      const float g = dy_at(dnext, flat, d, p0 + p, c, drop, seed);
      s1 += g;
      s2 += g * ((P[(p0 + p) * d.C + c] - m) * rs);
    }
    part1[(long long)blockIdx.x * d.C + c] = s1;
    part2[(long long)blockIdx.x * d.C + c] = s2;
  }
}

// tot1/2[c] = chunk sums in order; acc1/2[c] += them (nullable)
__global__ void __launch_bounds__(256) act_sum_chunks(const float* __restrict__ part1,
                                                      const float* __restrict__ part2, int nchunk,
                                                      int C, float* __restrict__ tot1,
                                                      float* __restrict__ tot2,
                                                      float* __restrict__ acc1,
                                                      float* __restrict__ acc2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nchunk; ++k) {
    s1 += part1[(long long)k * C + c];
    s2 += part2[(long long)k * C + c];
  }
  tot1[c] = s1;
  tot2[c] = s2;
  if (acc1) acc1[c] += s1;
  if (acc2) acc2[c] += s2;
}

// dz over every pixel of the conv output grid, chunked like the sums:
// part1 = sum dz (conv bias gradient), part2 = sum dy_act * z over z <= 0 (PReLU slope)
__global__ void __launch_bounds__(256) act_bwd_dz(const float* __restrict__ dnext, int flat,
                                                  const float* __restrict__ z,
                                                  const float* __restrict__ P,
                                                  const uint8_t* __restrict__ slot, ActDims d,
                                                  int act, const float* __restrict__ slope_p,
                                                  const float* __restrict__ mean,
                                                  const float* __restrict__ rstd,
                                                  const float* __restrict__ gamma,
                                                  const float* __restrict__ s1,
                                                  const float* __restrict__ s2, int training,
                                                  float drop, unsigned long long seed,
                                                  void* __restrict__ dz, int dz_bf16,
                                                  float* __restrict__ part1,
                                                  float* __restrict__ part2) {
  const long long nz = (long long)d.B * d.T * d.F;
  const long long npool = (long long)d.B * d.To * d.Fo;
  const long long p0 = (long long)blockIdx.x * ACT_CHUNK;
  const int np = (int)min((long long)ACT_CHUNK, nz - p0);
  const float slope = act == ASR_ACT_PRELU ? *slope_p : 0.f;
  const float inv_n = 1.f / (float)npool;
  for (int c = threadIdx.x; c < d.C; c += 256) {
    float m = 0.f, rs = 1.f, ga = 1.f, a1 = 0.f, a2 = 0.f;
    if (mean) {
      m = mean[c];
      rs = rstd[c];
      ga = gamma[c];
      if (training) {
        a1 = s1[c] * inv_n;
        a2 = s2[c] * inv_n;
      }
    }
    float sb = 0.f, ss = 0.f;
    for (int p = 0; p < np; ++p) {
      long long r = p0 + p;
      const int f = (int)(r % d.F);
      r /= d.F;
      const int t = (int)(r % d.T), b = (int)(r / d.T);
      int to = t, fo = f, mine = 0;
      if (d.pt) {
        to = t / d.pt;
        fo = f / d.pf;
        mine = (f - fo * d.pf) * d.pt + (t - to * d.pt);
      }
      float g = 0.f;
      if (to < d.To && fo < d.Fo) {
        const long long q = ((long long)b * d.To + to) * d.Fo + fo;
        if (!d.pt || slot[q * d.C + c] == mine) {
          g = dy_at(dnext, flat, d, q, c, drop, seed);
          if (mean) {
            const float xh = (P[q * d.C + c] - m) * rs;
            g = ga * rs * (g - a1 - xh * a2);
          }
        }
      }
      const long long zi = pad_px(b, t, f, d.T, d.F) * d.C + c;
      const float zv = z[zi];
      float gz;
      if (act == ASR_ACT_PRELU) {
        gz = zv > 0.f ? g : slope * g;
        if (!(zv > 0.f)) ss += g * zv;
      } else if (act == ASR_ACT_HARDTANH) {
        gz = (zv > 0.f && zv < 20.f) ? g : 0.f;
      } else {
        gz = zv > 0.f ? g : 0.f;
      }
      sb += gz;
      if (dz_bf16)
        static_cast<uint16_t*>(dz)[zi] = f2bf(gz);
      else
        static_cast<float*>(dz)[zi] = gz;
    }
    part1[(long long)blockIdx.x * d.C + c] = sb;
    part2[(long long)blockIdx.x * d.C + c] = ss;
  }
}

// dslope += sum over channels, in channel order
__global__ void act_slope_finish(const float* __restrict__ tot, int C, float* __restrict__ dslope) {
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += tot[c];
  *dslope += s;
}

int make_dims(const char* who, int B, int T, int F, int C, int pt, int pf, int ceil_mode,
              ActDims* d) {
  ASR_REQUIRE(B > 0 && T > 0 && F > 0 && C > 0, ASR_ERR_ARG, "%s: bad size", who);
  ASR_REQUIRE((pt == 0 && pf == 0) || (pt >= 1 && pf >= 1 && pt * pf <= 256), ASR_ERR_ARG,
              "%s: bad pool %d x %d", who, pt, pf);
  d->B = B; d->T = T; d->F = F; d->C = C; d->pt = pt; d->pf = pf; d->To = T; d->Fo = F;
  if (pt) {
    const int rc = asr_vgg_pool_dims(T, F, pt, pf, ceil_mode, &d->To, &d->Fo);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(d->To >= 1 && d->Fo >= 1, ASR_ERR_ARG, "%s: pool %d x %d leaves nothing of %d x %d",
                who, pt, pf, T, F);
  }
  return ASR_OK;
}

int nchunks(long long npx) { return ceil_div(npx, ACT_CHUNK); }

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_cnn_act_workspace_bytes(int B, int T, int F, int C) {
  if (B < 1 || T < 1 || F < 1 || C < 1) return 0;
  // two partial arrays over the chunks of the full grid + two per-channel totals
  return ((size_t)2 * nchunks((long long)B * T * F) * C + (size_t)2 * C) * sizeof(float);
}

extern "C" int asr_cnn_act_forward(const float* z, int B, int T, int F, int C, int act,
                                   const float* slope, int pt, int pf, int ceil_mode, float* P,
                                   uint8_t* slot, const float* gamma, const float* beta,
                                   float* run_mean, float* run_var, int training, float momentum,
                                   float eps, float* bn_mean, float* bn_rstd, float drop,
                                   unsigned long long seed, void* out, int out_dtype, int flat,
                                   void* workspace, size_t ws_bytes, void* stream) {
  ActDims d;
  const int rc = make_dims("cnn_act_forward", B, T, F, C, pt, pf, ceil_mode, &d);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(z && P && out && (!pt || slot), ASR_ERR_ARG, "cnn_act_forward: null pointer");
  ASR_REQUIRE(act == ASR_ACT_RELU || act == ASR_ACT_HARDTANH || (act == ASR_ACT_PRELU && slope),
              ASR_ERR_ARG, "cnn_act_forward: bad activation %d", act);
  ASR_REQUIRE(out_dtype == ASR_DT_F32 || (out_dtype == ASR_DT_BF16 && !flat), ASR_ERR_ARG,
              "cnn_act_forward: bad output dtype");
  ASR_REQUIRE(drop >= 0.f && drop < 1.f, ASR_ERR_ARG, "cnn_act_forward: bad dropout %f", drop);
  const bool bn = gamma != nullptr;
  ASR_REQUIRE(!bn || (beta && bn_mean && bn_rstd && (training || (run_mean && run_var))),
              ASR_ERR_ARG, "cnn_act_forward: batch norm needs beta, the stat outputs and (eval) "
              "running stats");
  ASR_REQUIRE(ws_bytes >= asr_cnn_act_workspace_bytes(B, T, F, C) && workspace, ASR_ERR_WORKSPACE,
              "cnn_act_forward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long long npx = (long long)B * d.To * d.Fo, n = npx * C;
  act_pool<<<ceil_div(n, 256), 256, 0, st>>>(z, d, act, slope, P, slot);
  ASR_LAUNCH_CHECK();
  if (bn && training) {
    float* part = (float*)workspace;
    const int nc = nchunks(npx);
    act_moment<<<nc, 256, 0, st>>>(P, npx, C, nullptr, 0, part);
    act_moment_finish<<<ceil_div(C, 256), 256, 0, st>>>(part, nc, C, npx, 0, bn_mean, bn_rstd, eps,
                                                        momentum, nullptr, nullptr);
    act_moment<<<nc, 256, 0, st>>>(P, npx, C, bn_mean, 1, part);
    act_moment_finish<<<ceil_div(C, 256), 256, 0, st>>>(part, nc, C, npx, 1, bn_mean, bn_rstd, eps,
                                                        momentum, run_mean, run_var);
    ASR_LAUNCH_CHECK();
  } else if (bn) {
    act_eval_stats<<<ceil_div(C, 256), 256, 0, st>>>(run_mean, run_var, eps, C, bn_mean, bn_rstd);
    ASR_LAUNCH_CHECK();
  }
  act_apply<<<ceil_div(n, 256), 256, 0, st>>>(P, d, bn ? bn_mean : nullptr, bn_rstd, gamma, beta,
                                              drop, seed, out, out_dtype == ASR_DT_BF16, flat);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_cnn_act_backward(const float* dnext, int flat, const float* z, int B, int T,
                                    int F, int C, int act, const float* slope, int pt, int pf,
                                    int ceil_mode, const float* P, const uint8_t* slot,
                                    const float* gamma, const float* bn_mean, const float* bn_rstd,
                                    int training, float* dgamma, float* dbeta, float drop,
                                    unsigned long long seed, void* dz, int dz_dtype, float* dbias,
                                    float* dslope, void* workspace, size_t ws_bytes, void* stream) {
  ActDims d;
  const int rc = make_dims("cnn_act_backward", B, T, F, C, pt, pf, ceil_mode, &d);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(dnext && z && P && dz && (!pt || slot), ASR_ERR_ARG,
              "cnn_act_backward: null pointer");
  ASR_REQUIRE(act == ASR_ACT_RELU || act == ASR_ACT_HARDTANH || (act == ASR_ACT_PRELU && slope),
              ASR_ERR_ARG, "cnn_act_backward: bad activation %d", act);
  ASR_REQUIRE(dz_dtype == ASR_DT_F32 || dz_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "cnn_act_backward: bad dz dtype");
  const bool bn = gamma != nullptr;
  ASR_REQUIRE(!bn || (bn_mean && bn_rstd), ASR_ERR_ARG, "cnn_act_backward: batch norm stats missing");
  ASR_REQUIRE(ws_bytes >= asr_cnn_act_workspace_bytes(B, T, F, C) && workspace, ASR_ERR_WORKSPACE,
              "cnn_act_backward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long long npx = (long long)B * d.To * d.Fo, nz = (long long)B * T * F;
  const int ncz = nchunks(nz);
  float* part1 = (float*)workspace;
  float* part2 = part1 + (size_t)ncz * C;
  float* tot1 = part2 + (size_t)ncz * C;
  float* tot2 = tot1 + C;
  if (bn) {
    const int nc = nchunks(npx);
    act_bn_bwd_sums<<<nc, 256, 0, st>>>(dnext, flat, P, d, bn_mean, bn_rstd, drop, seed, part1,
                                        part2);
    act_sum_chunks<<<ceil_div(C, 256), 256, 0, st>>>(part1, part2, nc, C, tot1, tot2, dbeta,
                                                     dgamma);
    ASR_LAUNCH_CHECK();
  }
  // the dz pass reads the BN sums from tot1 / tot2; its own partials go to part1 / part2
  act_bwd_dz<<<ncz, 256, 0, st>>>(dnext, flat, z, P, slot, d, act, slope, bn ? bn_mean : nullptr,
                                  bn_rstd, gamma, tot1, tot2, training, drop, seed, dz,
                                  dz_dtype == ASR_DT_BF16, part1, part2);
  ASR_LAUNCH_CHECK();
  if (dbias || (dslope && act == ASR_ACT_PRELU)) {
    // tot1 / tot2 are free again once the dz pass is done (same stream)
    act_sum_chunks<<<ceil_div(C, 256), 256, 0, st>>>(part1, part2, ncz, C, tot1, tot2, dbias,
                                                     nullptr);
    if (dslope && act == ASR_ACT_PRELU) act_slope_finish<<<1, 1, 0, st>>>(tot2, C, dslope);
    ASR_LAUNCH_CHECK();
  }
  return ASR_OK;
}
