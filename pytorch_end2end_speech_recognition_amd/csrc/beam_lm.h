// The RNN language model of the two device beam searches (csrc/att_beam.hip,
// csrc/ctc_beam.hip): stacked LSTM layers (torch's gate rows i, f, g, o), the
// output layer and its f32 log-sum-exp, and the host-side checks of an
// asr_att_beam_lm_t.  Each search keeps its own kernels, its workspace and the
// way it finds a row's parent state; the arithmetic is here (beam_lm_cell of the
// attention search keeps a copy of lm_lstm_step's loop and says why).
#pragma once
#include "common.h"

namespace asr {
namespace {

constexpr int kMaxLmLayers = ASR_ATT_BEAM_LM_MAX_LAYERS;
constexpr size_t kLdsLimit = 64 * 1024;
constexpr int LM_THREADS = 256;

struct LmNet {
  int layers, H, Y, V;
  const float* emb;        // [V][Y]
  const float *w_ih[kMaxLmLayers], *w_hh[kMaxLmLayers];   // [4H][Y or H], [4H][H]
  const float *b_ih[kMaxLmLayers], *b_hh[kMaxLmLayers];   // [4H]
  const float *w_out, *b_out;   // [V][H], [V]
};

// lm_lstm_step's LDS need
__host__ __device__ inline size_t lm_cell_lds_floats(int Y, int H) {
  return 2 * (size_t)(Y > H ? Y : H) + H;
}

// How one search words its refusals: the prefix of a decode call's texts and of
// the shape limits' (the attention search reports those as att_beam_lm from the
// query and the call alike), and what it calls the dimensions and its classes.
struct LmWho {
  const char *call, *shape, *dims, *classes, *classes_note;
};

// the LM's shape limits: all a workspace query knows of it
inline int lm_net_shape_check(int layers, int H, int Y, const LmWho& who) {
  ASR_REQUIRE(layers >= 1 && H > 0 && Y > 0, ASR_ERR_ARG, "%s: bad %s (layers %d, H %d, Y %d)",
              who.shape, who.dims, layers, H, Y);
  ASR_REQUIRE(layers <= kMaxLmLayers, ASR_ERR_UNSUPPORTED, "%s: %d LM layers > %d", who.shape,
              layers, kMaxLmLayers);
  const size_t lc = lm_cell_lds_floats(Y, H) * 4;
  ASR_REQUIRE(lc <= kLdsLimit, ASR_ERR_UNSUPPORTED, "%s: LDS need (lm cell %zu B) > %zu B",
              who.shape, lc, kLdsLimit);
  return ASR_OK;
}

// a decode call's LM against the search's V classes; lm->weight is the caller's to judge
inline int lm_net_check(const asr_att_beam_lm_t* lm, int V, const LmWho& who) {
  ASR_REQUIRE(lm->V == V, ASR_ERR_ARG, "%s: the LM has %d classes, the %s %d%s", who.call, lm->V,
              who.classes, V, who.classes_note);
  const int rc = lm_net_shape_check(lm->layers, lm->H, lm->Y, who);
  if (rc != ASR_OK) return rc;
  ASR_REQUIRE(lm->cell == ASR_ATT_BEAM_CELL_LSTM, ASR_ERR_UNSUPPORTED,
              "%s: only an LSTM language model runs on the device (cell %d)", who.call, lm->cell);
  ASR_REQUIRE(lm->emb && lm->w_out && lm->b_out, ASR_ERR_ARG, "%s: null pointer", who.call);
  for (int l = 0; l < lm->layers; ++l)
    ASR_REQUIRE(lm->w_ih[l] && lm->w_hh[l] && lm->b_ih[l] && lm->b_hh[l], ASR_ERR_ARG,
                "%s: null pointer (layer %d)", who.call, l);
  return ASR_OK;
}

inline LmNet lm_net_from(const asr_att_beam_lm_t* lm) {
  LmNet m = {};
  m.layers = lm->layers; m.H = lm->H; m.Y = lm->Y; m.V = lm->V;
  m.emb = lm->emb; m.w_out = lm->w_out; m.b_out = lm->b_out;
  for (int l = 0; l < lm->layers; ++l) {
    m.w_ih[l] = lm->w_ih[l]; m.w_hh[l] = lm->w_hh[l];
    m.b_ih[l] = lm->b_ih[l]; m.b_hh[l] = lm->b_hh[l];
  }
  return m;
}

// One step of the stacked LSTM on token `tok` by a work-group of LM_THREADS:
// ph / pc are the parent's h / c of all layers ([layers][H]; null: the zero
// state), oh / oc take the new ones, sm holds lm_cell_lds_floats(Y, H) floats.
// xa / xb alternate as a layer's input and output; hp is the parent's h of the
// layer.  Returns the top layer's h in LDS, complete for the whole work-group.
__device__ __forceinline__ const float* lm_lstm_step(const LmNet& m, int tok, const float* ph,
                                                     const float* pc, float* oh, float* oc,
                                                     float* sm) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = LM_THREADS / 64;
  const int H = m.H, XM = max(m.Y, H);
  float* xa = sm;            // [max(Y, H)]
  float* xb = xa + XM;       // [max(Y, H)]
  float* hp = xb + XM;       // [H]
  for (int y = tid; y < m.Y; y += LM_THREADS) xa[y] = m.emb[(long long)tok * m.Y + y];
  for (int l = 0; l < m.layers; ++l) {
    const int in = l == 0 ? m.Y : H;
    const long long so = (long long)l * H;
    for (int j = tid; j < H; j += LM_THREADS) hp[j] = ph ? ph[so + j] : 0.f;
    __syncthreads();
    const float* wi_l = m.w_ih[l];
    const float* wh_l = m.w_hh[l];
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
        s[g] = wave_sum(a) + m.b_ih[l][row] + m.b_hh[l][row];
      }
      if (lane == 0) {
        const float ig = sigmoidf_(s[0]), fg = sigmoidf_(s[1]);
        const float gg = tanhf_(s[2]), og = sigmoidf_(s[3]);
        const float cn = fg * (pc ? pc[so + u] : 0.f) + ig * gg;
        const float hn = og * tanhf_(cn);
        oc[so + u] = cn;
        oh[so + u] = hn;
        xb[u] = hn;
      }
    }
    __syncthreads();         // xb is complete; xa and hp are free
    float* sw = xa;
    xa = xb;
    xb = sw;
  }
  return xa;
}

// v, equal within each wave, reduced over the work-group's LM_THREADS / 64
// waves in wave order; red holds one float per wave.  The leading barrier
// makes red reusable from one call to the next.
template <bool MAX>
__device__ __forceinline__ float lm_cross_wave(float v, float* red) {
  constexpr int nw = LM_THREADS / 64;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int i = 1; i < nw; ++i) v = MAX ? fmaxf(v, red[i]) : v + red[i];
  return v;
}

// The output layer on h ([H], LDS): the V logits to the global row lg, one wave
// per class, then their maximum mx and lse = log(sum(exp(lg - mx))); lg is
// visible to the whole work-group on return.  WaveSum is the caller's sum over
// a wave's lanes: the two searches add the lanes in different orders (DPP rows
// there, an xor butterfly here), and each keeps the bits it has always produced.
template <float (*WaveSum)(float)>
__device__ __forceinline__ void lm_output_lse(const LmNet& m, const float* h, float* lg, float* red,
                                              float& mx, float& lse) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = LM_THREADS / 64;
  const int H = m.H;
  mx = neg_inf();
  for (int v = w; v < m.V; v += nw) {      // one wave per class
    const float* wr = m.w_out + (long long)v * H;
    float s = 0.f;
    for (int k = lane; k < H; k += 64) s += wr[k] * h[k];
    s = wave_sum(s) + m.b_out[v];
    if (lane == 0) lg[v] = s;
    mx = fmaxf(mx, s);
  }
  // s, hence mx, is equal within a wave; the barriers also publish lg to the work-group
  mx = lm_cross_wave<true>(mx, red);
  float se = 0.f;
  for (int v = tid; v < m.V; v += LM_THREADS) se += expf(lg[v] - mx);
  lse = logf(lm_cross_wave<false>(WaveSum(se), red));
}

}  // namespace
}  // namespace asr
