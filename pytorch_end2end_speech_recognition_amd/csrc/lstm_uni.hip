// Unidirectional LSTM recurrence for the encoder (gfx950).  Replaces the packed
// nn.LSTM(bidirectional=False) of models/pytorch_v3/encoders/rnn.py (:166-172
// fast path, :218-224 per-layer path) when encoder_bidirectional is False.
//
// Semantics (nn.LSTM, gate order i,f,g,o; h0 = c0 = 0):
//   pre  = gx[b,t] + h_{t-1} @ W_hh^T         (gx = x @ W_ih^T + b_ih + b_hh, one GEMM)
//   c    = sig(f) * c_{t-1} + sig(i) * tanh(g),  h = sig(o) * tanh(c)
// Packed-sequence behaviour through per-utterance length masks: for
// t >= lens[b] the state and the output are 0 (pad_packed's zeros).
//
// One launch per time step and pass; the stream orders the steps, no
// work-group waits on another.  The recurrent operand of step t is what step
// t -+ 1 stored to the pass's own output: the forward reads h_{t-1} from
// y[b][t-1], the backward reads dG_{t+1} from act_dg[b][t+1], both f32 and, in
// bf16 mode, rounded to bf16 as they are loaded into MFMA fragments.  No
// ping-pong state, no workspace that must be zero: the first step skips the
// product instead.
//
// Forward work-group (256 threads): 4 hidden units x 4 gates = 16 gate columns
// x 32 utterances; its 4 waves split K = H and combine through LDS (8 KB), so
// the 16x16 MFMA tile holds all four gates of its units and the cell update
// runs in the same kernel.  grid = (ceil(H/4), ceil(B/32)).  The product, the
// combine and the gate pre-activations are lstm_uni_step.h's uni_gate_partials
// and uni_gate_pre, which lstm_stream.hip's step calls too; the fragment
// loaders are there as well.
// Backward work-group (512 threads): 16 units x 16 utterances, its 8 waves
// split K = 4H over dG_{t+1} times a transposed copy of W_hh (each lane's
// 8-element fragment contiguous), LDS 8 KB.  grid = (ceil(H/16), ceil(B/16)).
#include "lstm_uni_step.h"
#include "prof.h"

extern "C" size_t asr_colsum_workspace_bytes(int M, int N);
extern "C" int asr_colsum_accumulate(const float* g, long long ld, int M, int N, float alpha,
                                     float* out0, float* out1, void* workspace, size_t ws_bytes,
                                     void* stream);

namespace asr {
namespace {

constexpr int UBU = 16;    // backward: units per work-group
constexpr int UBB = 16;    // backward: utterances per work-group
constexpr int UNI_MAX_H = 1024;
constexpr int UNI_MAX_B = 8192;
constexpr int UNI_MAX_T = 65536;

// ---------------------------------------------------------------------------
// forward step t.  grid = (ceil(H / UFU), ceil(B / UFB)), block = 256
// ---------------------------------------------------------------------------
template <bool BF16, typename TW>
__global__ void __launch_bounds__(256) lstm_uni_fwd_step(
    int t, int B, int T, int H, const int32_t* __restrict__ lens, const TW* __restrict__ whh,
    float* __restrict__ gx_act, float* __restrict__ y, float* __restrict__ cst,
    uint16_t* __restrict__ ybf) {
  __shared__ float part[4][UFB][16];
  const int u0 = blockIdx.x * UFU;
  const int b0 = blockIdx.y * UFB;
  const int tid = threadIdx.x, lane = tid & 63;
  // A rows: h_{t-1} = y[.][t-1] of utterances b0 + (l & 15) and b0 + 16 +
  // (l & 15) (t = 0 has none: the product is skipped, the rows are not read);
  // B rows: W_hh row g*H + u of gate column n = l & 15 (g = n >> 2, u = u0 +
  // (n & 3))
  const int ra = b0 + (lane & 15), rb = ra + 16, tp = max(t - 1, 0);
  const float* a0 = ra < B ? y + ((long long)ra * T + tp) * H : nullptr;
  const float* a1 = rb < B ? y + ((long long)rb * T + tp) * H : nullptr;
  const int n = lane & 15, u = u0 + (n & 3);
  const TW* br = u < H ? whh + ((long long)(n >> 2) * H + u) * H : nullptr;
  uni_gate_partials<BF16>(a0, a1, br, t == 0, H, part);
  if (tid >= UFB * UFU) return;
  const int b = b0 + (tid >> 2), j = u0 + (tid & 3);
  if (b >= B || j >= H) return;
  const bool active = t < lens[b];
  const long long gbase = ((long long)b * T + t) * 4 * H + j;
  const long long sidx = ((long long)b * T + t) * H + j;
  float pre[4];
  uni_gate_pre(part, gx_act + gbase, H, pre);
  const float cprev = t > 0 ? cst[sidx - H] : 0.f;
  const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]);
  const float gg = tanhf_(pre[2]), og = sigmoidf_(pre[3]);
  float c = fg * cprev + ig * gg;
  float h = og * tanhf_(c);
  if (!active) { c = 0.f; h = 0.f; }
  y[sidx] = h;
  cst[sidx] = c;
  if (ybf) ybf[sidx] = f2bf(h);
  gx_act[gbase] = active ? ig : 0.f;
  gx_act[gbase + H] = active ? fg : 0.f;
  gx_act[gbase + 2 * H] = active ? gg : 0.f;
  gx_act[gbase + 3 * H] = active ? og : 0.f;
}

// ---------------------------------------------------------------------------
// backward step t (launched for t = T-1 .. 0).  grid = (ceil(H / UBU),
// ceil(B / UBB)), block = 512.  wt: W_hh^T [H][4H] in the compute dtype.
// dc [B][H]: d loss / d c_t carried to step t - 1 (not read at t = T - 1).
// ---------------------------------------------------------------------------
template <bool BF16, typename TS>
__global__ void __launch_bounds__(512) lstm_uni_bwd_step(
    int t, int B, int T, int H, const int32_t* __restrict__ lens, const TS* __restrict__ wt,
    const float* __restrict__ dy, float* __restrict__ act_dg, const float* __restrict__ cst,
    float* __restrict__ dc, uint16_t* __restrict__ dgbf) {
  __shared__ float part[8][UBB][16];
  const int u0 = blockIdx.x * UBU;
  const int b0 = blockIdx.y * UBB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H4 = 4 * H;
  const bool last = t == T - 1;
  const bool vec = (H & 7) == 0;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (!last) {
    // dh[b][j] += sum_n dG_{t+1}[b][n] W_hh[n][j]: A rows dG_{t+1} of utterance
    // b0 + (l & 15), B rows W_hh^T row j = u0 + (l & 15)
    const int ra = b0 + (lane & 15), jl = u0 + (lane & 15);
    const float* ar = ra < B ? act_dg + ((long long)ra * T + (t + 1)) * H4 : nullptr;
    const TS* br = jl < H ? wt + (long long)jl * H4 : nullptr;
    if constexpr (BF16) {
      for (int k0 = wave * 32; k0 < H4; k0 += 8 * 32) {
        const int k = k0 + 8 * (lane >> 4);
        acc = mfma_bf16(ufrag8(ar, k, H4, vec), ufrag8(br, k, H4, vec), acc);
      }
    } else {
      for (int k0 = wave * 4; k0 < H4; k0 += 8 * 4) {
        const int k = k0 + (lane >> 4);
        acc = mfma_f32(ufrag1(ar, k, H4), ufrag1(br, k, H4), acc);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][4 * (lane >> 4) + r][lane & 15] = acc[r];
  __syncthreads();
  if (tid >= UBB * UBU) return;
  const int row = tid >> 4, uu = tid & 15;
  const int b = b0 + row, j = u0 + uu;
  if (b >= B || j >= H) return;
  const long long gbase = ((long long)b * T + t) * H4 + j;
  const long long sidx = ((long long)b * T + t) * H + j;
  const long long cidx = (long long)b * H + j;
  float d[4] = {0.f, 0.f, 0.f, 0.f}, dcn = 0.f;
  if (t < lens[b]) {
    float dh = dy ? dy[sidx] : 0.f;
    dh += ((part[0][row][uu] + part[1][row][uu]) + (part[2][row][uu] + part[3][row][uu])) +
          ((part[4][row][uu] + part[5][row][uu]) + (part[6][row][uu] + part[7][row][uu]));
    const float ig = act_dg[gbase], fg = act_dg[gbase + H], gg = act_dg[gbase + 2 * H],
                og = act_dg[gbase + 3 * H];
    const float c = cst[sidx];
    const float cprev = t > 0 ? cst[sidx - H] : 0.f;
    const float tc = tanhf_(c);
    const float dcell = (last ? 0.f : dc[cidx]) + dh * og * (1.f - tc * tc);
    d[0] = dcell * gg * ig * (1.f - ig);
    d[1] = dcell * cprev * fg * (1.f - fg);
    d[2] = dcell * ig * (1.f - gg * gg);
    d[3] = dh * tc * og * (1.f - og);
    dcn = dcell * fg;
  }
  dc[cidx] = dcn;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    act_dg[gbase + (long long)q * H] = d[q];
    if (dgbf) dgbf[gbase + (long long)q * H] = f2bf(d[q]);
  }
}

__device__ __forceinline__ void st(float* p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st(uint16_t* p, long long i, float v) { p[i] = f2bf(v); }

// W_hh [4H][H] (f32 or bf16) -> W_hh^T [H][4H] in the compute dtype.
template <typename TW, typename TS>
__global__ void __launch_bounds__(256) uni_transpose_whh(const TW* __restrict__ w, int H,
                                                         TS* __restrict__ out) {
  __shared__ float tile[32][33];
  const int R = 4 * H, C = H;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? ldw(w, (long long)r * C + c) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < R) st(out, (long long)c * R + r, tile[tx][i]);
  }
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// forward workspace: [bf16 copy of W_hh (bf16 mode, for f32 weights)]
size_t uni_fwd_ws(int H, int cdt) {
  return cdt == ASR_DT_BF16 ? al256((size_t)4 * H * H * 2) : 256;
}
// backward workspace: [W_hh^T, compute dtype][dc f32 B x H][column-sum partials 64 x 4H f32]
struct UniBwdLayout {
  size_t dc, bias, total;
};
UniBwdLayout uni_bwd_layout(int B, int H, int cdt) {
  UniBwdLayout l;
  l.dc = al256((size_t)4 * H * H * (cdt == ASR_DT_BF16 ? 2 : 4));
  l.bias = l.dc + al256((size_t)B * H * 4);
  l.total = l.bias + (size_t)64 * 4 * H * 4;
  return l;
}

bool uni_shape_ok(int B, int T, int H) {
  return B >= 1 && B <= UNI_MAX_B && T >= 1 && T <= UNI_MAX_T && H >= 1 && H <= UNI_MAX_H;
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_lstm_uni_shape_ok(int B, int T, int H) { return uni_shape_ok(B, T, H) ? 1 : 0; }

extern "C" size_t asr_lstm_uni_workspace_bytes(int B, int H, int compute_dtype, int backward) {
  if (B < 1 || H < 1) return 0;
  return backward ? uni_bwd_layout(B, H, compute_dtype).total : uni_fwd_ws(H, compute_dtype);
}

extern "C" int asr_lstm_uni_forward(float* gx_act, const void* whh, int w_dtype,
                                    const int32_t* lens, int B, int T, int H, int compute_dtype,
                                    float* y, float* cst, uint16_t* ybf, void* workspace,
                                    size_t ws_bytes, void* stream) {
  ASR_REQUIRE(gx_act && whh && lens && y && cst && workspace, ASR_ERR_ARG,
              "lstm_uni_forward: null pointer");
  ASR_REQUIRE(B > 0 && T > 0 && H > 0, ASR_ERR_ARG, "lstm_uni_forward: bad shape");
  ASR_REQUIRE(compute_dtype == ASR_DT_F32 || compute_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_uni_forward: compute dtype %d", compute_dtype);
  ASR_REQUIRE(w_dtype == ASR_DT_F32 || w_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_uni_forward: weight dtype %d", w_dtype);
  const bool bf = compute_dtype == ASR_DT_BF16;
  ASR_REQUIRE(bf || w_dtype == ASR_DT_F32, ASR_ERR_ARG, "lstm_uni_forward: f32 compute needs f32 W");
  ASR_REQUIRE(uni_shape_ok(B, T, H), ASR_ERR_UNSUPPORTED,
              "lstm_uni_forward: B %d T %d H %d outside B <= %d, T <= %d, H <= %d",
              B, T, H, UNI_MAX_B, UNI_MAX_T, UNI_MAX_H);
  ASR_REQUIRE(ws_bytes >= uni_fwd_ws(H, compute_dtype), ASR_ERR_WORKSPACE,
              "lstm_uni_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const uint16_t* wbf = (const uint16_t*)whh;
  if (bf && w_dtype == ASR_DT_F32) {
    // one conversion pass: the T step launches stream 2 bytes per weight
    const long long n = 4LL * H * H;
    hipLaunchKernelGGL(uni_to_bf16, dim3(ceil_div(n, 256)), dim3(256), 0, s, (const float*)whh,
                       (uint16_t*)workspace, n);
    ASR_LAUNCH_CHECK();
    wbf = (const uint16_t*)workspace;
  }
  const dim3 grid(ceil_div(H, UFU), ceil_div(B, UFB));
  for (int t = 0; t < T; ++t) {
    const int slot = prof_begin_launch(ASR_PROF_LSTM_FWD, s);
    if (bf)
      hipLaunchKernelGGL((lstm_uni_fwd_step<true, uint16_t>), grid, dim3(256), 0, s, t, B, T, H,
                         lens, wbf, gx_act, y, cst, ybf);
    else
      hipLaunchKernelGGL((lstm_uni_fwd_step<false, float>), grid, dim3(256), 0, s, t, B, T, H, lens,
                         (const float*)whh, gx_act, y, cst, ybf);
    ASR_LAUNCH_CHECK();
    prof_end_launch(ASR_PROF_LSTM_FWD, slot, s);
  }
  return ASR_OK;
}

extern "C" int asr_lstm_uni_backward(const float* dy, const void* whh, int w_dtype,
                                     const int32_t* lens, int B, int T, int H, int compute_dtype,
                                     float* act_dg, const float* cst, uint16_t* dgbf, float* db_ih,
                                     float* db_hh, void* workspace, size_t ws_bytes,
                                     void* stream) {
  ASR_REQUIRE(whh && lens && act_dg && cst && db_ih && workspace, ASR_ERR_ARG,
              "lstm_uni_backward: null pointer");
  ASR_REQUIRE(B > 0 && T > 0 && H > 0, ASR_ERR_ARG, "lstm_uni_backward: bad shape");
  ASR_REQUIRE(compute_dtype == ASR_DT_F32 || compute_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_uni_backward: compute dtype %d", compute_dtype);
  ASR_REQUIRE(w_dtype == ASR_DT_F32 || w_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_uni_backward: weight dtype %d", w_dtype);
  const bool bf = compute_dtype == ASR_DT_BF16;
  ASR_REQUIRE(bf || w_dtype == ASR_DT_F32, ASR_ERR_ARG,
              "lstm_uni_backward: f32 compute needs f32 W");
  ASR_REQUIRE(uni_shape_ok(B, T, H), ASR_ERR_UNSUPPORTED,
              "lstm_uni_backward: B %d T %d H %d outside B <= %d, T <= %d, H <= %d",
              B, T, H, UNI_MAX_B, UNI_MAX_T, UNI_MAX_H);
  const UniBwdLayout L = uni_bwd_layout(B, H, compute_dtype);
  ASR_REQUIRE(ws_bytes >= L.total, ASR_ERR_WORKSPACE, "lstm_uni_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  void* wt = base;
  float* dcb = (float*)(base + L.dc);
  const dim3 tg(ceil_div(H, 32), ceil_div(4 * H, 32));
  if (!bf)
    hipLaunchKernelGGL((uni_transpose_whh<float, float>), tg, dim3(256), 0, s, (const float*)whh, H,
                       (float*)wt);
  else if (w_dtype == ASR_DT_BF16)
    hipLaunchKernelGGL((uni_transpose_whh<uint16_t, uint16_t>), tg, dim3(256), 0, s,
                       (const uint16_t*)whh, H, (uint16_t*)wt);
  else
    hipLaunchKernelGGL((uni_transpose_whh<float, uint16_t>), tg, dim3(256), 0, s,
                       (const float*)whh, H, (uint16_t*)wt);
  ASR_LAUNCH_CHECK();
  const dim3 grid(ceil_div(H, UBU), ceil_div(B, UBB));
  for (int t = T - 1; t >= 0; --t) {
    const int slot = prof_begin_launch(ASR_PROF_LSTM_BWD, s);
    if (bf)
      hipLaunchKernelGGL((lstm_uni_bwd_step<true, uint16_t>), grid, dim3(512), 0, s, t, B, T, H,
                         lens, (const uint16_t*)wt, dy, act_dg, cst, dcb, dgbf);
    else
      hipLaunchKernelGGL((lstm_uni_bwd_step<false, float>), grid, dim3(512), 0, s, t, B, T, H, lens,
                         (const float*)wt, dy, act_dg, cst, dcb, dgbf);
    ASR_LAUNCH_CHECK();
    prof_end_launch(ASR_PROF_LSTM_BWD, slot, s);
  }
  // db_ih[n] += sum_{b,t} dG[b][t][n], db_hh the same: fixed-order column sums
  // (B * T <= UNI_MAX_B * UNI_MAX_T = 2^29 rows)
  return asr_colsum_accumulate(act_dg, 4 * H, B * T, 4 * H, 1.f, db_ih, db_hh, base + L.bias,
                               L.total - L.bias, stream);
}
