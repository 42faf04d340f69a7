// Stateful unidirectional LSTM recurrence for chunk-by-chunk (streaming)
// inference on gfx950: lstm_uni.hip's forward step with the state carried in
// and out of the call instead of starting from zero.
//
// Semantics (gate order i,f,g,o; asr_hip.h, asr_lstm_stream_forward):
//   pre  = gx[b,t] + h_{t-1} @ W_hh^T,  h_{-1} = h_in[b], c_{-1} = c_in[b]
//   c    = sig(f) * c_{t-1} + sig(i) * tanh(g),  h = sig(o) * tanh(c)   (t < lens[b])
// For t >= lens[b] the output is 0 and the state is FROZEN (lstm_uni.hip zeroes
// it): h_out / c_out hold the state after frame lens[b] - 1, or h_in / c_in
// when lens[b] == 0, so the next chunk of that utterance continues from it.
// Inference only: gx is read only, no gate activations and no [B][T][H] cell
// state are written.
//
// Structure as lstm_uni.hip: one launch per time step, the stream orders the
// steps, no work-group waits on another.  Step 0 reads h_{-1} from h_in, step
// t > 0 reads h_{t-1} from y[b][t-1] (f32, rounded to bf16 as it is loaded
// into MFMA fragments in bf16 mode), so a chunk boundary changes where the
// operand is read from and nothing about its value or the order of the sums:
// every chunk schedule of an utterance gives the same bits.
//
// The cell state lives in c_out between the steps: thread (b, j) of step t is
// the only reader and the only writer of c[b][j] in that launch (it reads
// c_in[b][j] at t = 0, c_out[b][j] after), so c_out may alias c_in.  h_out may
// NOT alias h_in: with lens[b] == 1, step 0 reads all of h_in[b] in every
// work-group of the row while the work-groups write their units of h_out[b].
//
// Work-group (256 threads): 4 hidden units x 4 gates = 16 gate columns x 32
// utterances, the 4 waves split K = H and combine through LDS (8 KB), then 128
// threads do the (scalar) cell math.  grid = (ceil(H/4), ceil(B/32)).  The
// product, the combine and the gate pre-activations are not a copy of
// lstm_uni.hip's: both steps call lstm_uni_step.h's uni_gate_partials and
// uni_gate_pre, so the two cannot drift apart.  This kernel's own: where
// h_{t-1} is read from, the cell update, the frozen state and the stores.
#include "lstm_uni_step.h"

extern "C" int asr_lstm_uni_shape_ok(int B, int T, int H);

namespace asr {
namespace {

// ---------------------------------------------------------------------------
// step t of a chunk of Tc frames.  grid = (ceil(H / UFU), ceil(B / UFB)),
// block = 256.  c_in / c_out may be one buffer (see the head of the file), so
// neither is __restrict__.
// ---------------------------------------------------------------------------
template <bool BF16, typename TW>
__global__ void __launch_bounds__(256) lstm_stream_step(
    int t, int B, int Tc, int H, const int32_t* __restrict__ lens, const TW* __restrict__ whh,
    const float* __restrict__ gx, float* __restrict__ y, const float* __restrict__ h_in,
    const float* c_in, float* __restrict__ h_out, float* c_out) {
  __shared__ float part[4][UFB][16];
  const int u0 = blockIdx.x * UFU;
  const int b0 = blockIdx.y * UFB;
  const int tid = threadIdx.x, lane = tid & 63;
  // A rows: h_{t-1} of utterances b0 + (l & 15) and b0 + 16 + (l & 15), from
  // h_in at t = 0 and from y[.][t-1] after; B rows: W_hh row g*H + u of gate
  // column n = l & 15 (g = n >> 2, u = u0 + (n & 3))
  const int ra = b0 + (lane & 15), rb = ra + 16;
  const float* hp = t > 0 ? y + (long long)(t - 1) * H : h_in;
  const long long hs = t > 0 ? (long long)Tc * H : (long long)H;
  const float* a0 = ra < B ? hp + ra * hs : nullptr;
  const float* a1 = rb < B ? hp + rb * hs : nullptr;
  const int n = lane & 15, u = u0 + (n & 3);
  const TW* br = u < H ? whh + ((long long)(n >> 2) * H + u) * H : nullptr;
  uni_gate_partials<BF16>(a0, a1, br, false, H, part);
  if (tid >= UFB * UFU) return;
  const int b = b0 + (tid >> 2), j = u0 + (tid & 3);
  if (b >= B || j >= H) return;
  const int lb = min(max(lens[b], 0), Tc);
  const long long yidx = ((long long)b * Tc + t) * H + j;
  const long long sidx = (long long)b * H + j;
  if (t >= lb) {
    // padded frame: zero output, frozen state (copied through once, at t = 0)
    y[yidx] = 0.f;
    if (t == 0) {
      h_out[sidx] = h_in[sidx];
      c_out[sidx] = c_in[sidx];
    }
    return;
  }
  float pre[4];
  uni_gate_pre(part, gx + ((long long)b * Tc + t) * 4 * H + j, H, pre);
  const float cprev = t > 0 ? c_out[sidx] : c_in[sidx];
  const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]);
  const float gg = tanhf_(pre[2]), og = sigmoidf_(pre[3]);
  const float c = fg * cprev + ig * gg;
  const float h = og * tanhf_(c);
  y[yidx] = h;
  c_out[sidx] = c;
  if (t == lb - 1) h_out[sidx] = h;
}

size_t stream_ws(int H, int cdt) {
  const size_t n = (size_t)4 * H * H * 2;
  return cdt == ASR_DT_BF16 ? (n + 255) & ~size_t(255) : 256;
}

// [a, a + na) and [b, b + nb) floats share a byte
bool ranges_overlap(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb * sizeof(float) && y < x + na * sizeof(float);
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_lstm_stream_workspace_bytes(int B, int H, int compute_dtype) {
  if (B < 1 || H < 1) return 0;
  return stream_ws(H, compute_dtype);
}

extern "C" int asr_lstm_stream_forward(const float* gx, const void* whh, int w_dtype,
                                       const int32_t* lens, int B, int Tc, int H,
                                       int compute_dtype, const float* h_in, const float* c_in,
                                       float* h_out, float* c_out, float* y, void* workspace,
                                       size_t ws_bytes, void* stream) {
  ASR_REQUIRE(gx && whh && lens && h_in && c_in && h_out && c_out && y, ASR_ERR_ARG,
              "lstm_stream_forward: null pointer");
  ASR_REQUIRE(B > 0 && Tc > 0 && H > 0, ASR_ERR_ARG, "lstm_stream_forward: bad shape");
  ASR_REQUIRE(compute_dtype == ASR_DT_F32 || compute_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_stream_forward: compute dtype %d", compute_dtype);
  ASR_REQUIRE(w_dtype == ASR_DT_F32 || w_dtype == ASR_DT_BF16, ASR_ERR_ARG,
              "lstm_stream_forward: weight dtype %d", w_dtype);
  const bool bf = compute_dtype == ASR_DT_BF16;
  ASR_REQUIRE(bf || w_dtype == ASR_DT_F32, ASR_ERR_ARG,
              "lstm_stream_forward: f32 compute needs f32 W");
  ASR_REQUIRE(asr_lstm_uni_shape_ok(B, Tc, H) == 1, ASR_ERR_UNSUPPORTED,
              "lstm_stream_forward: B %d Tc %d H %d outside the shapes asr_lstm_uni_shape_ok "
              "accepts", B, Tc, H);
  const size_t nst = (size_t)B * H;
  ASR_REQUIRE(!ranges_overlap(h_in, nst, h_out, nst), ASR_ERR_ARG,
              "lstm_stream_forward: h_out aliases h_in (step 0 reads all of h_in[b] in every "
              "work-group of the row while h_out[b] is written)");
  ASR_REQUIRE(c_in == c_out || !ranges_overlap(c_in, nst, c_out, nst), ASR_ERR_ARG,
              "lstm_stream_forward: c_out overlaps c_in without being c_in");
  // every other pair of an output with an output or an input: y, h_out, c_out
  // against each other, and against gx, h_in, c_in
  const size_t ny = nst * Tc;
  ASR_REQUIRE(!ranges_overlap(y, ny, h_out, nst) && !ranges_overlap(y, ny, c_out, nst) &&
                  !ranges_overlap(h_out, nst, c_out, nst),
              ASR_ERR_ARG, "lstm_stream_forward: y, h_out and c_out overlap each other");
  ASR_REQUIRE(!ranges_overlap(y, ny, h_in, nst) && !ranges_overlap(y, ny, c_in, nst) &&
                  !ranges_overlap(h_out, nst, c_in, nst) && !ranges_overlap(c_out, nst, h_in, nst),
              ASR_ERR_ARG, "lstm_stream_forward: an output overlaps the input state");
  ASR_REQUIRE(!ranges_overlap(gx, 4 * ny, y, ny) && !ranges_overlap(gx, 4 * ny, h_out, nst) &&
                  !ranges_overlap(gx, 4 * ny, c_out, nst),
              ASR_ERR_ARG, "lstm_stream_forward: an output overlaps gx");
  const bool convert = bf && w_dtype == ASR_DT_F32;
  // bf16 mode's vector fragment loads (H % 8 == 0) read 16-B aligned groups of
  // the rows of h and of the bf16 W_hh
  ASR_REQUIRE(!bf || (H & 7) != 0 ||
                  (((uintptr_t)h_in | (uintptr_t)y | (convert ? 0 : (uintptr_t)whh)) & 15) == 0,
              ASR_ERR_ARG, "lstm_stream_forward: h_in, y and a bf16 whh must be 16-byte aligned");
  if (convert) {
    ASR_REQUIRE(workspace && ws_bytes >= stream_ws(H, compute_dtype), ASR_ERR_WORKSPACE,
                "lstm_stream_forward: workspace too small");
    ASR_REQUIRE(((uintptr_t)workspace & 15) == 0, ASR_ERR_ARG,
                "lstm_stream_forward: workspace must be 16-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  const uint16_t* wbf = (const uint16_t*)whh;
  if (convert) {
    // a caller that streams many chunks passes a bf16 W_hh instead (w_dtype)
    const long long n = 4LL * H * H;
    hipLaunchKernelGGL(uni_to_bf16, dim3(ceil_div(n, 256)), dim3(256), 0, s, (const float*)whh,
                       (uint16_t*)workspace, n);
    ASR_LAUNCH_CHECK();
    wbf = (const uint16_t*)workspace;
  }
  const dim3 grid(ceil_div(H, UFU), ceil_div(B, UFB));
  for (int t = 0; t < Tc; ++t) {
    // (not recorded by the launch profiler: its per-step slot is the training
    // forward's, and a process may train and stream)
    if (bf)
      hipLaunchKernelGGL((lstm_stream_step<true, uint16_t>), grid, dim3(256), 0, s, t, B, Tc, H,
                         lens, wbf, gx, y, h_in, c_in, h_out, c_out);
    else
      hipLaunchKernelGGL((lstm_stream_step<false, float>), grid, dim3(256), 0, s, t, B, Tc, H,
                         lens, (const float*)whh, gx, y, h_in, c_in, h_out, c_out);
    ASR_LAUNCH_CHECK();
  }
  return ASR_OK;
}
