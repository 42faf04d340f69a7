// What the unidirectional LSTM recurrences share (lstm_uni.hip: training,
// state from zero; lstm_stream.hip: inference, state carried between calls):
// the MFMA fragment loaders, the forward step's tile, its recurrent product
// h_{t-1} @ W_hh^T and the gate pre-activations, and the f32 -> bf16 weight
// conversion.  The streaming contract -- any chunking of an utterance gives the
// whole-utterance bits -- rests on both forward steps forming `pre` by this one
// definition; the cell update, the masking and the stores are each kernel's own.
#pragma once
#include "mfma.h"

namespace asr {
namespace {

constexpr int UFU = 4;     // forward: units per work-group (16 gate columns)
constexpr int UFB = 32;    // forward: utterances per work-group

__device__ __forceinline__ float ldw(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float ldw(const uint16_t* p, long long i) { return bf2f(p[i]); }

// 8 consecutive elements [k, k + 8) of a row as a bf16 fragment, zeros from K
// on and for a nullptr row.  vec (H % 8 == 0: rows 16-B aligned, K a multiple
// of 8, so a fragment is whole or empty): vector loads.
__device__ __forceinline__ bf16x8 ufrag8_tail(const float* row, int k, int K) {
  u16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (k + j < K) ? f2bf(row[k + j]) : (uint16_t)0;
  return as_bf16x8(r);
}
__device__ __forceinline__ bf16x8 ufrag8_tail(const uint16_t* row, int k, int K) {
  u16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (k + j < K) ? row[k + j] : (uint16_t)0;
  return as_bf16x8(r);
}
__device__ __forceinline__ bf16x8 ufrag8(const float* row, int k, int K, bool vec) {
  if (row == nullptr || k >= K) return as_bf16x8(u16x8{0, 0, 0, 0, 0, 0, 0, 0});
  return vec ? load_bf16x8_from_f32(row + k) : ufrag8_tail(row, k, K);
}
__device__ __forceinline__ bf16x8 ufrag8(const uint16_t* row, int k, int K, bool vec) {
  if (row == nullptr || k >= K) return as_bf16x8(u16x8{0, 0, 0, 0, 0, 0, 0, 0});
  return vec ? load_bf16x8(row + k) : ufrag8_tail(row, k, K);
}
template <typename T>
__device__ __forceinline__ float ufrag1(const T* row, int k, int K) {
  return (row != nullptr && k < K) ? ldw(row, k) : 0.f;
}

// The recurrent product of a forward step, h_{t-1} @ W_hh^T for the work-group's
// UFB utterances x 16 gate columns, left in LDS as the four waves' partial sums
// over their quarters of K = H.  Called by all 256 threads; ends with the
// work-group's barrier.
//   a0, a1: h_{t-1} [H] f32 of utterances b0 + (lane & 15) and b0 + 16 + (lane
//           & 15), nullptr past B;
//   br:     W_hh row g * H + u of gate column n = lane & 15 (g = n >> 2, u = u0
//           + (n & 3)), nullptr past H;
//   no_h:   the step has no recurrent operand (h_{-1} = 0): the product is
//           skipped, its sums are the zeros a product of zeros gives.
// It is a function of its own, not one with uni_gate_pre below, so that a
// kernel can start its own loads (lens, the cell state) between the two: after
// the barrier and together with gx's, as both kernels always have.  Behind the
// pre-activations they are a second round trip to memory in a kernel that is
// nothing but latency: 2 to 3 % of a step, measured.
template <bool BF16, typename TW>
__device__ __forceinline__ void uni_gate_partials(const float* a0, const float* a1, const TW* br,
                                                  bool no_h, int H, float (*part)[UFB][16]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool vec = (H & 7) == 0;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if (!no_h) {
    if constexpr (BF16) {
      for (int k0 = wave * 32; k0 < H; k0 += 4 * 32) {
        const int k = k0 + 8 * (lane >> 4);
        const bf16x8 b = ufrag8(br, k, H, vec);
        acc0 = mfma_bf16(ufrag8(a0, k, H, vec), b, acc0);
        acc1 = mfma_bf16(ufrag8(a1, k, H, vec), b, acc1);
      }
    } else {
      for (int k0 = wave * 4; k0 < H; k0 += 4 * 4) {
        const int k = k0 + (lane >> 4);
        const float b = ufrag1(br, k, H);
        acc0 = mfma_f32(ufrag1(a0, k, H), b, acc0);
        acc1 = mfma_f32(ufrag1(a1, k, H), b, acc1);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    part[wave][4 * (lane >> 4) + r][lane & 15] = acc0[r];
    part[wave][16 + 4 * (lane >> 4) + r][lane & 15] = acc1[r];
  }
  __syncthreads();
}

// The gate pre-activations of thread tid < UFB * UFU, which owns utterance row
// tid >> 2 and unit tid & 3 of the tile, from uni_gate_partials' sums and
// gx = &gx[b][t][j] of its (b, j):
//   pre[q] = ((p0 + p1) + (p2 + p3)) + gx[q * H], gate q of i, f, g, o.
__device__ __forceinline__ void uni_gate_pre(const float (*part)[UFB][16], const float* gx, int H,
                                             float pre[4]) {
  const int row = threadIdx.x >> 2, uu = threadIdx.x & 3;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    pre[q] = ((part[0][row][q * 4 + uu] + part[1][row][q * 4 + uu]) +
              (part[2][row][q * 4 + uu] + part[3][row][q * 4 + uu])) +
             gx[(long long)q * H];
}

// f32 weights -> bf16, once per call: the step launches stream 2 bytes per weight
__global__ void __launch_bounds__(256) uni_to_bf16(const float* __restrict__ x,
                                                   uint16_t* __restrict__ o, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = f2bf(x[i]);
}

}  // namespace
}  // namespace asr
