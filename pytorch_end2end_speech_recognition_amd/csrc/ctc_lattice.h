// Pieces of the blank-interleaved CTC lattice shared by the forward-backward
// (ctc.hip) and the forced alignment (ctc_align.hip): the states-per-lane
// choice, the LDS-only barrier, the online log-sum-exp accumulator, the
// K-wide register <-> memory moves and the DPP wave shifts.
#pragma once
#include "common.h"

namespace asr {
namespace {

constexpr int kMaxK = 16;  // up to 64*16 = 1024 lattice states (labels <= 511)

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

inline int pick_k(int max_label_len) {
  int S = 2 * max_label_len + 1;
  int k = 1;
  while (64 * k < S) k <<= 1;
  return k;
}

// A work-group barrier that orders LDS only, for the lattices' per-chunk
// barriers: __syncthreads also drains vmcnt, i.e. waits for the lattice rows'
// global stores and the loader's prefetch loads issued just before it -- one
// memory round trip per chunk on the sequential chain.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Online log-sum-exp accumulator (running max m, sum s of exp(x - m)).
// While m is still -inf the values seen so far are -inf (masked classes) or
// NaN: they add 0, or a NaN to keep -- exp(-inf - -inf) would turn a run of
// masked classes into a NaN log-sum-exp.  lse_none(t): that term, from the
// plain sum t of the values (-inf, or NaN).
__device__ __forceinline__ float lse_none(float t) { return t == neg_inf() ? 0.f : t; }
__device__ __forceinline__ void lse_acc4(float& m, float& s, float4 v) {
  const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  if (mx > m) { s *= __expf(m - mx); m = mx; }
  if (m == neg_inf()) { s += lse_none((v.x + v.y) + (v.z + v.w)); return; }
  s += __expf(v.x - m) + __expf(v.y - m) + __expf(v.z - m) + __expf(v.w - m);
}
__device__ __forceinline__ void lse_acc1(float& m, float& s, float x) {
  if (x > m) { s *= __expf(m - x); m = x; }
  if (m == neg_inf()) { s += lse_none(x); return; }
  s += __expf(x - m);
}

// Elements of a row before its first 16-B boundary.
__device__ __forceinline__ int head_elems(const float* p) {
  return (int)((4 - (((size_t)p >> 2) & 3)) & 3);
}

template <int K>
__device__ __forceinline__ void load_k(float (&r)[K], const float* p) {
  if constexpr (K % 4 == 0) {
#pragma unroll
    for (int k = 0; k < K; k += 4) {
      float4 v = *reinterpret_cast<const float4*>(p + k);
      r[k] = v.x; r[k + 1] = v.y; r[k + 2] = v.z; r[k + 3] = v.w;
    }
  } else if constexpr (K == 2) {
    float2 v = *reinterpret_cast<const float2*>(p);
    r[0] = v.x; r[1] = v.y;
  } else {
    r[0] = p[0];
  }
}

template <int K>
__device__ __forceinline__ void store_k(float* p, const float (&r)[K]) {
  if constexpr (K % 4 == 0) {
#pragma unroll
    for (int k = 0; k < K; k += 4)
      *reinterpret_cast<float4*>(p + k) = make_float4(r[k], r[k + 1], r[k + 2], r[k + 3]);
  } else if constexpr (K == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
  } else {
    p[0] = r[0];
  }
}

// DPP wave shifts (GFX9 wave_shr:1 / wave_shl:1): lane i receives lane i-1 /
// i+1; the lane without a source receives 0 (callers overwrite it).
__device__ __forceinline__ float from_lower_lane(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper_lane(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130, 0xf, 0xf, false));
}

}  // namespace
}  // namespace asr
