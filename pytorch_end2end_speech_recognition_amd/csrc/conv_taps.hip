// Stride-1 convolution with kf x kt taps (kf, kt in {3, 5}) over the
// channels-last, zero-haloed layer layout [B][T+2][F+2][C] (one-pixel halo =
// the reference's Conv2d padding of 1, encoders/cnn.py:68-73): forward, input
// gradient and weight-gradient image.  Unlike the 3x3 kernels (conv.hip,
// gemm.hip's tap addressing) the output grid is (T + 3 - kt) x (F + 3 - kf), so
// input and output rows are addressed by their own pitches.
//
// One kernel serves the forward and the input gradient ("a correlation of a
// grid with a tap image, written to another grid"):
//   out(b, to, fo)[n] = bias[n] + sum_{dt < kt, df < kf, c}
//                       in_p(b, to + dt - off_t, fo + df - off_f)[c] * w[n][(dt kf + df) Cin + c]
// where in_p is the padded input grid and positions outside it read as zero.
//   forward:        in = x,  off = (0, 0),            out grid = To x Fo
//   input gradient: in = dz, off = (kt - 3, kf - 3),  out grid = T x F, w the
//                   mirrored, transposed image (asr_conv_taps_weight_pack mode 1)
//
// bf16 mode: a work-group owns 64 consecutive output pixels of one utterance
// and up to 128 output channels.  Per chunk of CK input channels it stages the
// input window those pixels touch (every tap) in LDS once, as a 2-D "virtual"
// tile [rows][Wv = out width + kf - 1][CK] whose out-of-grid positions are
// zero, and runs the tap loop over that resident tile: v_mfma_f32_16x16x32_bf16,
// A fragments = 16-B LDS reads at pixel + tap shift, B fragments = 16-B global
// reads of the weight image (each wave owns its own output-channel blocks, so
// no weight is fetched twice by a work-group).  f32 mode: one thread per output
// pixel and 8 output channels, exact f32 products and sums in k order.
#include "common.h"
#include "mfma.h"

namespace asr {
namespace {

constexpr int TP_BM = 64;          // output pixels per work-group
constexpr int TP_BN = 128;         // output channels per work-group (2 blocks of 16 per wave)
constexpr int TP_LDS_MAX = 64 * 1024;

struct TapsArgs {
  const void* in;     // [B][Tip][Fip][Cin]
  const void* w;      // [Cout][kt kf Cin]
  const float* bias;  // [Cout] or null
  float* out;         // [B][To + 2][Fo + 2][Cout], interior written
  int B, Tip, Fip, Cin, Cout, To, Fo, kt, kf, off_t, off_f;
  int tiles_per_b, Wv;
};

template <int CK>
__global__ void __launch_bounds__(256) taps_bf16(TapsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int PITCH = CK + 8;   // bf16 per LDS pixel (80 / 48 B: 16-B aligned, off the 64-B stride)
  constexpr int PIECES = CK / 8;
  uint16_t* tile = reinterpret_cast<uint16_t*>(smem);
  const uint16_t* in = static_cast<const uint16_t*>(a.in);
  const uint16_t* wg = static_cast<const uint16_t*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x / a.tiles_per_b, tl = blockIdx.x - b * a.tiles_per_b;
  const int npix = a.To * a.Fo;
  const int m0 = tl * TP_BM, m1 = min(m0 + TP_BM, npix);
  const int to_min = m0 / a.Fo, to_max = (m1 - 1) / a.Fo;
  const int nrows = to_max - to_min + a.kt;
  const int Wv = a.Wv, ntap = a.kt * a.kf;
  const long long K = (long long)ntap * a.Cin;
  const int kg = lane >> 4, l16 = lane & 15;
  // LDS pixel of this lane's row in each of the four 16-row blocks (rows past
  // the tile's end are clamped: they compute a value nobody stores)
  int lp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = min(m0 + 16 * i + l16, m1 - 1);
    const int to = m / a.Fo;
    lp[i] = (to - to_min) * Wv + (m - to * a.Fo);
  }
  int nb[2];
  bool nok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    nb[j] = blockIdx.y * (TP_BN / 16) + w + 4 * j;
    nok[j] = nb[j] * 16 < a.Cout;   // wave-uniform
  }
  const bool klive = CK == 32 || kg < 2;   // CK = 16: the upper half of the MFMA's K is zero
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int c0 = 0; c0 < a.Cin; c0 += CK) {
    __syncthreads();   // the previous chunk's fragment reads are done
    const int items = nrows * Wv * PIECES;
    for (int it = tid; it < items; it += 256) {
      const int piece = it % PIECES, pv = it / PIECES;
      const int r = pv / Wv, v = pv - r * Wv;
      const int tr = to_min + r - a.off_t, fc = v - a.off_f;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (tr >= 0 && tr < a.Tip && fc >= 0 && fc < a.Fip)
        val = *reinterpret_cast<const uint4*>(
            in + (((long long)b * a.Tip + tr) * a.Fip + fc) * a.Cin + c0 + piece * 8);
      *reinterpret_cast<uint4*>(tile + (size_t)pv * PITCH + piece * 8) = val;
    }
    __syncthreads();
    if (!nok[0]) continue;   // this wave has no output channels (Cout < 64 ...); it staged only
    for (int tap = 0; tap < ntap; ++tap) {
      const int dt = tap / a.kf, df = tap - dt * a.kf;
      const int sh = dt * Wv + df;
      bf16x8 fb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        u16x8 v = zero8;
        if (nok[j] && klive)
          v = *reinterpret_cast<const u16x8*>(wg + (long long)(nb[j] * 16 + l16) * K +
                                              (long long)tap * a.Cin + c0 + kg * 8);
        fb[j] = as_bf16x8(v);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u16x8 v = zero8;
        if (klive)
          v = *reinterpret_cast<const u16x8*>(tile + (size_t)(lp[i] + sh) * PITCH + kg * 8);
        const bf16x8 fa = as_bf16x8(v);
        acc[i][0] = mfma_bf16(fa, fb[0], acc[i][0]);
        if (nok[1]) acc[i][1] = mfma_bf16(fa, fb[1], acc[i][1]);
      }
    }
  }
  // C fragment: column n = l16, rows 4 kg + r of the 16-row block
  const int Top = a.To + 2, Fop = a.Fo + 2;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!nok[j]) continue;
    const int n = nb[j] * 16 + l16;
    const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + 4 * kg + r;
        if (m >= m1) continue;
        const int to = m / a.Fo, fo = m - to * a.Fo;
        a.out[(((long long)b * Top + to + 1) * Fop + fo + 1) * a.Cout + n] = acc[i][j][r] + bv;
      }
  }
}

// f32 mode: thread = output pixel, blockIdx.y = group of 8 output channels
// (weights wave-uniform, so they are scalar loads).
__global__ void __launch_bounds__(256) taps_f32(TapsArgs a) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  const int npix = a.To * a.Fo;
  if (m >= (long long)a.B * npix) return;
  const int b = (int)(m / npix), q = (int)(m - (long long)b * npix);
  const int to = q / a.Fo, fo = q - to * a.Fo;
  const int n0 = blockIdx.y * 8;
  const float* in = static_cast<const float*>(a.in);
  const float* wg = static_cast<const float*>(a.w);
  const long long K = (long long)a.kt * a.kf * a.Cin;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int dt = 0; dt < a.kt; ++dt) {
    const int tr = to + dt - a.off_t;
    if (tr < 0 || tr >= a.Tip) continue;
    for (int df = 0; df < a.kf; ++df) {
      const int fc = fo + df - a.off_f;
      if (fc < 0 || fc >= a.Fip) continue;
      const float* x = in + (((long long)b * a.Tip + tr) * a.Fip + fc) * a.Cin;
      const float* wp = wg + (long long)n0 * K + (long long)(dt * a.kf + df) * a.Cin;
      for (int c = 0; c < a.Cin; ++c) {
        const float xv = x[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(xv, wp[j * K + c], acc[j]);
      }
    }
  }
  float* o = a.out + (((long long)b * (a.To + 2) + to + 1) * (a.Fo + 2) + fo + 1) * a.Cout + n0;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = acc[j] + (a.bias ? a.bias[n0 + j] : 0.f);
}

bool taps_ok(int k) { return k == 3 || k == 5; }

// rows of the virtual tile a 64-pixel strip of a To x Fo grid can touch
int tile_rows(int To, int Fo, int kt) {
  int span = (TP_BM - 2 + Fo) / Fo + 1;
  if (span > To) span = To;
  return span + kt - 1;
}

// channel chunk of the bf16 kernel for this shape (0: none fits)
int pick_ck(int To, int Fo, int Cin, int kt, int kf) {
  const long long px = (long long)tile_rows(To, Fo, kt) * (Fo + kf - 1);
  if (Cin % 32 == 0 && px * (32 + 8) * 2 <= TP_LDS_MAX) return 32;
  if (px * (16 + 8) * 2 <= TP_LDS_MAX) return 16;
  return 0;
}

// shape check shared by the forward and the input gradient; (To, Fo) = the grid written
int check_shape(const char* who, int cd, int B, int Ti, int Fi, int Cin, int Cout, int To, int Fo,
                int kf, int kt) {
  ASR_REQUIRE(cd == ASR_DT_F32 || cd == ASR_DT_BF16, ASR_ERR_ARG, "%s: bad compute dtype %d", who,
              cd);
  ASR_REQUIRE(B > 0 && Ti > 0 && Fi > 0 && Cin > 0 && Cout > 0, ASR_ERR_ARG, "%s: bad size", who);
  ASR_REQUIRE(taps_ok(kf) && taps_ok(kt), ASR_ERR_UNSUPPORTED,
              "%s: kernel %d x %d (extents 3 and 5 only)", who, kf, kt);
  ASR_REQUIRE(To >= 1 && Fo >= 1, ASR_ERR_UNSUPPORTED,
              "%s: grid %d x %d is smaller than the %d x %d (time x freq) kernel allows", who, Ti,
              Fi, kt, kf);
  ASR_REQUIRE((long long)B * (Ti + 2) * (Fi + 2) < (1ll << 31) &&
                  (long long)B * (To + 2) * (Fo + 2) < (1ll << 31),
              ASR_ERR_UNSUPPORTED, "%s: more than 2^31 pixels", who);
  if (cd == ASR_DT_BF16) {
    ASR_REQUIRE(Cin % 16 == 0 && Cout % 16 == 0 && Cin <= 256 && Cout <= 256, ASR_ERR_UNSUPPORTED,
                "%s: bf16 mode takes channel counts that are multiples of 16 up to 256 (%d -> %d)",
                who, Cin, Cout);
    ASR_REQUIRE(pick_ck(To, Fo, Cin, kt, kf) != 0, ASR_ERR_UNSUPPORTED,
                "%s: the input window of a %d-pixel strip (width %d) exceeds %d B of LDS", who,
                TP_BM, Fo + kf - 1, TP_LDS_MAX);
  } else {
    ASR_REQUIRE(Cout % 8 == 0, ASR_ERR_UNSUPPORTED, "%s: f32 mode takes Cout %% 8 == 0 (%d)", who,
                Cout);
  }
  return ASR_OK;
}

int launch_taps(int cd, const TapsArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (cd == ASR_DT_F32) {
    dim3 grid(ceil_div((long long)a.B * a.To * a.Fo, 256), a.Cout / 8);
    taps_f32<<<grid, 256, 0, st>>>(a);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
  }
  const int ck = pick_ck(a.To, a.Fo, a.Cin, a.kt, a.kf);
  const size_t lds = (size_t)tile_rows(a.To, a.Fo, a.kt) * a.Wv * (ck + 8) * 2;
  dim3 grid(a.B * a.tiles_per_b, ceil_div(a.Cout, TP_BN));
  if (ck == 32)
    taps_bf16<32><<<grid, 256, lds, st>>>(a);
  else
    taps_bf16<16><<<grid, 256, lds, st>>>(a);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// Weight-gradient image: packed[n][(dt kf + df) Cin + c] =
//   sum over (b, to, fo) of dz(b, to, fo)[n] * x_p(b, to + dt, fo + df)[c].
// The reduction runs over pixels, which are the slow index of both operands,
// so both are transposed into LDS one output row (b, to) at a time:
//   dzT [32 n][FoP]           (FoP = Fo rounded up to 32, zero past Fo)
//   xT  [KT rows][CW c][WvP]  (the KT input rows under that output row)
// Wave w owns 16 input channels for every tap and both 16-row blocks of the
// work-group's 32 output channels: per 32-pixel k step and input row dt it
// reads a window of 8 + KF - 1 pixels of its channel once and forms the KF
// shifted B fragments from it.  Grid = S row chunks x Cout / 32 x channel
// groups; each chunk writes its own slab, summed in chunk order afterwards
// (bitwise reproducible).
// ---------------------------------------------------------------------------
struct TapsWArgs {
  const uint16_t* x;    // [B][T+2][F+2][Cin]
  const uint16_t* dz;   // [B][To+2][Fo+2][Cout]
  float* slab;          // [S][Cout][ntap Cin]
  int B, Tip, Fip, Cin, Cout, To, Fo, S, FoP, WvP, CW;
};

template <int KF, int KT>
__global__ void __launch_bounds__(256) taps_wgrad_bf16(TapsWArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NTAP = KF * KT, WIN = 8 + KF - 1;
  uint16_t* dzT = reinterpret_cast<uint16_t*>(smem);
  uint16_t* xT = dzT + 32 * a.FoP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kg = lane >> 4, l16 = lane & 15;
  const int n0 = blockIdx.y * 32, c0 = blockIdx.z * a.CW;
  const int R = a.B * a.To;
  const int rbeg = (int)((long long)R * blockIdx.x / a.S);
  const int rend = (int)((long long)R * (blockIdx.x + 1) / a.S);
  const int Top = a.To + 2, Fop = a.Fo + 2;
  const bool live = w * 16 < a.CW && c0 + w * 16 < a.Cin;   // wave-uniform
  f32x4 acc[2][NTAP];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < NTAP; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int row = rbeg; row < rend; ++row) {
    const int b = row / a.To, to = row - b * a.To;
    __syncthreads();
    // dz row -> dzT (8 channels per item)
    for (int it = tid; it < a.FoP * 4; it += 256) {
      const int piece = it & 3, fo = it >> 2;
      const int n = n0 + piece * 8;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (fo < a.Fo && n < a.Cout)
        v = *reinterpret_cast<const u16x8*>(
            a.dz + (((long long)b * Top + to + 1) * Fop + fo + 1) * a.Cout + n);
#pragma unroll
      for (int e = 0; e < 8; ++e) dzT[(piece * 8 + e) * a.FoP + fo] = v[e];
    }
    // the KT input rows -> xT
    const int cpieces = a.CW / 8;
    for (int it = tid; it < KT * a.WvP * cpieces; it += 256) {
      const int piece = it % cpieces, rv = it / cpieces;
      const int r = rv / a.WvP, v = rv - r * a.WvP;
      const int c = c0 + piece * 8;
      u16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
      if (v < a.Fip && c < a.Cin)
        val = *reinterpret_cast<const u16x8*>(
            a.x + (((long long)b * a.Tip + to + r) * a.Fip + v) * a.Cin + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) xT[((size_t)r * a.CW + piece * 8 + e) * a.WvP + v] = val[e];
    }
    __syncthreads();
    if (!live) continue;
    for (int k0 = 0; k0 < a.FoP; k0 += 32) {
      bf16x8 fa[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fa[j] = as_bf16x8(*reinterpret_cast<const u16x8*>(dzT + (16 * j + l16) * a.FoP + k0 +
                                                          kg * 8));
#pragma unroll
      for (int dt = 0; dt < KT; ++dt) {
        const uint16_t* xr = xT + ((size_t)dt * a.CW + w * 16 + l16) * a.WvP + k0 + kg * 8;
        uint16_t win[WIN];
#pragma unroll
        for (int e = 0; e < WIN; ++e) win[e] = xr[e];
#pragma unroll
        for (int df = 0; df < KF; ++df) {
          u16x8 v;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = win[df + e];
          const bf16x8 fb = as_bf16x8(v);
          acc[0][dt * KF + df] = mfma_bf16(fa[0], fb, acc[0][dt * KF + df]);
          acc[1][dt * KF + df] = mfma_bf16(fa[1], fb, acc[1][dt * KF + df]);
        }
      }
    }
  }
  if (!live) return;
  // C fragment: rows (output channels) 4 kg + r, column (input channel) l16
  const long long K = (long long)NTAP * a.Cin;
  float* o = a.slab + (long long)blockIdx.x * a.Cout * K;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 16 * j + 4 * kg + r;
        if (n < a.Cout) o[n * K + (long long)t * a.Cin + c0 + w * 16 + l16] = acc[j][t][r];
      }
}

// packed[i] = sum over chunks s of slab[s][i], in chunk order
__global__ void __launch_bounds__(256) taps_wgrad_reduce(const float* __restrict__ slab, int S,
                                                         long long n, float* __restrict__ packed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += slab[(long long)k * n + i];
  packed[i] = s;
}

// f32 mode: thread = one element (n, tap, c) of the image, pixels summed in order
__global__ void __launch_bounds__(256) taps_wgrad_f32(const float* __restrict__ x,
                                                      const float* __restrict__ dz, int B, int Tip,
                                                      int Fip, int Cin, int Cout, int To, int Fo,
                                                      int kf, int kt, float* __restrict__ packed) {
  const long long K = (long long)kf * kt * Cin;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * Cout) return;
  const int n = (int)(i / K), k = (int)(i - n * K);
  const int tap = k / Cin, c = k - tap * Cin;
  const int dt = tap / kf, df = tap - dt * kf;
  float s = 0.f;
  for (int b = 0; b < B; ++b)
    for (int to = 0; to < To; ++to) {
      const float* xr = x + (((long long)b * Tip + to + dt) * Fip + df) * Cin + c;
      const float* zr = dz + (((long long)b * (To + 2) + to + 1) * (Fo + 2) + 1) * Cout + n;
      for (int fo = 0; fo < Fo; ++fo) s = fmaf(zr[(long long)fo * Cout], xr[(long long)fo * Cin], s);
    }
  packed[i] = s;
}

struct WPlan {
  int S, FoP, WvP, CW;
  size_t lds, ws;
};

bool wgrad_plan(int B, int T, int F, int Cin, int Cout, int kf, int kt, WPlan* p) {
  const int To = T + 3 - kt, Fo = F + 3 - kf;
  if (To < 1 || Fo < 1) return false;
  p->FoP = (Fo + 31) / 32 * 32;
  int wv = p->FoP + kf - 1 + 8;   // every window read (k0 + 8 kg + WIN) stays inside the row
  if (wv < F + 2) wv = F + 2;
  wv = (wv + 1) / 2 * 2;
  if ((wv / 2) % 2 == 0) wv += 2;   // an odd number of dwords per channel row: the 16 lanes of a
                                    // fragment read spread over the banks
  p->WvP = wv;
  p->CW = Cin < 64 ? Cin : 64;
  p->lds = (size_t)32 * p->FoP * 2 + (size_t)kt * p->CW * p->WvP * 2;
  const int R = B * To;
  p->S = R < 16 ? R : 16;
  p->ws = (size_t)p->S * Cout * kf * kt * Cin * sizeof(float);
  return p->lds <= 160 * 1024 - 1024;
}

template <int KF, int KT>
int launch_wgrad(const TapsWArgs& a, const WPlan& p, void* stream) {
  auto k = taps_wgrad_bf16<KF, KT>;
  if (p.lds > 64 * 1024)
    ASR_CHECK_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)p.lds));
  dim3 grid(p.S, ceil_div(a.Cout, 32), ceil_div(a.Cin, p.CW));
  k<<<grid, 256, p.lds, (hipStream_t)stream>>>(a);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

// Conv2d weight [Co][Ci][kf][kt] <-> tap images
__global__ void __launch_bounds__(256) taps_pack(const float* __restrict__ w, int Co, int Ci,
                                                 int Cip, int kf, int kt, int mode, int bf,
                                                 void* __restrict__ out) {
  const int ntap = kf * kt;
  const long long n = mode == 0 ? (long long)Co * ntap * Cip : (long long)Ci * ntap * Co;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
  if (mode == 0) {   // out[co][tap Cip + ci]
    const int ci = (int)(i % Cip), tap = (int)(i / Cip % ntap), co = (int)(i / Cip / ntap);
    const int dt = tap / kf, df = tap - dt * kf;
    if (ci < Ci) v = w[(((long long)co * Ci + ci) * kf + df) * kt + dt];
  } else {           // out[ci][tap' Co + co], tap' the mirrored tap
    const int co = (int)(i % Co), tap = (int)(i / Co % ntap), ci = (int)(i / Co / ntap);
    const int dt = tap / kf, df = tap - dt * kf;
    v = w[(((long long)co * Ci + ci) * kf + (kf - 1 - df)) * kt + (kt - 1 - dt)];
  }
  if (bf)
    static_cast<uint16_t*>(out)[i] = f2bf(v);
  else
    static_cast<float*>(out)[i] = v;
}

__global__ void __launch_bounds__(256) taps_unpack_acc(const float* __restrict__ packed, int Co,
                                                       int Ci, int Cip, int kf, int kt,
                                                       float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Co * Ci * kf * kt) return;
  const int dt = (int)(i % kt), df = (int)(i / kt % kf), ci = (int)(i / kt / kf % Ci);
  const int co = (int)(i / kt / kf / Ci);
  dw[i] += packed[(long long)co * kf * kt * Cip + (long long)(dt * kf + df) * Cip + ci];
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_conv_taps_supported(int compute_dtype, int B, int T, int F, int Cin, int Cout,
                                       int kf, int kt) {
  const int To = T + 3 - kt, Fo = F + 3 - kf;
  if (check_shape("conv_taps", compute_dtype, B, T, F, Cin, Cout, To, Fo, kf, kt) != ASR_OK)
    return 0;
  // the input gradient: the same kernel over the dz grid, writing T x F
  if (check_shape("conv_taps", compute_dtype, B, To, Fo, Cout, Cin, T, F, kf, kt) != ASR_OK)
    return 0;
  if (compute_dtype == ASR_DT_BF16) {
    WPlan p;
    if (!wgrad_plan(B, T, F, Cin, Cout, kf, kt, &p)) {
      set_error("conv_taps: the weight gradient's row tiles (F = %d, kt = %d) exceed the LDS", F,
                kt);
      return 0;
    }
  }
  return 1;
}

extern "C" int asr_conv_taps_forward(int compute_dtype, const void* in, int B, int T, int F,
                                     int Cin, const void* w, int Cout, int kf, int kt,
                                     const float* bias, float* out, void* stream) {
  ASR_REQUIRE(in && w && out, ASR_ERR_ARG, "conv_taps_forward: null pointer");
  const int To = T + 3 - kt, Fo = F + 3 - kf;
  const int rc = check_shape("conv_taps_forward", compute_dtype, B, T, F, Cin, Cout, To, Fo, kf,
                             kt);
  if (rc != ASR_OK) return rc;
  TapsArgs a;
  a.in = in; a.w = w; a.bias = bias; a.out = out;
  a.B = B; a.Tip = T + 2; a.Fip = F + 2; a.Cin = Cin; a.Cout = Cout; a.To = To; a.Fo = Fo;
  a.kt = kt; a.kf = kf; a.off_t = 0; a.off_f = 0;
  a.tiles_per_b = ceil_div((long long)To * Fo, TP_BM);
  a.Wv = Fo + kf - 1;
  return launch_taps(compute_dtype, a, stream);
}

extern "C" int asr_conv_taps_dgrad(int compute_dtype, const void* dz, int B, int T, int F, int Cin,
                                   const void* wt, int Cout, int kf, int kt, float* dx,
                                   void* stream) {
  ASR_REQUIRE(dz && wt && dx, ASR_ERR_ARG, "conv_taps_dgrad: null pointer");
  const int To = T + 3 - kt, Fo = F + 3 - kf;
  ASR_REQUIRE(To >= 1 && Fo >= 1, ASR_ERR_UNSUPPORTED,
              "conv_taps_dgrad: grid %d x %d is smaller than the %d x %d (time x freq) kernel allows",
              T, F, kt, kf);
  const int rc = check_shape("conv_taps_dgrad", compute_dtype, B, To, Fo, Cout, Cin, T, F, kf, kt);
  if (rc != ASR_OK) return rc;
  TapsArgs a;
  a.in = dz; a.w = wt; a.bias = nullptr; a.out = dx;
  a.B = B; a.Tip = To + 2; a.Fip = Fo + 2; a.Cin = Cout; a.Cout = Cin; a.To = T; a.Fo = F;
  a.kt = kt; a.kf = kf; a.off_t = kt - 3; a.off_f = kf - 3;
  a.tiles_per_b = ceil_div((long long)T * F, TP_BM);
  a.Wv = F + kf - 1;
  return launch_taps(compute_dtype, a, stream);
}

extern "C" size_t asr_conv_taps_wgrad_workspace_bytes(int compute_dtype, int B, int T, int F,
                                                      int Cin, int Cout, int kf, int kt) {
  if (!taps_ok(kf) || !taps_ok(kt) || B < 1 || T + 3 - kt < 1 || F + 3 - kf < 1) return 0;
  if (compute_dtype == ASR_DT_F32) return 16;
  WPlan p;
  if (compute_dtype != ASR_DT_BF16 || Cin % 16 || Cout % 16 || Cin > 256 || Cout > 256 ||
      Cin < 16 || Cout < 16 || !wgrad_plan(B, T, F, Cin, Cout, kf, kt, &p))
    return 0;
  return p.ws;
}

extern "C" int asr_conv_taps_wgrad(int compute_dtype, const void* x, const void* dz, int B, int T,
                                   int F, int Cin, int Cout, int kf, int kt, float* packed,
                                   void* ws, size_t ws_bytes, void* stream) {
  ASR_REQUIRE(x && dz && packed, ASR_ERR_ARG, "conv_taps_wgrad: null pointer");
  const size_t need =
      asr_conv_taps_wgrad_workspace_bytes(compute_dtype, B, T, F, Cin, Cout, kf, kt);
  ASR_REQUIRE(need != 0, ASR_ERR_UNSUPPORTED,
              "conv_taps_wgrad: shape not supported (kernel %d x %d, grid %d x %d, %d -> %d channels)",
              kf, kt, T, F, Cin, Cout);
  const int To = T + 3 - kt, Fo = F + 3 - kf;
  ASR_REQUIRE((long long)B * (T + 2) * (F + 2) < (1ll << 31), ASR_ERR_UNSUPPORTED,
              "conv_taps_wgrad: more than 2^31 pixels");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)Cout * kf * kt * Cin;
  if (compute_dtype == ASR_DT_F32) {
    taps_wgrad_f32<<<ceil_div(n, 256), 256, 0, st>>>((const float*)x, (const float*)dz, B, T + 2,
                                                     F + 2, Cin, Cout, To, Fo, kf, kt, packed);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
  }
  ASR_REQUIRE(ws && ws_bytes >= need, ASR_ERR_WORKSPACE,
              "conv_taps_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
  WPlan p;
  wgrad_plan(B, T, F, Cin, Cout, kf, kt, &p);
  TapsWArgs a;
  a.x = (const uint16_t*)x; a.dz = (const uint16_t*)dz; a.slab = (float*)ws;
  a.B = B; a.Tip = T + 2; a.Fip = F + 2; a.Cin = Cin; a.Cout = Cout; a.To = To; a.Fo = Fo;
  a.S = p.S; a.FoP = p.FoP; a.WvP = p.WvP; a.CW = p.CW;
  int rc;
  if (kf == 3 && kt == 3) rc = launch_wgrad<3, 3>(a, p, stream);
  else if (kf == 3 && kt == 5) rc = launch_wgrad<3, 5>(a, p, stream);
  else if (kf == 5 && kt == 3) rc = launch_wgrad<5, 3>(a, p, stream);
  else rc = launch_wgrad<5, 5>(a, p, stream);
  if (rc != ASR_OK) return rc;
  taps_wgrad_reduce<<<ceil_div(n, 256), 256, 0, st>>>((const float*)ws, p.S, n, packed);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_conv_taps_weight_pack(const float* w, int Co, int Ci, int Cip, int kf, int kt,
                                         int mode, int out_dtype, void* out, void* stream) {
  ASR_REQUIRE(w && out, ASR_ERR_ARG, "conv_taps_weight_pack: null pointer");
  ASR_REQUIRE(taps_ok(kf) && taps_ok(kt) && Co > 0 && Ci > 0 && Cip >= Ci &&
                  (mode == 0 || (mode == 1 && Cip == Ci)),
              ASR_ERR_ARG, "conv_taps_weight_pack: bad argument");
  const long long n = (long long)Co * kf * kt * Cip;
  taps_pack<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(w, Co, Ci, Cip, kf, kt, mode,
                                                                out_dtype == ASR_DT_BF16, out);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_conv_taps_weight_unpack_acc(const float* packed, int Co, int Ci, int Cip, int kf,
                                               int kt, float* dw, void* stream) {
  ASR_REQUIRE(packed && dw, ASR_ERR_ARG, "conv_taps_weight_unpack_acc: null pointer");
  ASR_REQUIRE(taps_ok(kf) && taps_ok(kt) && Co > 0 && Ci > 0 && Cip >= Ci, ASR_ERR_ARG,
              "conv_taps_weight_unpack_acc: bad argument");
  const long long n = (long long)Co * Ci * kf * kt;
  taps_unpack_acc<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(packed, Co, Ci, Cip, kf, kt,
                                                                      dw);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
