// Batched edit distance with substitution / insertion / deletion counts on
// gfx950: scores the decoders' device hypotheses against the transcripts
// (replaces the reference's per-utterance Python table,
// utils/evaluation/edit_distance.py:53-126, and the token-level part of the
// recipes' text clean-up, examples/*/exp/metrics/{phone,character,word}.py).
//
// One work-group of one wave per utterance pair, integers only.
//
// clean-up (both sequences, 64 raw tokens per round, into LDS):
//   1. hypothesis only: cut before the first eos; entries at or past the
//      length and negative entries are not part of the sequence;
//   2. map[token] (a mapped value < 0 deletes the token);
//   3. space >= 0: a separator survives iff the last surviving token before it
//      is not a separator (runs collapse, a leading one goes); a trailing one
//      is dropped at the end.
//   Survivors are compacted with a ballot + popcount scan; the only state
//   carried from round to round is the count, "cut" and "last survivor was a
//   separator or nothing".
// units:
//   ASR_ED_TOKEN: the surviving tokens.
//   ASR_ED_WORD: maximal runs of non-separator tokens, interned to integers so
//   that the table compares integers in both modes: a reference word takes the
//   index of the first equal reference word, a hypothesis word that of the
//   first equal reference word or else a number no reference word has
//   (hypothesis words are only ever compared with reference words).  Equality
//   is length + 20-bit hash first, then CONFIRMED token by token.
// table (compute_wer): d[i][0] = i, d[0][j] = j, d[i][j] = d[i-1][j-1] on a
//   match else 1 + min(diagonal, left, up).  Strips of 64 reference positions,
//   one per lane; lane l is at hypothesis position s - l at step s, so a step
//   is one anti-diagonal of the strip.  "up" arrives from lane l - 1 by a
//   one-lane DPP shift, "diagonal" is last step's "up"; lane 0 reads both from
//   the previous strip's last row, kept in LDS (uint16: d <= 4095).
// backtrace: the move the reference's backtrace takes at (x, y) depends on
//   d[x][y] and its three neighbours only, so it is recorded while the table
//   is filled -- 0 correct, 1 insertion, 2 substitution, 3 deletion, in the
//   reference's order of preference -- 16 cells to a 32-bit word, each word
//   owned by one lane; the table itself is never stored.  The codes live in
//   LDS when ref x ceil(hyp / 16) <= 4096 words, in the caller's workspace
//   otherwise.  Lane 0 then walks from (ref, hyp) to (0, 0).  On the borders
//   the only moves are insertion (x == 0) and deletion (y == 0): the reference
//   has no border rule (its indices wrap and it raises), DESIGN.md.
#include "common.h"

namespace asr {
namespace {

constexpr int kMaxUnits = 4095;           // per sequence, raw tokens included
constexpr int kTok = 4096;
constexpr int kLdsCodeWords = 4096;

__device__ __forceinline__ int dpp_wave_shr1(int old, int v) {
  // lane l <- lane l - 1; lane 0 keeps `old`
  return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ unsigned hash_tok(unsigned h, int c) {
  h = (h ^ (unsigned)c) * 0x9E3779B1u;
  return h ^ (h >> 15);
}

struct EdArgs {
  const void* hyp;
  const int32_t* hyp_lens;
  const int32_t* ref;
  const int32_t* ref_lens;
  const int32_t* map;
  long long ld_hyp, ld_ref;
  int max_ref, max_hyp, unit, eos, space, map_len, hyp_i64;
  int32_t* out;
  unsigned long long* totals;
  uint32_t* ws_codes;             // nullptr: the codes fit LDS
  long long ws_codes_stride;      // words per utterance
};

// steps 1-3 of one sequence into dst[0, n); returns n (uniform)
__device__ int clean_sequence(const EdArgs& a, const void* src, bool i64, int len, int eos,
                              int32_t* dst) {
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n = 0;
  bool cut = false, last_sep = true;     // "nothing yet" strips like a separator
  for (int base = 0; base < len && !cut; base += 64) {
    const int p = base + lane;
    int t = -1;
    if (p < len) t = i64 ? (int)((const long long*)src)[p] : ((const int32_t*)src)[p];
    bool alive = t >= 0;
    if (eos >= 0) {
      const unsigned long long em = __ballot(alive && t == eos);
      if (em) {
        cut = true;
        alive = alive && (below & em) == 0ull && t != eos;
      }
    }
    if (alive && a.map && t < a.map_len) {
      t = a.map[t];
      alive = t >= 0;
    }
    bool keep = alive;
    const bool sep = alive && a.space >= 0 && t == a.space;
    const unsigned long long vm = __ballot(alive), sm = __ballot(sep);
    if (sep) {
      const unsigned long long before = vm & below;
      const bool prev_sep = before ? ((sm >> (63 - __clzll((long long)before))) & 1ull) != 0ull
                                   : last_sep;
      keep = !prev_sep;
    }
    if (vm) last_sep = ((sm >> (63 - __clzll((long long)vm))) & 1ull) != 0ull;
    const unsigned long long km = __ballot(keep);
    if (keep) dst[n + __popcll(km & below)] = t;
    n += __popcll(km);
  }
  __syncthreads();
  if (a.space >= 0 && n > 0 && dst[n - 1] == a.space) --n;
  return n;
}

// ASR_ED_WORD: the word table of dst[0, n) -- tab[k] = start | hash << 12 --
// returns the number of words (uniform).  After clean-up separators are
// single and inner, so word k ends one before word k + 1 starts.
__device__ int word_table(const int32_t* tok, int n, int space, uint32_t* tab) {
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int nw = 0;
  for (int base = 0; base < n; base += 64) {
    const int p = base + lane;
    const bool start = p < n && tok[p] != space && (p == 0 || tok[p - 1] == space);
    const unsigned long long m = __ballot(start);
    if (start) {
      unsigned h = 0x811C9DC5u;
      for (int q = p; q < n && tok[q] != space; ++q) h = hash_tok(h, tok[q]);
      tab[nw + __popcll(m & below)] = (unsigned)p | (h << 12);
    }
    nw += __popcll(m);
  }
  return nw;
}

__device__ __forceinline__ int word_end(const uint32_t* tab, int k, int nw, int n) {
  return k + 1 < nw ? (int)(tab[k + 1] & 0xfffu) - 1 : n;
}

__device__ __forceinline__ bool same_word(const int32_t* ta, unsigned ea, int la,
                                          const int32_t* tb, unsigned eb, int lb) {
  if ((ea >> 12) != (eb >> 12) || la != lb) return false;
  const int32_t* pa = ta + (ea & 0xfffu);
  const int32_t* pb = tb + (eb & 0xfffu);
  for (int q = 0; q < la; ++q)
    if (pa[q] != pb[q]) return false;
  return true;
}

__global__ void __launch_bounds__(64) edit_distance_kernel(EdArgs a) {
  __shared__ int32_t s_tok[2][kTok];          // cleaned tokens, then the units
  __shared__ uint32_t s_codes[kLdsCodeWords]; // word tables first, then the move codes
  __shared__ uint16_t s_row[kTok];            // ids first, then d[strip's row 0][j]
  __shared__ int s_dist;

  const int b = blockIdx.x, lane = threadIdx.x;
  const int rl = max(0, min(a.ref_lens[b], a.max_ref));
  const int hl = max(0, min(a.hyp_lens[b], a.max_hyp));
  const int32_t* ref = a.ref + (long long)b * a.ld_ref;
  const void* hyp = a.hyp_i64 ? (const void*)((const long long*)a.hyp + (long long)b * a.ld_hyp)
                              : (const void*)((const int32_t*)a.hyp + (long long)b * a.ld_hyp);
  int R = clean_sequence(a, ref, false, rl, -1, s_tok[0]);
  int H = clean_sequence(a, hyp, a.hyp_i64 != 0, hl, a.eos, s_tok[1]);

  if (a.unit == ASR_ED_WORD) {
    uint32_t* tab_r = s_codes;
    uint32_t* tab_h = s_codes + kTok / 2;       // a sequence of n tokens has <= (n + 1) / 2 words
    const int Rw = word_table(s_tok[0], R, a.space, tab_r);
    const int Hw = word_table(s_tok[1], H, a.space, tab_h);
    __syncthreads();
    for (int k = lane; k < Rw + Hw; k += 64) {
      const bool is_ref = k < Rw;
      const int kk = is_ref ? k : k - Rw;
      const uint32_t* tab = is_ref ? tab_r : tab_h;
      const int32_t* tk = is_ref ? s_tok[0] : s_tok[1];
      const unsigned e = tab[kk];
      const int len = word_end(tab, kk, is_ref ? Rw : Hw, is_ref ? R : H) - (int)(e & 0xfffu);
      int id = k;
      const int lim = is_ref ? kk : Rw;         // earlier reference words / all of them
      for (int j = 0; j < lim; ++j) {
        const unsigned ej = tab_r[j];
        if (same_word(tk, e, len, s_tok[0], ej, word_end(tab_r, j, Rw, R) - (int)(ej & 0xfffu))) {
          id = j;
          break;
        }
      }
      s_row[k] = (uint16_t)id;
    }
    __syncthreads();
    for (int k = lane; k < Rw; k += 64) s_tok[0][k] = s_row[k];
    for (int k = lane; k < Hw; k += 64) s_tok[1][k] = s_row[Rw + k];
    R = Rw;
    H = Hw;
    __syncthreads();
  }

  const int CW = (H + 15) >> 4;
  uint32_t* codes = a.ws_codes ? a.ws_codes + (long long)b * a.ws_codes_stride : s_codes;
  for (int j = lane; j <= H; j += 64) s_row[j] = (uint16_t)j;
  if (lane == 0) s_dist = H;
  __syncthreads();

  for (int i0 = 0; i0 < R; i0 += 64) {
    const int rows = min(64, R - i0);
    const bool more = i0 + 64 < R;              // the next strip reads this one's last row
    const int i = i0 + 1 + lane;
    const int ru = s_tok[0][min(i, R) - 1];
    int left = i, diag = i - 1;
    int hu_n = s_tok[1][max(0, min(-lane, kTok - 1))];
    int row_n = s_row[min(1, H)];
    uint32_t acc = 0;
    uint32_t* crow = codes + (long long)(i - 1) * CW;
    const int steps = H + rows - 1;
    for (int s = 0; s < steps; ++s) {
      const int j = s - lane + 1;
      const int hu = hu_n, rowv = row_n;
      hu_n = s_tok[1][max(0, min(s + 1 - lane, kTok - 1))];
      row_n = s_row[min(s + 2, H)];
      const int up = dpp_wave_shr1(rowv, left);
      if (lane < rows && j >= 1 && j <= H) {
        const bool match = ru == hu;
        const int m = min(min(diag, left), up) + 1;
        const int v = match ? diag : m;
        const unsigned code = match ? 0u : (v == left + 1 ? 1u : (v == diag + 1 ? 2u : 3u));
        acc |= code << (2 * ((j - 1) & 15));
        if (((j - 1) & 15) == 15 || j == H) {
          crow[(j - 1) >> 4] = acc;
          acc = 0;
        }
        if (more && lane == 63) s_row[j] = (uint16_t)v;
        left = v;
      }
      diag = up;
    }
    if (i == R) s_dist = left;
    if (lane == 0) s_row[0] = (uint16_t)(i0 + 64);
    __syncthreads();
  }
  __syncthreads();

  if (lane == 0) {
    int x = R, y = H, sub = 0, ins = 0, del = 0;
    while (x > 0 && y > 0) {
      const unsigned c = (codes[(long long)(x - 1) * CW + ((y - 1) >> 4)] >> (2 * ((y - 1) & 15))) & 3u;
      if (c == 0u) { --x; --y; }
      else if (c == 1u) { ++ins; --y; }
      else if (c == 2u) { ++sub; --x; --y; }
      else { ++del; --x; }
    }
    ins += y;                                   // x == 0: insertions only
    del += x;                                   // y == 0: deletions only
    const int v[5] = {s_dist, sub, ins, del, R};
    for (int k = 0; k < 5; ++k) {
      a.out[(long long)b * 5 + k] = v[k];
      if (a.totals) atomicAdd(a.totals + k, (unsigned long long)v[k]);
    }
  }
}

inline size_t code_words(int max_ref, int max_hyp) {
  return (size_t)max_ref * (size_t)((max_hyp + 15) / 16);
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_edit_distance_ws_bytes(int B, int max_ref, int max_hyp) {
  if (B <= 0 || max_ref < 0 || max_hyp < 0 || max_ref > kMaxUnits || max_hyp > kMaxUnits) return 0;
  const size_t w = code_words(max_ref, max_hyp);
  // never 0 for a shape the kernel takes: 0 means "refused"
  return w <= (size_t)kLdsCodeWords ? 16 : (size_t)B * w * sizeof(uint32_t);
}

extern "C" int asr_edit_distance(const void* hyp, long long ld_hyp, const int32_t* hyp_lens,
                                 const int32_t* ref, long long ld_ref, const int32_t* ref_lens,
                                 int B, int max_ref, int max_hyp, const asr_edit_opts_t* opts,
                                 int32_t* out, long long* totals, void* workspace, size_t ws_bytes,
                                 void* stream) {
  ASR_REQUIRE(hyp && hyp_lens && ref && ref_lens && opts && out, ASR_ERR_ARG,
              "edit_distance: null pointer");
  ASR_REQUIRE(B > 0 && max_ref >= 0 && max_hyp >= 0 && ld_hyp >= max_hyp && ld_ref >= max_ref,
              ASR_ERR_ARG, "edit_distance: bad shape (B %d, max_ref %d, max_hyp %d, ld %lld / %lld)",
              B, max_ref, max_hyp, ld_ref, ld_hyp);
  ASR_REQUIRE(opts->unit == ASR_ED_TOKEN || opts->unit == ASR_ED_WORD, ASR_ERR_ARG,
              "edit_distance: unit = %d", opts->unit);
  ASR_REQUIRE(opts->unit != ASR_ED_WORD || opts->space >= 0, ASR_ERR_ARG,
              "edit_distance: ASR_ED_WORD needs a separator token (space >= 0)");
  ASR_REQUIRE(!opts->map || opts->map_len > 0, ASR_ERR_ARG, "edit_distance: map_len = %d",
              opts->map_len);
  ASR_REQUIRE(max_ref <= kMaxUnits && max_hyp <= kMaxUnits, ASR_ERR_UNSUPPORTED,
              "edit_distance: max_ref = %d / max_hyp = %d: more than %d units per sequence "
              "cannot be excluded", max_ref, max_hyp, kMaxUnits);
  const long long two_gib = 1ll << 31;
  ASR_REQUIRE((long long)B * ld_hyp * (opts->hyp_i64 ? 8 : 4) < two_gib &&
                  (long long)B * ld_ref * 4 < two_gib,
              ASR_ERR_UNSUPPORTED, "edit_distance: an operand of 2 GiB or more");
  const size_t w = code_words(max_ref, max_hyp);
  const bool in_lds = w <= (size_t)kLdsCodeWords;
  if (!in_lds) {
    ASR_REQUIRE(workspace, ASR_ERR_ARG, "edit_distance: null workspace");
    ASR_REQUIRE(ws_bytes >= (size_t)B * w * sizeof(uint32_t), ASR_ERR_WORKSPACE,
                "edit_distance: workspace %zu < %zu bytes", ws_bytes,
                (size_t)B * w * sizeof(uint32_t));
    ASR_REQUIRE(((uintptr_t)workspace & 3) == 0, ASR_ERR_ARG,
                "edit_distance: workspace not 4-B aligned");
  }
  EdArgs a;
  a.hyp = hyp;
  a.hyp_lens = hyp_lens;
  a.ref = ref;
  a.ref_lens = ref_lens;
  a.map = opts->map;
  a.ld_hyp = ld_hyp;
  a.ld_ref = ld_ref;
  a.max_ref = max_ref;
  a.max_hyp = max_hyp;
  a.unit = opts->unit;
  a.eos = opts->eos;
  a.space = opts->space;
  a.map_len = opts->map ? opts->map_len : 0;
  a.hyp_i64 = opts->hyp_i64;
  a.out = out;
  a.totals = (unsigned long long*)totals;
  a.ws_codes = in_lds ? nullptr : (uint32_t*)workspace;
  a.ws_codes_stride = (long long)w;
  hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
