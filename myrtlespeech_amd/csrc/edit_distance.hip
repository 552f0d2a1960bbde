// Batched edit distance with operation counts: the word (or token) error rate's arithmetic on the device.  The specification
// is the comment on ms_edit_distance in include/ms_hotpath.h; tests/edit_distance_ref.py restates it in Python.  Integers only.
//
//   launch 1 (word mode)  ed_units_kernel   a workgroup per utterance: the labels of both rows -> letters (in-range labels that
//                                           are not the separator, compacted in LDS) and word starts, by one wave per side and
//                                           64 labels per step (two ballots, a carried "the last label seen was a separator");
//                                           a key per word (18 bits of a hash, the length); then every word looks for the FIRST
//                                           equal word among the utterance's hypothesis and reference words (the key filters,
//                                           the letters decide) and takes its index as its unit id.  Ids and counts go to the
//                                           workspace.  Token mode has no launch 1: a label is its own id.
//   launch 2              ed_wave_kernel    when one side's units fit a wave (<= 63: host arithmetic on the row widths): a wave
//                                           per utterance, a lane per unit of that side, the two previous anti-diagonals in
//                                           registers, the other side's units moving through the lanes as a shift register fed
//                                           from 64-unit chunks.  No LDS, no barrier.
//                         ed_block_kernel   otherwise: a workgroup per utterance, three rolling anti-diagonals in LDS indexed
//                                           by the hypothesis position (a strided loop once they exceed the workgroup), one
//                                           barrier per anti-diagonal.
//
// A cell is ONE 32-bit word, cost << 16 | substitutions.  Deletions and insertions need not travel: every path to (i, j) has
// i - I = j - D diagonal steps and cost = S + D + I, so D = (cost - S - (i - j)) / 2 and I = D + i - j at the last cell.
// A diagonal step adds 0x10001 on a mismatch, a deletion or an insertion 0x10000; candidates are compared on cost alone, in the
// specification's order, strictly.
#include "common.h"

namespace {

constexpr int ED_THREADS = 256;
constexpr int ED_MAX_LEN = 4096;                      // units a side (MS_EDIT_MAX_LEN): a row of 4096 labels in token mode,
constexpr int ED_MAX_WORD_ROW = 2 * ED_MAX_LEN - 1;   // of 8191 in word mode (4096 one-letter words and their separators)
constexpr int ED_WAVE_UNITS = 63;                     // a wave serves a side of up to 63 units: lanes 0 .. 63 are positions 0 .. 63
constexpr size_t ED_LDS_MAX = 132 * 1024;             // dynamic LDS at the limits: ed_block_kernel 80 KB, ed_units_kernel 128 KB

static_assert(ED_MAX_LEN == MS_EDIT_MAX_LEN, "the header documents the limit");
static_assert((size_t)ED_MAX_LEN * 2 * 4 + (size_t)3 * (ED_MAX_LEN + 1) * 4 <= ED_LDS_MAX, "ed_block_kernel");
static_assert((size_t)ED_MAX_WORD_ROW * 2 * 4 + (size_t)2 * (2 * ED_MAX_LEN) * 4 <= ED_LDS_MAX, "ed_units_kernel");
static_assert(ED_MAX_WORD_ROW < (1 << 14), "a word's length takes 14 bits of its key");

typedef unsigned long long u64;

// units a row of `stride` labels can hold
inline int unit_cap(int stride, int mode) { return mode == MS_EDIT_WORDS ? (stride + 1) / 2 : stride; }

struct WsLayout {
  size_t counts, ids_h, ids_r, total;                 // byte offsets: counts int32 [n][2] | ids_h [n][cap_h] | ids_r [n][cap_r]
};
inline WsLayout ws_layout(int n, int max_hyp, int max_ref) {
  WsLayout l;
  const size_t cap_h = (size_t)unit_cap(max_hyp, MS_EDIT_WORDS), cap_r = (size_t)unit_cap(max_ref, MS_EDIT_WORDS);
  l.counts = 0;
  l.ids_h = ms::align_up((size_t)n * 2 * sizeof(int32_t), 256);
  l.ids_r = l.ids_h + ms::align_up((size_t)n * cap_h * sizeof(int32_t), 256);
  l.total = l.ids_r + ms::align_up((size_t)n * cap_r * sizeof(int32_t), 256);
  return l;
}

__device__ __forceinline__ int ed_clamp_len(int len, int cap) { return min(max(len, 0), cap); }

// One side of one utterance by one wave: letters -> let[let_off ..), word starts (positions in `let`) -> wstart[w_off ..).
// Returns the letter and word counts in every lane.
__device__ __forceinline__ void ed_scan_side(const int32_t* __restrict__ row, int len, int separator, int n_symbols, int lane,
                                             int* let, int let_off, int* wstart, int w_off, int& n_letters, int& n_words) {
  int letters = 0, words = 0;
  bool prev_sep = true;                               // nothing seen yet: the next letter starts a word
  const u64 below = (1ull << lane) - 1ull;
  for (int base = 0; base < len; base += 64) {        // (uniform: every lane reaches the ballots)
    const int p = base + lane;
    int lab = -1;
    if (p < len) lab = row[p];                        // nothing at or past `len` is read
    const bool valid = p < len && lab >= 0 && lab < n_symbols;
    const bool sep = valid && lab == separator;
    const u64 V = __ballot(valid), Sp = __ballot(sep);
    const u64 L = V & ~Sp;
    bool start = false;
    if (valid && !sep) {
      const u64 before = V & below;                   // the valid labels of this step in front of this one
      start = before ? (((Sp >> (63 - __clzll((long long)before))) & 1ull) != 0ull) : prev_sep;
    }
    const u64 Ws = __ballot(start);
    if (valid && !sep) {
      const int li = let_off + letters + __popcll(L & below);
      let[li] = lab;
      if (start) wstart[w_off + words + __popcll(Ws & below)] = li;
    }
    if (V) prev_sep = ((Sp >> (63 - __clzll((long long)V))) & 1ull) != 0ull;
    letters += __popcll(L);
    words += __popcll(Ws);
  }
  n_letters = letters;
  n_words = words;
}

// LDS: let [hyp_stride + ref_stride] | wstart [cap_h + cap_r] | wkey [cap_h + cap_r] (hash << 14 | length)
// Hypothesis letters start at let[0], reference letters at let[hyp_stride]; hypothesis words take slots 0 .., reference words
// slots cap_h ...  A word's combined index c (hypothesis words first, then reference words, both in order) is its unit id
// unless an equal word has a smaller one.
__global__ __launch_bounds__(ED_THREADS) void ed_units_kernel(const int32_t* __restrict__ hyp, int hyp_stride,
                                                              const int32_t* __restrict__ hyp_lens,
                                                              const int32_t* __restrict__ ref, int ref_stride,
                                                              const int32_t* __restrict__ ref_lens, int separator, int n_symbols,
                                                              int32_t* __restrict__ counts, int32_t* __restrict__ ids_h,
                                                              int32_t* __restrict__ ids_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ed_smem[];
  __shared__ int side_counts[4];                      // letters, words of the hypothesis; of the reference
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap_h = (hyp_stride + 1) / 2, cap_r = (ref_stride + 1) / 2;
  int* let = reinterpret_cast<int*>(ed_smem);
  int* wstart = let + hyp_stride + ref_stride;
  unsigned* wkey = reinterpret_cast<unsigned*>(wstart + cap_h + cap_r);

  if (w < 2) {
    int nl, nw;
    if (w == 0)
      ed_scan_side(hyp + (size_t)n * hyp_stride, ed_clamp_len(hyp_lens[n], hyp_stride), separator, n_symbols, lane, let, 0, wstart,
                   0, nl, nw);
    else
      ed_scan_side(ref + (size_t)n * ref_stride, ed_clamp_len(ref_lens[n], ref_stride), separator, n_symbols, lane, let,
                   hyp_stride, wstart, cap_h, nl, nw);
    if (lane == 0) {
      side_counts[2 * w] = nl;
      side_counts[2 * w + 1] = nw;
    }
  }
  __syncthreads();
  const int Lh = side_counts[0], Wh = side_counts[1], Lr = side_counts[2], Wr = side_counts[3];
  const int W = Wh + Wr;                              // Wh <= cap_h and Wr <= cap_r: a word has a letter, two words a separator between
  for (int c = tid; c < W; c += ED_THREADS) {
    const bool is_h = c < Wh;
    const int slot = is_h ? c : cap_h + (c - Wh);
    const int start = wstart[slot];
    const bool last = is_h ? (c + 1 == Wh) : (c + 1 == W);
    const int end = last ? (is_h ? Lh : hyp_stride + Lr) : wstart[slot + 1];
    unsigned h = 2166136261u;                         // FNV-1a over the letters: a filter only
    for (int k = start; k < end; ++k) h = (h ^ (unsigned)let[k]) * 16777619u;
    wkey[slot] = (h << 14) | (unsigned)(end - start);
  }
  __syncthreads();
  for (int c = tid; c < W; c += ED_THREADS) {
    const int slot = c < Wh ? c : cap_h + (c - Wh);
    const int start = wstart[slot];
    const unsigned key = wkey[slot];
    const int len = (int)(key & 0x3fffu);
    int id = c;
    for (int o = 0; o < c; ++o) {                     // (every lane of a wave reads the same word o: a broadcast)
      const int oslot = o < Wh ? o : cap_h + (o - Wh);
      if (wkey[oslot] != key) continue;
      const int ostart = wstart[oslot];
      int k = 0;
      while (k < len && let[ostart + k] == let[start + k]) ++k;
      if (k == len) { id = o; break; }
    }
    if (c < Wh) ids_h[(size_t)n * cap_h + c] = id;
    else ids_r[(size_t)n * cap_r + (c - Wh)] = id;
  }
  if (tid == 0) {
    counts[2 * n] = Wh;
    counts[2 * n + 1] = Wr;
  }
}

__device__ __forceinline__ unsigned ed_cell(unsigned diag, unsigned del, unsigned ins, bool differ) {
  unsigned best = diag + (differ ? 0x10001u : 0u);
  const unsigned d = del + 0x10000u, i = ins + 0x10000u;
  if ((d >> 16) < (best >> 16)) best = d;
  if ((i >> 16) < (best >> 16)) best = i;
  return best;
}

// distance, S, D, I, m, n of one utterance from its last cell; `totals` += the six (64-bit integer atomics: any order, same sum)
__device__ __forceinline__ void ed_write(unsigned cell, int m, int n_units, int32_t* __restrict__ out, u64* __restrict__ totals) {
  const int cost = (int)(cell >> 16), S = (int)(cell & 0xffffu);
  const int D = (cost - S - (m - n_units)) / 2, I = D + m - n_units;
  const int v[6] = {cost, S, D, I, m, n_units};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    out[k] = v[k];
    if (totals && v[k]) atomicAdd(totals + k, (u64)v[k]);
  }
}

// A wave per utterance.  Lane x is position x of the SHORT side (the hypothesis, or the reference with BY_REF), y = d - x the
// position on the other side; p1 / p2 hold this lane's cells of the two previous anti-diagonals, the lane below supplies
// (x - 1, y) and (x - 1, y - 1).  The other side's unit for lane x at diagonal d is the one lane x - 1 used at d - 1.
template <bool BY_REF>
__global__ __launch_bounds__(ED_THREADS) void ed_wave_kernel(const int32_t* __restrict__ A, int a_stride, int a_cap,
                                                             const int32_t* __restrict__ a_len, const int32_t* __restrict__ B,
                                                             int b_stride, int b_cap, const int32_t* __restrict__ b_len,
                                                             int len_stride, int N, int32_t* __restrict__ out,
                                                             u64* __restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * (ED_THREADS / 64) + (threadIdx.x >> 6);
  if (u >= N) return;                                 // (a whole wave: the kernel has no workgroup barrier)
  const int m = ed_clamp_len(a_len[u * len_stride], a_cap), nn = ed_clamp_len(b_len[u * len_stride], b_cap);
  const int32_t* X = BY_REF ? B + (size_t)u * b_stride : A + (size_t)u * a_stride;
  const int32_t* Y = BY_REF ? A + (size_t)u * a_stride : B + (size_t)u * b_stride;
  const int sx = min(BY_REF ? nn : m, ED_WAVE_UNITS), sy = BY_REF ? m : nn;     // (sx <= its cap <= 63 by the host's gate)
  const int x = lane;
  const int ux = (x >= 1 && x <= sx) ? X[x - 1] : 0;
  unsigned p1 = 0, p2 = 0;
  int uy = 0, ychunk = 0;
  for (int d = 0; d <= sx + sy; ++d) {                // (uniform in the wave: every lane reaches the shuffles)
    const int k = d - 2;                              // lane 1 needs Y[k] now
    if (k >= 0 && (k & 63) == 0) ychunk = (k + lane < sy) ? Y[k + lane] : 0;
    const int feed = __shfl(ychunk, k & 63, 64);
    const int uy_up = __shfl_up(uy, 1, 64);
    uy = (lane == 1) ? feed : uy_up;
    const unsigned up1 = __shfl_up(p1, 1, 64), up2 = __shfl_up(p2, 1, 64);
    const int y = d - x;
    unsigned v;
    if (x == 0) v = (unsigned)max(y, 0) << 16;
    else if (y <= 0) v = (unsigned)x << 16;           // (y < 0: not a cell yet; the value is never used)
    else v = BY_REF ? ed_cell(up2, up1, p1, ux != uy) : ed_cell(up2, p1, up1, ux != uy);
    p2 = p1;
    p1 = v;                                           // (lanes past sx, and y past sy, carry values nobody reads)
  }
  // lane sx finished with cell (sx, sy) at the last diagonal; lanes below it have since moved past y = sy
  const unsigned cell = __shfl(p1, sx, 64);
  if (lane == 0) ed_write(cell, m, nn, out + (size_t)u * 6, totals);
}

// LDS: ua [a_cap] | ub [b_cap] | three anti-diagonals [a_cap + 1] each, indexed by the hypothesis position i
__global__ __launch_bounds__(ED_THREADS) void ed_block_kernel(const int32_t* __restrict__ A, int a_stride, int a_cap,
                                                              const int32_t* __restrict__ a_len, const int32_t* __restrict__ B,
                                                              int b_stride, int b_cap, const int32_t* __restrict__ b_len,
                                                              int len_stride, int32_t* __restrict__ out, u64* __restrict__ totals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ed_smem[];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int m = ed_clamp_len(a_len[(size_t)u * len_stride], a_cap), nn = ed_clamp_len(b_len[(size_t)u * len_stride], b_cap);
  int* ua = reinterpret_cast<int*>(ed_smem);
  int* ub = ua + a_cap;
  unsigned* cur = reinterpret_cast<unsigned*>(ub + b_cap);
  unsigned* p1 = cur + (a_cap + 1);
  unsigned* p2 = p1 + (a_cap + 1);
  for (int i = tid; i < m; i += ED_THREADS) ua[i] = A[(size_t)u * a_stride + i];
  for (int j = tid; j < nn; j += ED_THREADS) ub[j] = B[(size_t)u * b_stride + j];
  __syncthreads();
  for (int d = 0; d <= m + nn; ++d) {
    const int lo = max(0, d - nn), hi = min(m, d);
    for (int i = lo + tid; i <= hi; i += ED_THREADS) {
      const int j = d - i;
      unsigned v;
      if (i == 0) v = (unsigned)j << 16;
      else if (j == 0) v = (unsigned)i << 16;
      else v = ed_cell(p2[i - 1], p1[i], p1[i - 1], ua[i - 1] != ub[j - 1]);   // (i-1, j-1) | (i, j-1) deletion | (i-1, j) insertion
      cur[i] = v;
    }
    __syncthreads();
    unsigned* t = p2; p2 = p1; p1 = cur; cur = t;
  }
  if (tid == 0) ed_write(p1[m], m, nn, out + (size_t)u * 6, totals);
}

}  // namespace

extern "C" size_t ms_edit_distance_workspace_bytes(int n, int max_hyp, int max_ref) {
  if (n <= 0 || max_hyp < 0 || max_ref < 0) return 0;
  return ws_layout(n, max_hyp, max_ref).total;
}

extern "C" int ms_edit_distance(const int32_t* hyp, int hyp_stride, const int32_t* hyp_lens, const int32_t* ref, int ref_stride,
                                const int32_t* ref_lens, int n, int mode, int separator, int n_symbols, int32_t* out,
                                int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(n >= 0 && hyp_stride >= 0 && ref_stride >= 0, "bad shape");
  MS_REQUIRE(mode == MS_EDIT_TOKENS || mode == MS_EDIT_WORDS, "mode takes MS_EDIT_TOKENS or MS_EDIT_WORDS");
  MS_REQUIRE(mode == MS_EDIT_TOKENS || n_symbols >= 0, "n_symbols must not be negative");
  if (n == 0) return MS_OK;
  MS_REQUIRE(hyp && hyp_lens && ref && ref_lens && out && workspace, "null pointer");
  MS_REQUIRE(totals == nullptr || ((uintptr_t)totals & 7) == 0, "totals must be 8-byte aligned");
  const int max_row = mode == MS_EDIT_WORDS ? ED_MAX_WORD_ROW : ED_MAX_LEN;
  if (hyp_stride > max_row || ref_stride > max_row) {
    ms::set_error("ms_edit_distance: supported up to 4096 units a side (rows of 4096 labels, of 8191 in word mode)");
    return MS_ERR_UNSUPPORTED;
  }
  const WsLayout l = ws_layout(n, hyp_stride, ref_stride);
  if (workspace_bytes < l.total) {
    ms::set_error("ms_edit_distance: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  static ms::DeviceOnce attr_once;
  if (attr_once.need()) {
    MS_HIP(hipFuncSetAttribute((const void*)ed_units_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ED_LDS_MAX));
    MS_HIP(hipFuncSetAttribute((const void*)ed_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ED_LDS_MAX));
    attr_once.done();
  }
  hipStream_t st = (hipStream_t)stream;
  const int cap_h = unit_cap(hyp_stride, mode), cap_r = unit_cap(ref_stride, mode);
  const int32_t *A = hyp, *B = ref, *a_len = hyp_lens, *b_len = ref_lens;
  int a_stride = hyp_stride, b_stride = ref_stride, len_stride = 1;
  if (mode == MS_EDIT_WORDS) {
    int32_t* counts = (int32_t*)((char*)workspace + l.counts);
    int32_t* ids_h = (int32_t*)((char*)workspace + l.ids_h);
    int32_t* ids_r = (int32_t*)((char*)workspace + l.ids_r);
    const size_t lds = ((size_t)hyp_stride + ref_stride + (size_t)2 * (cap_h + cap_r)) * sizeof(int32_t);
    hipLaunchKernelGGL(ed_units_kernel, dim3(n), dim3(ED_THREADS), lds, st, hyp, hyp_stride, hyp_lens, ref, ref_stride, ref_lens,
                       separator, n_symbols, counts, ids_h, ids_r);
    MS_LAUNCH_CHECK();
    A = ids_h; B = ids_r; a_len = counts; b_len = counts + 1;
    a_stride = cap_h; b_stride = cap_r; len_stride = 2;
  }
  u64* tot = (u64*)totals;
  if (cap_h <= ED_WAVE_UNITS || cap_r <= ED_WAVE_UNITS) {
    const dim3 grid((unsigned)((n + ED_THREADS / 64 - 1) / (ED_THREADS / 64)));
    if (cap_r < cap_h)
      hipLaunchKernelGGL(ed_wave_kernel<true>, grid, dim3(ED_THREADS), 0, st, A, a_stride, cap_h, a_len, B, b_stride, cap_r, b_len,
                         len_stride, n, out, tot);
    else
      hipLaunchKernelGGL(ed_wave_kernel<false>, grid, dim3(ED_THREADS), 0, st, A, a_stride, cap_h, a_len, B, b_stride, cap_r, b_len,
                         len_stride, n, out, tot);
  } else {
    const size_t lds = ((size_t)cap_h + cap_r + (size_t)3 * (cap_h + 1)) * sizeof(int32_t);
    hipLaunchKernelGGL(ed_block_kernel, dim3(n), dim3(ED_THREADS), lds, st, A, a_stride, cap_h, a_len, B, b_stride, cap_r, b_len,
                       len_stride, out, tot);
  }
  MS_LAUNCH_CHECK();
  return MS_OK;
}
