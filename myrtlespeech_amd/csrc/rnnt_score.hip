// RNN-T scoring without the logit lattice: the joint network fused into the loss's normaliser pass.
// OWN specification (the reference snapshot has no transducer): the comment on ms_rnnt_score in include/ms_hotpath.h, which
// rests on the one on ms_rnnt_loss_forward; tests/rnnt_score_ref.py restates it in numpy.
//
//   launch 1  rnnt_score_pack_kernel    w_out [V1, J] split into fp16 hi + lo and laid out in MFMA operand order in the workspace
//   launch 2  rnnt_score_cells_kernel   per existing cell (n, t, u): x = w_out . tanh(enc_p[t] + pred_p[u]) + b_out, its
//                                       log-sum-exp Z, and b = x[blank] - Z, e = x[y_u] - Z into the two skewed planes
//   launch 3  rnnt_loss_lattice_kernel  (rnnt_loss.hip, through ms::rnnt_lattice_launch): alpha, beta, nll
//
// The cells kernel is a GEMM whose A operand is generated: rows = cells, A = tanh(enc_p[t] + pred_p[u]), B = w_out.  A
// workgroup (4 waves) owns a tile of RS_TT = 8 frames x RS_TU = 16 prediction rows of one utterance = 128 GEMM rows, 32 per
// wave (2 frames x 16 u), and walks V1 in column tiles of NB x 32 columns (NB = 1, 2 or 4 by V1) with an ONLINE log-sum-exp:
// a running maximum and a running sum per accumulator row and LANE (16 rows per lane), merged across the 32 lanes of a row
// only once, after the last column tile.  The logits never leave registers.
// Inside a column tile the loop runs over J in slabs of RS_JS = 64: 8 rows of enc_p and 16 rows of pred_p are staged in LDS
// (6.5 KB; the next slab's loads are in flight while this one is computed), every lane forms the 8 tanh values of its
// mfma_f32_32x32x16_f16 A fragment in registers, splits them into fp16 hi + lo, and issues hi.hi + lo.hi + hi.lo per 32-column
// block (f16x3, the lo.lo term dropped); the B fragments come straight out of the packed image (L2-resident, 1 KB contiguous
// per wave and plane).
//
// Arithmetic: always f16x3 -- MS_PRECISION is NOT consulted (there is no float32-MFMA or bf16 variant of this kernel).
// w_out is split without a per-tensor scale: a lo plane below 2^-24 flushes, which the error bound of
// tests/test_rnnt_score_gpu.py charges for; the bound is stated for weights of magnitude within [2^-10, 2^10].
// tanh(x) = 1 - 2 / (exp(2x) + 1) with the hardware exp and reciprocal: absolute error of a few 2^-24, +-1 at +-inf, NaN kept.
//
// RECOMPUTE, not hold: with V1 above one column tile the tanh rows of a cell tile are formed again for every column tile
// (8 tanh per lane and 16-wide K step, against 3 NB MFMAs).  Holding 128 rows x J as hi + lo planes would need 4 J x 128 bytes
// of LDS (256 KB at J = 512: does not fit; 64 rows would), and J is arbitrary here.  The measured share is in
// profiles/rnnt_score_time.json (tools/rnnt_score_time.py).
//
// Rows of a partial tile that do not exist are computed on clamped, in-bounds rows and never stored; MFMA rows are
// independent, so they cannot reach an existing row.  Tiles without an existing cell exit at once.  No workgroup waits on
// another: no spin, no status word, no atomics; the result bits are deterministic.
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"

namespace {

using ms::f32x16;
using ms::f32x4;
using ms::u32x4_;

constexpr int RS_TT = 8;               // frames of a cell tile
constexpr int RS_TU = 16;              // prediction rows of a cell tile
constexpr int RS_ROWS = RS_TT * RS_TU; // 128 GEMM rows, 32 per wave
constexpr int RS_THREADS = 256;
constexpr int RS_JS = 64;              // J slab staged in LDS: 4 MFMA K steps of 16
constexpr int RS_STRIDE = RS_JS + 4;   // LDS row stride in floats: 16-byte aligned rows, 16 rows spread over all 64 banks
constexpr int RS_CB_PAD = 4;           // the packed image holds a multiple of 4 column blocks (the widest column tile)

inline size_t rs_col_blocks(int V1) { return (size_t)ms::cdiv(ms::cdiv(V1, 32), RS_CB_PAD) * RS_CB_PAD; }
inline size_t rs_k_steps(int J) { return (size_t)ms::cdiv(J, RS_JS) * (RS_JS / 16); }
// [column block][K step][hi, lo][lane] x 16 bytes
inline size_t rs_packed_bytes(int J, int V1) { return rs_col_blocks(V1) * rs_k_steps(J) * 2 * 64 * sizeof(u32x4_); }

// one thread per (column block, K step, lane): the 8 consecutive k of w_out row v = 32 cb + (lane & 31) that lane holds as
// the B fragment of mfma_f32_32x32x16_f16, zero outside [V1, J]
__global__ __launch_bounds__(256) void rnnt_score_pack_kernel(const float* __restrict__ w_out, u32x4_* __restrict__ packed,
                                                              int J, int V1, int k_steps, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  const long q = i >> 6;
  const int ks = (int)(q % k_steps);
  const long cb = q / k_steps;
  const long v = cb * 32 + (lane & 31);
  const int k0 = ks * 16 + 8 * (lane >> 5);
  unsigned hi[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float w = (v < V1 && k0 + j < J) ? w_out[(size_t)v * J + k0 + j] : 0.f;
    ms::plane_split<true>(w, hi[j], lo[j]);
  }
  const u32x4_ h4 = {hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
  const u32x4_ l4 = {lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
  packed[(size_t)q * 128 + lane] = h4;
  packed[(size_t)q * 128 + 64 + lane] = l4;
}

__device__ __forceinline__ float rs_tanh(float x) {
#ifdef RS_PROBE_NO_TANH
  return x;   // MEASUREMENT BUILD ONLY (tools/rnnt_score_time.py --probe-lib): the same MFMA work and traffic, wrong results
#else
  // exp(2x) = +inf gives 1, 0 gives -1, NaN stays NaN
  return 1.f - 2.f * __frcp_rn(__expf(2.f * x) + 1.f);
#endif
}

// NB: 32-column blocks per column tile
template <int NB>
__global__ __launch_bounds__(RS_THREADS) void rnnt_score_cells_kernel(
    const float* __restrict__ enc_p, const float* __restrict__ pred_p, const u32x4_* __restrict__ packed,
    const float* __restrict__ b_out, const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ tgt_lens, float* __restrict__ b_sk, float* __restrict__ e_sk, int N, int T, int U1, int J,
    int V1, int blank, int tiles_t, int tiles_u) {
  __shared__ __attribute__((aligned(16))) float stage[(RS_TT + RS_TU) * RS_STRIDE];   // enc rows 0..7, pred rows 8..23
  __shared__ float xb_s[RS_ROWS], xe_s[RS_ROWS], m_s[RS_ROWS], s_s[RS_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ui = blockIdx.x % tiles_u;
  const int q_ = blockIdx.x / tiles_u;
  const int ti = q_ % tiles_t, n = q_ / tiles_t;
  const int t0 = ti * RS_TT, u0 = ui * RS_TU;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  if (!ms::rl_lens_ok(Tn, Un, T, U1) || t0 >= Tn || u0 > Un) return;   // (uniform: the whole workgroup leaves)

  if (tid < RS_ROWS) xb_s[tid] = xe_s[tid] = ms::rl_neg_inf();

  // ---- staging: thread -> 6 words of the slab, row sr + 4 i (i < 6), column sk; rows clamped to existing cells
  const int sk = tid & (RS_JS - 1), sr = tid >> 6;
  const float* src[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int row = sr + 4 * i;                                  // 0..7 enc, 8..23 pred
    if (row < RS_TT) src[i] = enc_p + ((size_t)min(t0 + row, Tn - 1) * N + n) * J;
    else src[i] = pred_p + ((size_t)min(u0 + row - RS_TT, Un) * N + n) * J;
  }
  const int n_slabs = (J + RS_JS - 1) / RS_JS;
  const int k_steps = n_slabs * (RS_JS / 16);
  const int n_ctiles = (V1 + 32 * NB - 1) / (32 * NB);
  float pre[6];
  auto load_slab = [&](int slab) {
    const int k = slab * RS_JS + sk;
#pragma unroll
    for (int i = 0; i < 6; ++i) pre[i] = k < J ? src[i][k] : 0.f;   // ragged slab: tanh(0 + 0) = 0 against zero weights
  };

  // ---- this lane's A rows and accumulator rows
  const int r = lane & 31, h = lane >> 5;
  const float* a_enc = stage + (2 * w + (r >> 4)) * RS_STRIDE + 8 * h;
  const float* a_pred = stage + (RS_TT + (r & 15)) * RS_STRIDE + 8 * h;
  // accumulator register i is row (i & 3) + 8 (i >> 2) + 4 h of the wave's 32: prediction row (i & 3) + 4 h + 8 ((i >> 2) & 1)
  int lab[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int u = u0 + (q & 3) + 4 * h + 8 * (q >> 2);
    lab[q] = -1;
    if (u < Un) {
      const int l = targets[(size_t)n * (U1 - 1) + u];
      if (ms::rl_label_ok(l, V1, blank)) lab[q] = l;
    }
  }

  float m_run[16], s_run[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    m_run[i] = ms::rl_neg_inf();
    s_run[i] = 0.f;
  }
  f32x16 acc[NB];

  load_slab(0);
  for (int ct = 0; ct < n_ctiles; ++ct) {
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
    const u32x4_* bt = packed + ((size_t)ct * NB * k_steps) * 128 + lane;
    for (int slab = 0; slab < n_slabs; ++slab) {
      __syncthreads();                                           // the previous slab's reads are done
#pragma unroll
      for (int i = 0; i < 6; ++i) stage[(sr + 4 * i) * RS_STRIDE + sk] = pre[i];
      __syncthreads();
      {                                                          // the next slab (of the next column tile: slab 0 again)
        const int nx = slab + 1 < n_slabs ? slab + 1 : 0;
        if (slab + 1 < n_slabs || ct + 1 < n_ctiles) load_slab(nx);
      }
#pragma unroll
      for (int ks = 0; ks < RS_JS / 16; ++ks) {
        const f32x4 e0 = *reinterpret_cast<const f32x4*>(a_enc + ks * 16);
        const f32x4 e1 = *reinterpret_cast<const f32x4*>(a_enc + ks * 16 + 4);
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(a_pred + ks * 16);
        const f32x4 p1 = *reinterpret_cast<const f32x4*>(a_pred + ks * 16 + 4);
        unsigned hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ms::plane_split_bounded<true>(rs_tanh(e0[j] + p0[j]), hi[j], lo[j]);
          ms::plane_split_bounded<true>(rs_tanh(e1[j] + p1[j]), hi[4 + j], lo[4 + j]);
        }
        const u32x4_ ah = {hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
        const u32x4_ al = {lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
        const int kstep = slab * (RS_JS / 16) + ks;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          const u32x4_* bp = bt + ((size_t)cb * k_steps + kstep) * 128;
          const u32x4_ bh = bp[0], bl = bp[64];
          acc[cb] = ms::mfma_32x32x16<true>(al, bh, acc[cb]);
          acc[cb] = ms::mfma_32x32x16<true>(ah, bl, acc[cb]);
          acc[cb] = ms::mfma_32x32x16<true>(ah, bh, acc[cb]);
        }
      }
    }
    // ---- the column tile's logits: into the running (max, sum) of every row, blank and label picked where they pass
    const int c0 = ct * 32 * NB;
    float x[NB][16];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      const int v = c0 + 32 * cb + r;
      const bool in = v < V1;
      const float bias = (in && b_out) ? b_out[v] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[cb][i] = in ? acc[cb][i] + bias : ms::rl_neg_inf();     // a ragged last tile: -inf into the log-sum-exp
        const int row = 32 * w + ms::mfma32_row(i, lane);
        if (v == blank) xb_s[row] = x[cb][i];                     // (one lane per row and symbol: no race)
        if (v == lab[(i & 3) + 4 * ((i >> 2) & 1)]) xe_s[row] = x[cb][i];
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float tm = x[0][i];
#pragma unroll
      for (int cb = 1; cb < NB; ++cb) tm = fmaxf(tm, x[cb][i]);
      const float mn = fmaxf(m_run[i], tm);
      // while every column so far is -inf the sum stays 0 and no (-inf) - (-inf) is formed; fmaxf drops a NaN logit, the
      // exp below keeps it; +inf gives exp(inf - inf) = NaN
      const float ms_ = mn == ms::rl_neg_inf() ? 0.f : mn;
      float s = s_run[i] * __expf(m_run[i] - ms_);
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) s += __expf(x[cb][i] - ms_);
      s_run[i] = s;
      m_run[i] = mn;
    }
  }

  // ---- merge the 32 lanes of every row (fixed order: deterministic)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float M = m_run[i];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    const float Ms = M == ms::rl_neg_inf() ? 0.f : M;
    float S = s_run[i] * __expf(m_run[i] - Ms);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) S += __shfl_xor(S, o, 64);
    if (r == 0) {
      const int row = 32 * w + ms::mfma32_row(i, lane);
      m_s[row] = M;
      s_s[row] = S;
    }
  }
  __syncthreads();
  if (tid >= RS_ROWS) return;
  const int t = t0 + (tid >> 4), u = u0 + (tid & 15);
  if (t >= Tn || u > Un) return;
  const float M = m_s[tid];
  const float lse = logf(s_s[tid]);
  const float z = M + lse;
  const bool bad = !(fabsf(z) < INFINITY);         // a NaN or +inf logit, a row of -inf: poisons the utterance
  float bv = (xb_s[tid] - M) - lse;
  float ev = ms::rl_neg_inf();
  if (u < Un) {
    const int l = targets[(size_t)n * (U1 - 1) + u];
    if (ms::rl_label_ok(l, V1, blank)) ev = (xe_s[tid] - M) - lse;   // (else: the lattice pass reports the utterance)
  }
  if (bad) bv = ev = ms::rl_nan();
  const size_t o = ((size_t)n * ms::rl_skew_rows(T, U1) + (size_t)(t + u)) * U1 + u;
  b_sk[o] = bv;
  e_sk[o] = ev;
}

}  // namespace

extern "C" size_t ms_rnnt_score_lattice_bytes(int N, int T, int U1) {
  if (N <= 0 || T <= 0 || U1 <= 0) return 0;
  return (size_t)2 * N * T * U1 * sizeof(float);
}

extern "C" size_t ms_rnnt_score_workspace_bytes(int N, int T, int U1, int J, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V1 <= 0) return 0;
  return 2 * ms::rl_skew_plane_bytes(N, T, U1) + rs_packed_bytes(J, V1);
}

extern "C" int ms_rnnt_score(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                             const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* nll, float* lattice,
                             int N, int T, int U1, int J, int V1, int blank, void* workspace, size_t workspace_bytes,
                             void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && J > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(enc_p && pred_p && w_out && in_lens && tgt_lens && nll && lattice && workspace, "null pointer");
  MS_REQUIRE(targets || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  MS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  const int tiles_t = ms::cdiv(T, RS_TT), tiles_u = ms::cdiv(U1, RS_TU);
  const long tiles = (long)N * tiles_t * tiles_u;
  const long pack_threads = (long)(rs_col_blocks(V1) * rs_k_steps(J) * 64);
  if (!ms::rl_supported(N, T, U1) || tiles > 0x7fffffffL || (pack_threads + 255) / 256 > 0x7fffffffL) {
    ms::set_error("ms_rnnt_score: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_score_workspace_bytes(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_score: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t plane_bytes = ms::rl_skew_plane_bytes(N, T, U1);
  float* b_sk = (float*)workspace;
  float* e_sk = (float*)((char*)workspace + plane_bytes);
  u32x4_* packed = (u32x4_*)((char*)workspace + 2 * plane_bytes);
  const int k_steps = (int)rs_k_steps(J);
  hipLaunchKernelGGL(rnnt_score_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, st, w_out, packed, J,
                     V1, k_steps, pack_threads);
  MS_LAUNCH_CHECK();
  const dim3 grid((unsigned)tiles), block(RS_THREADS);
#define RS_CELLS(NB)                                                                                                      \
  hipLaunchKernelGGL(rnnt_score_cells_kernel<NB>, grid, block, 0, st, enc_p, pred_p, packed, b_out, in_lens, targets,     \
                     tgt_lens, b_sk, e_sk, N, T, U1, J, V1, blank, tiles_t, tiles_u)
  if (V1 <= 32) RS_CELLS(1);
  else if (V1 <= 64) RS_CELLS(2);
  else RS_CELLS(4);
#undef RS_CELLS
  MS_LAUNCH_CHECK();
  const size_t plane = (size_t)N * T * U1;
  return ms::rnnt_lattice_launch(in_lens, targets, tgt_lens, b_sk, e_sk, lattice, lattice + plane, nll, N, T, U1, V1, blank, st);
}
