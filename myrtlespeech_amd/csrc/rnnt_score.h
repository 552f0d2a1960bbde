// The fused scorer's kernels (rnnt_score.hip), shared with the fused loss's backward (rnnt_joint_loss.hip): the packing of
// w_out into fp16 hi + lo planes in MFMA operand order, and the cells kernel -- a GEMM whose A operand tanh(enc_p[t] +
// pred_p[u]) is generated -- with its two epilogues:
//   EMIT = false  the scorer's: online log-sum-exp over the column tiles, b and e into the skewed planes (and Z, when asked)
//   EMIT = true   the backward's: ONE column tile per workgroup (blockIdx.y), the logits turned into the cell's gradient row
//                 g (the formula of ms_rnnt_loss_forward's comment) and stored as fp16 hi + lo planes, row-major and transposed
// The mainloop is one piece of code: a logit of the EMIT form is the scorer's bit for bit (the same planes, the same K order;
// a 32-column block's accumulator does not depend on how many blocks the column tile holds).
#pragma once
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"

namespace ms {

constexpr int RS_TT = 8;               // frames of a cell tile
constexpr int RS_TU = 16;              // prediction rows of a cell tile
constexpr int RS_ROWS = RS_TT * RS_TU; // 128 GEMM rows, 32 per wave
constexpr int RS_THREADS = 256;
constexpr int RS_JS = 64;              // J slab staged in LDS: 4 MFMA K steps of 16
constexpr int RS_STRIDE = RS_JS + 4;   // LDS row stride in floats: 16-byte aligned rows, 16 rows spread over all 64 banks
constexpr int RS_CB_PAD = 4;           // the packed image holds a multiple of 4 column blocks (the widest column tile)
constexpr float RS_G_SCALE = 4096.f;   // g is split as 2^12 g: |g| <= |grad_nll| <= 8 stays inside fp16, 2^-26 is still normal

static inline size_t rs_col_blocks(int V1) { return (size_t)cdiv(cdiv(V1, 32), RS_CB_PAD) * RS_CB_PAD; }
static inline size_t rs_k_steps(int J) { return (size_t)cdiv(J, RS_JS) * (RS_JS / 16); }
// [column block][K step][hi, lo][lane] x 16 bytes
static inline size_t rs_packed_bytes(int J, int V1) { return rs_col_blocks(V1) * rs_k_steps(J) * 2 * 64 * sizeof(u32x4_); }

// pack, cells (Z may be NULL), lattice pass: what ms_rnnt_score and ms_rnnt_joint_loss_forward both are.  The workspace holds
// the two skewed planes and the packed w_out; the arguments have been checked.
int rnnt_score_launch(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out, const int32_t* in_lens,
                      const int32_t* targets, const int32_t* tgt_lens, float* nll, float* Z, float* alpha, float* beta, int N,
                      int T, int U1, int J, int V1, int blank, void* workspace, hipStream_t st);

// pack and cells alone, without the lattice pass: the two skewed planes (and Z, when asked) are left in the workspace laid
// out as above.  What the forced aligner (rnnt_align.hip) runs its own walk on.
int rnnt_score_cells_launch(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                            const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* Z, int N, int T,
                            int U1, int J, int V1, int blank, void* workspace, hipStream_t st);

// the shapes the launches serve: the loss's, and grids that fit 31 bits
bool rnnt_score_supported(int N, int T, int U1, int J, int V1);

}  // namespace ms

// (rnnt_align.hip runs the launches above and has no use for the kernels: it defines RNNT_SCORE_DECLARATIONS_ONLY)
#ifndef RNNT_SCORE_DECLARATIONS_ONLY
namespace {

using ms::f32x16;
using ms::f32x4;
using ms::u32x4_;
using ms::RS_CB_PAD;
using ms::RS_JS;
using ms::RS_ROWS;
using ms::RS_STRIDE;
using ms::RS_THREADS;
using ms::RS_TT;
using ms::RS_TU;

// one thread per (column block, K step, lane): the 8 consecutive k of row v = 32 cb + (lane & 31) of the [V1, J] operand
// w[v row_stride + k k_stride] that lane holds as the B fragment of mfma_f32_32x32x16_f16, zero outside [V1, J]
// (w_out itself: row_stride = J, k_stride = 1; its transpose, for the backward's dH product: V1 <-> J, row_stride = 1)
__global__ __launch_bounds__(256) void rnnt_score_pack_kernel(const float* __restrict__ w_out, u32x4_* __restrict__ packed,
                                                              int J, int V1, int k_steps, long total, long row_stride,
                                                              long k_stride) {
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
    const float w = (v < V1 && k0 + j < J) ? w_out[(size_t)v * row_stride + (size_t)(k0 + j) * k_stride] : 0.f;
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

// fp16 hi + lo of a gradient value; a NaN stays one (the clamp of plane_split would not keep it)
__device__ __forceinline__ void rs_split_g(float g, unsigned& hi, unsigned& lo) {
  if (g != g) {
    hi = 0x7e00u;
    lo = 0u;
  } else {
    ms::plane_split<true>(g, hi, lo);
  }
}

// What the EMIT epilogue reads and writes: the band is the units (utterance n, frame tile ti) q0 .. q0 + units - 1 in the
// order q = n tiles_t + ti; band row ((q - q0) 8 + frame of the tile) U1p + u, U1p = 16 tiles_u.
struct rs_emit_args {
  const float* nll;
  const float* Z;
  const float* alpha;
  const float* beta;
  const float* grad_nll;
  unsigned short* g_hi;    // [rows_b][v1p]
  unsigned short* g_lo;
  unsigned short* gt_hi;   // [v1p][rows_b]
  unsigned short* gt_lo;
  int q0, rows_b, v1p;
};

// NB: 32-column blocks per column tile
template <int NB, bool EMIT>
__global__ __launch_bounds__(RS_THREADS) void rnnt_score_cells_kernel(
    const float* __restrict__ enc_p, const float* __restrict__ pred_p, const u32x4_* __restrict__ packed,
    const float* __restrict__ b_out, const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ tgt_lens, float* __restrict__ b_sk, float* __restrict__ e_sk, float* __restrict__ z_out, int N,
    int T, int U1, int J, int V1, int blank, int tiles_t, int tiles_u, rs_emit_args em) {
  __shared__ __attribute__((aligned(16))) float stage[(RS_TT + RS_TU) * RS_STRIDE];   // enc rows 0..7, pred rows 8..23
  // scorer: x[blank], x[y_u], the row's maximum and sum.  EMIT: Z, alpha + beta - ll, alpha + beta(t+1, u), alpha + beta(t, u+1)
  __shared__ float xb_s[RS_ROWS], xe_s[RS_ROWS], m_s[RS_ROWS], s_s[RS_ROWS];
  __shared__ float gn_s[EMIT ? RS_ROWS : 1];       // EMIT: 2^12 grad_nll[n]
  __shared__ int live_s[EMIT ? RS_ROWS : 1];       // EMIT: the row's cell exists
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ui = blockIdx.x % tiles_u;
  const int q_ = blockIdx.x / tiles_u + (EMIT ? em.q0 : 0);
  const int ti = q_ % tiles_t, n = q_ / tiles_t;
  const int t0 = ti * RS_TT, u0 = ui * RS_TU;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  const int n_slabs = (J + RS_JS - 1) / RS_JS;
  const int k_steps = n_slabs * (RS_JS / 16);
  const int n_ctiles = (V1 + 32 * NB - 1) / (32 * NB);
  const int ct_begin = EMIT ? (int)blockIdx.y : 0, ct_end = EMIT ? (int)blockIdx.y + 1 : n_ctiles;
  float nl = 0.f;
  // EMIT: first band row of the tile's frame 0, row u0
  size_t rb0 = 0;
  if constexpr (EMIT) {
    nl = em.nll[n];
    rb0 = ((size_t)(blockIdx.x / tiles_u) * RS_TT) * ((size_t)tiles_u * RS_TU) + u0;
    // no cell, or an utterance that contributes nothing (nll = +inf): zeros, so that the rows drop out of every sum
    if (!ms::rl_lens_ok(Tn, Un, T, U1) || t0 >= Tn || u0 > Un || fabsf(nl) == INFINITY) {   // (uniform)
      const size_t u1p = (size_t)tiles_u * RS_TU;
      const int c0 = ct_begin * 32 * NB;
      for (int i = tid; i < RS_ROWS * 32 * NB; i += RS_THREADS) {
        const int row = i / (32 * NB), col = i % (32 * NB);
        const size_t o = (rb0 + (size_t)(row >> 4) * u1p + (row & 15)) * em.v1p + c0 + col;
        em.g_hi[o] = 0;
        em.g_lo[o] = 0;
      }
      for (int i = tid; i < RS_ROWS * 32 * NB; i += RS_THREADS) {
        const int col = i / RS_ROWS, row = i % RS_ROWS;
        const size_t o = (size_t)(c0 + col) * em.rows_b + rb0 + (size_t)(row >> 4) * u1p + (row & 15);
        em.gt_hi[o] = 0;
        em.gt_lo[o] = 0;
      }
      return;
    }
    if (tid < RS_ROWS) {
      const int t = t0 + (tid >> 4), u = u0 + (tid & 15);
      const bool live = t < Tn && u <= Un;
      live_s[tid] = live;
      if (live) {
        const size_t r = ((size_t)n * T + t) * U1 + u;
        const float a = em.alpha[r];
        // the successor through the blank: beta(t+1, u); past the last frame only (T_n-1, U_n) has one, the end itself
        const float tb = (t + 1 < Tn) ? em.beta[r + U1] : (u == Un ? 0.f : ms::rl_neg_inf());
        const float te = (u < Un) ? em.beta[r + 1] : ms::rl_neg_inf();
        xb_s[tid] = em.Z[r];
        xe_s[tid] = (a + em.beta[r]) + nl;               // alpha + beta - ll
        m_s[tid] = a + tb;
        s_s[tid] = a + te;
        gn_s[tid] = em.grad_nll[n] * ms::RS_G_SCALE;
      }
    }
  } else {
    if (!ms::rl_lens_ok(Tn, Un, T, U1) || t0 >= Tn || u0 > Un) return;   // (uniform: the whole workgroup leaves)
    if (tid < RS_ROWS) xb_s[tid] = xe_s[tid] = ms::rl_neg_inf();
  }

  // ---- staging: thread -> 6 words of the slab, row sr + 4 i (i < 6), column sk; rows clamped to existing cells
  const int sk = tid & (RS_JS - 1), sr = tid >> 6;
  const float* src[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int row = sr + 4 * i;                                  // 0..7 enc, 8..23 pred
    if (row < RS_TT) src[i] = enc_p + ((size_t)min(t0 + row, Tn - 1) * N + n) * J;
    else src[i] = pred_p + ((size_t)min(u0 + row - RS_TT, Un) * N + n) * J;
  }
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
  for (int ct = ct_begin; ct < ct_end; ++ct) {
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
        if (slab + 1 < n_slabs || ct + 1 < ct_end) load_slab(nx);
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
    const int c0 = ct * 32 * NB;
    if constexpr (EMIT) {
      // ---- the column tile's logits into the gradient row g of every cell, 2^12 g as fp16 hi + lo, in both layouts
      const size_t u1p = (size_t)tiles_u * RS_TU;
      const bool poisoned = nl != nl;                            // a NaN utterance: NaN in its cells' rows
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        const int v = c0 + 32 * cb + r;
        const bool in = v < V1;
        const float bias = (in && b_out) ? b_out[v] : 0.f;
        unsigned ghi[16], glo[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float x = in ? acc[cb][i] + bias : ms::rl_neg_inf();
          const int row = 32 * w + ms::mfma32_row(i, lane);
          float g = 0.f;
          if (live_s[row]) {
            const float d = x - xb_s[row];
            float val = __expf(d + xe_s[row]);
            if (v == blank) val -= __expf((d + m_s[row]) + nl);
            if (v == lab[(i & 3) + 4 * ((i >> 2) & 1)]) val -= __expf((d + s_s[row]) + nl);
            g = gn_s[row] * val;
            if (poisoned) g = in ? ms::rl_nan() : 0.f;
          }
          rs_split_g(g, ghi[i], glo[i]);
          // band row of accumulator row: frame 2 w + (row >> 4) of the tile, prediction row u0 + (row & 15)
          const int rw = ms::mfma32_row(i, lane);
          const size_t rb = rb0 + (size_t)(2 * w + (rw >> 4)) * u1p + (rw & 15);
          em.g_hi[rb * em.v1p + v] = (unsigned short)ghi[i];
          em.g_lo[rb * em.v1p + v] = (unsigned short)glo[i];
        }
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {                         // registers 4 gq .. 4 gq + 3: four consecutive band rows
          const int rw = 8 * gq + 4 * h;
          const size_t o = (size_t)v * em.rows_b + rb0 + (size_t)(2 * w + (rw >> 4)) * u1p + (rw & 15);
          const uint2 ph = {ghi[4 * gq] | (ghi[4 * gq + 1] << 16), ghi[4 * gq + 2] | (ghi[4 * gq + 3] << 16)};
          const uint2 pl = {glo[4 * gq] | (glo[4 * gq + 1] << 16), glo[4 * gq + 2] | (glo[4 * gq + 3] << 16)};
          *reinterpret_cast<uint2*>(em.gt_hi + o) = ph;
          *reinterpret_cast<uint2*>(em.gt_lo + o) = pl;
        }
      }
    } else {
      // ---- the column tile's logits: into the running (max, sum) of every row, blank and label picked where they pass
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
  }
  if constexpr (EMIT) return;

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
  if (z_out) z_out[((size_t)n * T + t) * U1 + u] = bad ? ms::rl_nan() : z;   // (the fused loss: Z as ms_rnnt_loss_forward stores it)
}

}  // namespace
#endif  // RNNT_SCORE_DECLARATIONS_ONLY
