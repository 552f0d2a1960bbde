// The fused transducer loss WITH its gradient: ms_rnnt_score's forward plus a Z plane, and a backward that never holds a
// V1-wide row per cell for the whole lattice.  OWN specification: the comment on ms_rnnt_joint_loss_forward in
// include/ms_hotpath.h; tests/rnnt_joint_loss_ref.py restates it in numpy.
//
// forward   the scorer's three launches (ms::rnnt_score_launch, rnnt_score.hip) with one more output pointer: Z.
// backward  pack w_out (the scorer's image) and its transpose, then, band by band in stream order:
//   rjl_h_kernel      H^T of the band: tanh(enc_p[t] + pred_p[u]) as fp16 hi + lo planes [Jp][rows], zero rows for cells that
//                     do not exist or whose utterance has nll = +inf
//   cells kernel, EMIT (rnnt_score.h): the scorer's mainloop, one column tile per workgroup; the logits -- the forward's bit
//                     for bit -- become g = grad_nll (exp(x - Z + alpha + beta - ll) - blank term - label term), stored as
//                     2^12 g in fp16 hi + lo planes, G [rows][V1p] and G^T [V1p][rows]
//   rjl_dh_kernel     da = (G W) / 2^12 * (1 - h^2), float32 [rows][Jp]             (f16x3 MFMA, K = V1)
//   rjl_enc_kernel    d_enc_p[t, n] = sum_u da: complete, a band is whole frames of an utterance
//   rjl_pred_kernel   d_pred_p[u, n] (+)= sum_t da over the band's frames of n, bands in order
//   rjl_dw_kernel     partial sums of G^T H over chunks of the band's rows           (f16x3 MFMA, K = the chunk's rows)
//   rjl_dw_reduce_kernel  d_w_out (+)= (the chunks' partial sums, in order) / 2^12   (two-stage: a fixed order, no atomics)
//   rjl_db_kernel     d_b_out (+)= column sums of G / 2^12
// A band is a run of UNITS q = n tiles_t + ti (8 frames of one utterance, all U1 prediction rows, padded to whole cell
// tiles); the workspace sets how many units a band holds.  "(+)=": the first band that touches an output row writes it,
// later ones add -- launches on one stream, no atomics, no workgroup waits on another: the same inputs and the same
// workspace size give the same bits.  MS_PRECISION is not consulted.
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"
#include "rnnt_score.h"

namespace {

using ms::rs_col_blocks;
using ms::rs_k_steps;
using ms::rs_packed_bytes;

constexpr long RJL_MAX_UNITS = 4096;     // of a band: its rows stay far below 2^31
constexpr size_t RJL_PREFERRED = 500000000;

struct rjl_layout {
  size_t tiles_t, tiles_u, u1p, unit_rows, v1p, jp, total_units;
  size_t packed_bytes, packed_t_bytes, dw_splits, partial_bytes, fixed_bytes, unit_bytes;
};
constexpr size_t RJL_DW_WORKGROUPS = 640;   // the d_w_out product splits its K extent until it has about this many workgroups
constexpr size_t RJL_DW_MAX_SPLITS = 64;

inline rjl_layout rjl_make_layout(int N, int T, int U1, int J, int V1) {
  rjl_layout L;
  L.tiles_t = (size_t)ms::cdiv(T, RS_TT);
  L.tiles_u = (size_t)ms::cdiv(U1, RS_TU);
  L.u1p = L.tiles_u * RS_TU;
  L.unit_rows = RS_TT * L.u1p;                       // a multiple of 128
  L.v1p = rs_col_blocks(V1) * 32;                    // multiples of 128
  L.jp = rs_col_blocks(J) * 32;
  L.total_units = (size_t)N * L.tiles_t;
  L.packed_bytes = rs_packed_bytes(J, V1);
  L.packed_t_bytes = rs_packed_bytes(V1, J);
  // d_w_out has only (V1p / 128) (Jp / 128) output tiles: its K extent (the band's rows) is split over workgroups, the
  // partial sums [split][V1p][Jp] float32 are added in a second launch
  const size_t out_tiles = (L.v1p / 128) * (L.jp / 128);
  L.dw_splits = (RJL_DW_WORKGROUPS + out_tiles - 1) / out_tiles;
  if (L.dw_splits > RJL_DW_MAX_SPLITS) L.dw_splits = RJL_DW_MAX_SPLITS;
  L.partial_bytes = L.dw_splits * L.v1p * L.jp * sizeof(float);
  L.fixed_bytes = L.packed_bytes + L.packed_t_bytes + L.partial_bytes;
  // per band row: G and G^T as hi + lo (8 V1p), H^T as hi + lo (4 Jp), da float32 (4 Jp)
  L.unit_bytes = L.unit_rows * (8 * L.v1p + 8 * L.jp);
  return L;
}

inline size_t rjl_units_for(const rjl_layout& L, size_t bytes) {
  if (bytes < L.fixed_bytes + L.unit_bytes) return 0;
  size_t u = (bytes - L.fixed_bytes) / L.unit_bytes;
  if (u > L.total_units) u = L.total_units;
  if (u > (size_t)RJL_MAX_UNITS) u = RJL_MAX_UNITS;
  return u;
}

// band row -> (n, t, u) and whether its cell contributes: it exists and its utterance's nll is not +inf
struct rjl_cell {
  int n, t, u;
  bool live;
};
__device__ __forceinline__ rjl_cell rjl_cell_of(long row, int q0, int tiles_t, int u1p, const int32_t* in_lens,
                                                const int32_t* tgt_lens, const float* nll, int T, int U1) {
  rjl_cell c;
  const long fr = row / u1p;                          // (unit of the band) 8 + frame
  c.u = (int)(row - fr * u1p);
  const int q = q0 + (int)(fr / RS_TT);
  c.n = q / tiles_t;
  c.t = (q - c.n * tiles_t) * RS_TT + (int)(fr % RS_TT);
  const int Tn = in_lens[c.n], Un = tgt_lens[c.n];
  c.live = ms::rl_lens_ok(Tn, Un, T, U1) && c.t < Tn && c.u <= Un && fabsf(nll[c.n]) != INFINITY;
  return c;
}

// one thread per (j, band row), rows fastest
__global__ __launch_bounds__(256) void rjl_h_kernel(const float* __restrict__ enc_p, const float* __restrict__ pred_p,
                                                    const int32_t* __restrict__ in_lens, const int32_t* __restrict__ tgt_lens,
                                                    const float* __restrict__ nll, unsigned short* __restrict__ ht_hi,
                                                    unsigned short* __restrict__ ht_lo, int N, int T, int U1, int J, int q0,
                                                    int tiles_t, int u1p, long rows_b, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long j = i / rows_b, row = i - j * rows_b;
  unsigned hi = 0, lo = 0;
  if (j < J) {
    const rjl_cell c = rjl_cell_of(row, q0, tiles_t, u1p, in_lens, tgt_lens, nll, T, U1);
    if (c.live)
      ms::plane_split_bounded<true>(rs_tanh(enc_p[((size_t)c.t * N + c.n) * J + j] + pred_p[((size_t)c.u * N + c.n) * J + j]), hi,
                                    lo);
  }
  ht_hi[i] = (unsigned short)hi;
  ht_lo[i] = (unsigned short)lo;
}

// C = A B^T over fp16 hi + lo planes, f16x3: a workgroup of 4 waves owns 128 rows x 128 columns, a wave 32 rows.  A row-major
// [rows][lda] (halves), the lane's 8 consecutive k straight from global memory.
__device__ __forceinline__ void rjl_mma_step(const u32x4_ ah, const u32x4_ al, const u32x4_ bh, const u32x4_ bl, f32x16& acc) {
  acc = ms::mfma_32x32x16<true>(al, bh, acc);
  acc = ms::mfma_32x32x16<true>(ah, bl, acc);
  acc = ms::mfma_32x32x16<true>(ah, bh, acc);
}

// da[row, j] = (sum_v G[row, v] w_out[v, j]) / 2^12 * (1 - h^2); grid (rows / 128, Jp / 128)
__global__ __launch_bounds__(256) void rjl_dh_kernel(const unsigned short* __restrict__ g_hi, const unsigned short* __restrict__ g_lo,
                                                     const u32x4_* __restrict__ packed_t, const float* __restrict__ enc_p,
                                                     const float* __restrict__ pred_p, const int32_t* __restrict__ in_lens,
                                                     const int32_t* __restrict__ tgt_lens, const float* __restrict__ nll,
                                                     float* __restrict__ da, int N, int T, int U1, int J, int q0, int tiles_t,
                                                     int u1p, int v1p, int k_steps, int jp) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const long row0 = (long)blockIdx.x * 128 + 32 * w;
  const int ct = blockIdx.y;
  const u32x4_* a_hi = reinterpret_cast<const u32x4_*>(g_hi + (size_t)(row0 + r) * v1p + 8 * h);
  const u32x4_* a_lo = reinterpret_cast<const u32x4_*>(g_lo + (size_t)(row0 + r) * v1p + 8 * h);
  const u32x4_* bt = packed_t + ((size_t)ct * 4 * k_steps) * 128 + lane;
  f32x16 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
  for (int ks = 0; ks < k_steps; ++ks) {
    const u32x4_ ah = a_hi[2 * ks], al = a_lo[2 * ks];          // 16 halves = 2 x 16 bytes per K step
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const u32x4_* bp = bt + ((size_t)cb * k_steps + ks) * 128;
      rjl_mma_step(ah, al, bp[0], bp[64], acc[cb]);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long row = row0 + ms::mfma32_row(i, lane);
    const rjl_cell c = rjl_cell_of(row, q0, tiles_t, u1p, in_lens, tgt_lens, nll, T, U1);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int j = ct * 128 + 32 * cb + r;
      float val = 0.f;
      if (c.live && j < J) {
        const float hh = rs_tanh(enc_p[((size_t)c.t * N + c.n) * J + j] + pred_p[((size_t)c.u * N + c.n) * J + j]);
        val = acc[cb][i] * (1.f / ms::RS_G_SCALE) * (1.f - hh * hh);
      }
      da[(size_t)row * jp + j] = val;
    }
  }
}

// d_enc_p[t, n, j] = sum_u da; one thread per (frame of the band, j)
__global__ __launch_bounds__(256) void rjl_enc_kernel(const float* __restrict__ da, float* __restrict__ d_enc_p, int N, int T,
                                                      int J, int q0, int tiles_t, int u1p, int jp, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long fr = i / J;
  const int j = (int)(i - fr * J);
  const int q = q0 + (int)(fr / RS_TT);
  const int n = q / tiles_t, t = (q - n * tiles_t) * RS_TT + (int)(fr % RS_TT);
  if (t >= T) return;
  const float* p = da + (size_t)fr * u1p * jp + j;
  float s = 0.f;
  for (int u = 0; u < u1p; ++u) s += p[(size_t)u * jp];
  d_enc_p[((size_t)t * N + n) * J + j] = s;
}

// d_pred_p[u, n, j] (+)= sum over the band's frames of n; one thread per (utterance of the band, u, j)
__global__ __launch_bounds__(256) void rjl_pred_kernel(const float* __restrict__ da, float* __restrict__ d_pred_p, int N, int U1,
                                                       int J, int q0, int units, int tiles_t, int u1p, int jp, int n_first,
                                                       long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long nu = i / J;
  const int j = (int)(i - nu * J);
  const int n = n_first + (int)(nu / U1), u = (int)(nu % U1);
  const int qa = max(q0, n * tiles_t), qb = min(q0 + units, (n + 1) * tiles_t);
  float s = 0.f;
  for (int q = qa; q < qb; ++q)
    for (int tt = 0; tt < RS_TT; ++tt) s += da[((size_t)((q - q0) * RS_TT + tt) * u1p + u) * jp + j];
  float* o = d_pred_p + ((size_t)u * N + n) * J + j;
  *o = (qa == n * tiles_t) ? s : *o + s;              // the utterance's first frames: this band writes the row
}

// partial[z][v, j] = sum over the rows of chunk z of G^T[v, row] H^T[j, row]; grid (V1p / 128, Jp / 128, chunks)
__global__ __launch_bounds__(256) void rjl_dw_kernel(const unsigned short* __restrict__ gt_hi, const unsigned short* __restrict__ gt_lo,
                                                     const unsigned short* __restrict__ ht_hi, const unsigned short* __restrict__ ht_lo,
                                                     float* __restrict__ partial, int v1p, int jp, long rows_b, long chunk_rows) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int v0 = blockIdx.x * 128 + 32 * w, j0 = blockIdx.y * 128;
  const long k_begin = (long)blockIdx.z * chunk_rows, k_end = min(rows_b, k_begin + chunk_rows);
  const u32x4_* a_hi = reinterpret_cast<const u32x4_*>(gt_hi + (size_t)(v0 + r) * rows_b + k_begin + 8 * h);
  const u32x4_* a_lo = reinterpret_cast<const u32x4_*>(gt_lo + (size_t)(v0 + r) * rows_b + k_begin + 8 * h);
  const u32x4_* b_hi[4];
  const u32x4_* b_lo[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    b_hi[cb] = reinterpret_cast<const u32x4_*>(ht_hi + (size_t)(j0 + 32 * cb + r) * rows_b + k_begin + 8 * h);
    b_lo[cb] = reinterpret_cast<const u32x4_*>(ht_lo + (size_t)(j0 + 32 * cb + r) * rows_b + k_begin + 8 * h);
  }
  f32x16 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
  const long k_steps = (k_end - k_begin) / 16;         // (chunks are multiples of 128 rows, and so is the band)
  for (long ks = 0; ks < k_steps; ++ks) {
    const u32x4_ ah = a_hi[2 * ks], al = a_lo[2 * ks];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) rjl_mma_step(ah, al, b_hi[cb][2 * ks], b_lo[cb][2 * ks], acc[cb]);
  }
  float* out = partial + (size_t)blockIdx.z * v1p * jp;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int v = v0 + ms::mfma32_row(i, lane);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) out[(size_t)v * jp + j0 + 32 * cb + r] = acc[cb][i];
  }
}

// d_w_out[v, j] (+)= (partial[0] + partial[1] + ...)[v, j] / 2^12; one thread per element
__global__ __launch_bounds__(256) void rjl_dw_reduce_kernel(const float* __restrict__ partial, float* __restrict__ d_w_out, int J,
                                                            int v1p, int jp, int chunks, int accumulate, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long v = i / J;
  const int j = (int)(i - v * J);
  float s = 0.f;
  for (int z = 0; z < chunks; ++z) s += partial[((size_t)z * v1p + v) * jp + j];
  s *= 1.f / ms::RS_G_SCALE;
  d_w_out[i] = accumulate ? d_w_out[i] + s : s;
}

// d_b_out[v] (+)= (sum_rows G^T[v, row]) / 2^12; one workgroup per symbol, threads over the rows, merged in a fixed order
__global__ __launch_bounds__(256) void rjl_db_kernel(const unsigned short* __restrict__ gt_hi, const unsigned short* __restrict__ gt_lo,
                                                     float* __restrict__ d_b_out, long rows_b, int accumulate) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int v = blockIdx.x;
  const unsigned short* ph = gt_hi + (size_t)v * rows_b;
  const unsigned short* pl = gt_lo + (size_t)v * rows_b;
  float s = 0.f;
  for (long k = tid; k < rows_b; k += 256) s += ms::plane_val<true>(ph[k]) + ms::plane_val<true>(pl[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    const float val = ((part[0] + part[1]) + (part[2] + part[3])) * (1.f / ms::RS_G_SCALE);
    d_b_out[v] = accumulate ? d_b_out[v] + val : val;
  }
}

}  // namespace

extern "C" size_t ms_rnnt_joint_loss_lattice_bytes(int N, int T, int U1) {
  if (N <= 0 || T <= 0 || U1 <= 0) return 0;
  return (size_t)3 * N * T * U1 * sizeof(float);
}

extern "C" int ms_rnnt_joint_loss_forward(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                                          const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* nll,
                                          float* lattice, int N, int T, int U1, int J, int V1, int blank, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && J > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(enc_p && pred_p && w_out && in_lens && tgt_lens && nll && lattice && workspace, "null pointer");
  MS_REQUIRE(targets || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  MS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (!ms::rnnt_score_supported(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_joint_loss_forward: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_score_workspace_bytes(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_joint_loss_forward: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  const size_t plane = (size_t)N * T * U1;
  return ms::rnnt_score_launch(enc_p, pred_p, w_out, b_out, in_lens, targets, tgt_lens, nll, lattice, lattice + plane,
                               lattice + 2 * plane, N, T, U1, J, V1, blank, workspace, (hipStream_t)stream);
}

extern "C" size_t ms_rnnt_joint_loss_backward_workspace_min_bytes(int N, int T, int U1, int J, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V1 <= 0) return 0;
  const rjl_layout L = rjl_make_layout(N, T, U1, J, V1);
  return L.fixed_bytes + L.unit_bytes;
}

extern "C" size_t ms_rnnt_joint_loss_backward_workspace_bytes(int N, int T, int U1, int J, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V1 <= 0) return 0;
  const rjl_layout L = rjl_make_layout(N, T, U1, J, V1);
  size_t units = rjl_units_for(L, RJL_PREFERRED);
  if (units == 0) units = 1;                         // a single unit is already larger: the minimum
  return L.fixed_bytes + units * L.unit_bytes;
}

extern "C" int ms_rnnt_joint_loss_backward(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                                           const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                                           const float* nll, const float* lattice, const float* grad_nll, float* d_enc_p,
                                           float* d_pred_p, float* d_w_out, float* d_b_out, int N, int T, int U1, int J, int V1,
                                           int blank, void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && J > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(enc_p && pred_p && w_out && in_lens && tgt_lens && nll && lattice && grad_nll && d_enc_p && d_pred_p && d_w_out &&
                 workspace,
             "null pointer");
  MS_REQUIRE(targets || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  MS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  const rjl_layout L = rjl_make_layout(N, T, U1, J, V1);
  const long pack_t_threads = (long)(rs_col_blocks(J) * rs_k_steps(V1) * 64);
  if (!ms::rnnt_score_supported(N, T, U1, J, V1) || (pack_t_threads + 255) / 256 > 0x7fffffffL || L.total_units > 0x7fffffffUL ||
      L.v1p / 128 > 65535 || L.jp / 128 > 65535) {
    ms::set_error("ms_rnnt_joint_loss_backward: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  const size_t band_units = rjl_units_for(L, workspace_bytes);
  if (band_units == 0) {
    ms::set_error("ms_rnnt_joint_loss_backward: workspace below ms_rnnt_joint_loss_backward_workspace_min_bytes");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t rows_max = band_units * L.unit_rows;
  char* p = (char*)workspace;
  u32x4_* packed = (u32x4_*)p;
  p += L.packed_bytes;
  u32x4_* packed_t = (u32x4_*)p;
  p += L.packed_t_bytes;
  float* partial = (float*)p;
  p += L.partial_bytes;
  // (every plane is a multiple of 256 bytes: rows are multiples of 128, V1p and Jp as well)
  unsigned short* g_hi = (unsigned short*)p;
  unsigned short* g_lo = g_hi + rows_max * L.v1p;
  unsigned short* gt_hi = g_lo + rows_max * L.v1p;
  unsigned short* gt_lo = gt_hi + rows_max * L.v1p;
  unsigned short* ht_hi = gt_lo + rows_max * L.v1p;
  unsigned short* ht_lo = ht_hi + rows_max * L.jp;
  float* da = (float*)(ht_lo + rows_max * L.jp);

  const int k_steps_j = (int)rs_k_steps(J), k_steps_v = (int)rs_k_steps(V1);
  const long pack_threads = (long)(rs_col_blocks(V1) * rs_k_steps(J) * 64);
  hipLaunchKernelGGL(rnnt_score_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, st, w_out, packed, J,
                     V1, k_steps_j, pack_threads, (long)J, 1L);
  MS_LAUNCH_CHECK();
  // the transpose: rows j, K = v
  hipLaunchKernelGGL(rnnt_score_pack_kernel, dim3((unsigned)((pack_t_threads + 255) / 256)), dim3(256), 0, st, w_out, packed_t,
                     V1, J, k_steps_v, pack_t_threads, 1L, (long)J);
  MS_LAUNCH_CHECK();

  const size_t plane = (size_t)N * T * U1;
  const int tiles_t = (int)L.tiles_t, tiles_u = (int)L.tiles_u, u1p = (int)L.u1p, v1p = (int)L.v1p, jp = (int)L.jp;
  int band = 0;
  for (size_t q0 = 0; q0 < L.total_units; q0 += band_units, ++band) {
    const int units = (int)(L.total_units - q0 < band_units ? L.total_units - q0 : band_units);
    const long rows_b = (long)units * (long)L.unit_rows;
    // the band's planes are laid out for ITS rows (the transposed ones have the rows as their inner extent)
    const long h_total = rows_b * jp;
    hipLaunchKernelGGL(rjl_h_kernel, dim3((unsigned)((h_total + 255) / 256)), dim3(256), 0, st, enc_p, pred_p, in_lens, tgt_lens,
                       nll, ht_hi, ht_lo, N, T, U1, J, (int)q0, tiles_t, u1p, rows_b, h_total);
    MS_LAUNCH_CHECK();
    rs_emit_args em;
    em.nll = nll;
    em.Z = lattice;
    em.alpha = lattice + plane;
    em.beta = lattice + 2 * plane;
    em.grad_nll = grad_nll;
    em.g_hi = g_hi;
    em.g_lo = g_lo;
    em.gt_hi = gt_hi;
    em.gt_lo = gt_lo;
    em.q0 = (int)q0;
    em.rows_b = (int)rows_b;
    em.v1p = v1p;
    hipLaunchKernelGGL((rnnt_score_cells_kernel<4, true>), dim3((unsigned)(units * tiles_u), (unsigned)(v1p / 128)),
                       dim3(RS_THREADS), 0, st, enc_p, pred_p, packed, b_out, in_lens, targets, tgt_lens, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, N, T, U1, J, V1, blank, tiles_t, tiles_u, em);
    MS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rjl_dh_kernel, dim3((unsigned)(rows_b / 128), (unsigned)(jp / 128)), dim3(256), 0, st, g_hi, g_lo, packed_t,
                       enc_p, pred_p, in_lens, tgt_lens, nll, da, N, T, U1, J, (int)q0, tiles_t, u1p, v1p, k_steps_v, jp);
    MS_LAUNCH_CHECK();
    const long enc_total = (long)units * RS_TT * J;
    hipLaunchKernelGGL(rjl_enc_kernel, dim3((unsigned)((enc_total + 255) / 256)), dim3(256), 0, st, da, d_enc_p, N, T, J, (int)q0,
                       tiles_t, u1p, jp, enc_total);
    MS_LAUNCH_CHECK();
    const int n_first = (int)(q0 / L.tiles_t), n_last = (int)((q0 + units - 1) / L.tiles_t);
    const long pred_total = (long)(n_last - n_first + 1) * U1 * J;
    hipLaunchKernelGGL(rjl_pred_kernel, dim3((unsigned)((pred_total + 255) / 256)), dim3(256), 0, st, da, d_pred_p, N, U1, J,
                       (int)q0, units, tiles_t, u1p, jp, n_first, pred_total);
    MS_LAUNCH_CHECK();
    // chunks of whole 128 rows, at most dw_splits of them
    const long chunk_rows = (long)((rows_b / 128 + (long)L.dw_splits - 1) / (long)L.dw_splits) * 128;
    const int chunks = (int)((rows_b + chunk_rows - 1) / chunk_rows);
    hipLaunchKernelGGL(rjl_dw_kernel, dim3((unsigned)(v1p / 128), (unsigned)(jp / 128), (unsigned)chunks), dim3(256), 0, st, gt_hi,
                       gt_lo, ht_hi, ht_lo, partial, v1p, jp, rows_b, chunk_rows);
    MS_LAUNCH_CHECK();
    const long dw_total = (long)V1 * J;
    hipLaunchKernelGGL(rjl_dw_reduce_kernel, dim3((unsigned)((dw_total + 255) / 256)), dim3(256), 0, st, partial, d_w_out, J, v1p,
                       jp, chunks, band > 0, dw_total);
    MS_LAUNCH_CHECK();
    if (d_b_out) {
      hipLaunchKernelGGL(rjl_db_kernel, dim3((unsigned)V1), dim3(256), 0, st, gt_hi, gt_lo, d_b_out, rows_b, band > 0);
      MS_LAUNCH_CHECK();
    }
  }
  return MS_OK;
}
