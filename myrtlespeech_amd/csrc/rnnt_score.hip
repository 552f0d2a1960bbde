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
//
// The kernels live in rnnt_score.h: the fused loss (rnnt_joint_loss.hip) runs the same launches with a Z plane for its
// forward, and the cells kernel's mainloop under another epilogue for its backward.
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"
#include "rnnt_score.h"

using ms::rs_col_blocks;
using ms::rs_k_steps;
using ms::rs_packed_bytes;

int ms::rnnt_score_cells_launch(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                                const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* Z, int N, int T,
                                int U1, int J, int V1, int blank, void* workspace, hipStream_t st) {
  const int tiles_t = ms::cdiv(T, RS_TT), tiles_u = ms::cdiv(U1, RS_TU);
  const long tiles = (long)N * tiles_t * tiles_u;
  const long pack_threads = (long)(rs_col_blocks(V1) * rs_k_steps(J) * 64);
  const size_t plane_bytes = ms::rl_skew_plane_bytes(N, T, U1);
  float* b_sk = (float*)workspace;
  float* e_sk = (float*)((char*)workspace + plane_bytes);
  u32x4_* packed = (u32x4_*)((char*)workspace + 2 * plane_bytes);
  const int k_steps = (int)rs_k_steps(J);
  hipLaunchKernelGGL(rnnt_score_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, st, w_out, packed, J,
                     V1, k_steps, pack_threads, (long)J, 1L);
  MS_LAUNCH_CHECK();
  const dim3 grid((unsigned)tiles), block(RS_THREADS);
#define RS_CELLS(NB)                                                                                                      \
  hipLaunchKernelGGL((rnnt_score_cells_kernel<NB, false>), grid, block, 0, st, enc_p, pred_p, packed, b_out, in_lens,     \
                     targets, tgt_lens, b_sk, e_sk, Z, N, T, U1, J, V1, blank, tiles_t, tiles_u, rs_emit_args{})
  if (V1 <= 32) RS_CELLS(1);
  else if (V1 <= 64) RS_CELLS(2);
  else RS_CELLS(4);
#undef RS_CELLS
  MS_LAUNCH_CHECK();
  return MS_OK;
}

int ms::rnnt_score_launch(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out, const int32_t* in_lens,
                          const int32_t* targets, const int32_t* tgt_lens, float* nll, float* Z, float* alpha, float* beta,
                          int N, int T, int U1, int J, int V1, int blank, void* workspace, hipStream_t st) {
  const int rc = ms::rnnt_score_cells_launch(enc_p, pred_p, w_out, b_out, in_lens, targets, tgt_lens, Z, N, T, U1, J, V1, blank,
                                             workspace, st);
  if (rc != MS_OK) return rc;
  const float* b_sk = (const float*)workspace;
  const float* e_sk = (const float*)((const char*)workspace + ms::rl_skew_plane_bytes(N, T, U1));
  return ms::rnnt_lattice_launch(in_lens, targets, tgt_lens, b_sk, e_sk, alpha, beta, nll, N, T, U1, V1, blank, st);
}

bool ms::rnnt_score_supported(int N, int T, int U1, int J, int V1) {
  const long tiles = (long)N * ms::cdiv(T, RS_TT) * ms::cdiv(U1, RS_TU);
  const long pack_threads = (long)(rs_col_blocks(V1) * rs_k_steps(J) * 64);
  return ms::rl_supported(N, T, U1) && tiles <= 0x7fffffffL && (pack_threads + 255) / 256 <= 0x7fffffffL;
}

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
  if (!ms::rnnt_score_supported(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_score: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_score_workspace_bytes(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_score: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  const size_t plane = (size_t)N * T * U1;
  return ms::rnnt_score_launch(enc_p, pred_p, w_out, b_out, in_lens, targets, tgt_lens, nll, nullptr, lattice, lattice + plane, N,
                               T, U1, J, V1, blank, workspace, (hipStream_t)stream);
}
