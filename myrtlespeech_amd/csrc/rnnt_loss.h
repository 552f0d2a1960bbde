// What the transducer loss (rnnt_loss.hip), the fused scorer (rnnt_score.hip) and the forced aligner (rnnt_align.hip) share:
// the layout of the two skewed planes b = lp(blank), e = lp(y_u), the tests on lengths and labels, the supported shapes, and
// the launches of the normaliser and the lattice pass.
#pragma once
#include <math.h>

#include "common.h"

namespace ms {

constexpr int RL_MAX_U1 = 1024;        // one thread per u: a workgroup

__device__ __forceinline__ float rl_neg_inf() { return -INFINITY; }
__device__ __forceinline__ float rl_nan() { return __uint_as_float(0x7fc00000u); }

// rows of a skewed plane [n][t + u][u]
__host__ __device__ __forceinline__ size_t rl_skew_rows(int T, int U1) { return (size_t)T + U1 - 1; }
// bytes of one skewed plane, rounded as the workspaces lay them out
static inline size_t rl_skew_plane_bytes(int N, int T, int U1) {
  return align_up((size_t)N * rl_skew_rows(T, U1) * U1 * sizeof(float), 256);
}

// the caller's error otherwise: such an utterance has no cells, nll = +inf and a zero gradient
__device__ __forceinline__ bool rl_lens_ok(int Tn, int Un, int T, int U1) { return Tn >= 1 && Tn <= T && Un >= 0 && Un <= U1 - 1; }

__device__ __forceinline__ bool rl_label_ok(int lab, int V1, int blank) { return lab >= 0 && lab < V1 && lab != blank; }

// MS_ERR_UNSUPPORTED past the shapes the kernels serve (U1 <= 1024; a row-pass grid that fits 31 bits)
static inline bool rl_supported(int N, int T, int U1) {
  if (U1 > RL_MAX_U1) return false;
  const long R = (long)N * T * U1;
  return (R + 3) / 4 <= 0x7fffffffL && (long)N * 2 <= 0x7fffffffL;
}

// The lattice pass (rnnt_loss_lattice_kernel, 2 N workgroups) over two skewed planes: alpha, beta [N, T, U1] and nll [N].
// Enqueues on `st`; MS_OK or MS_ERR_HIP.
int rnnt_lattice_launch(const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, const float* b_sk,
                        const float* e_sk, float* alpha, float* beta, float* nll, int N, int T, int U1, int V1, int blank,
                        hipStream_t st);

// The normaliser pass (rnnt_loss_normalise_kernel) alone: Z [N, T, U1] and the two skewed planes from logits [N, T, U1, V1].
// What ms_rnnt_loss_forward launches first; ms_rnnt_align (rnnt_align.hip) runs it with Z in workspace scratch.
// Enqueues on `st`; MS_OK or MS_ERR_HIP.
int rnnt_normalise_launch(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* Z,
                          float* b_sk, float* e_sk, int N, int T, int U1, int V1, int blank, hipStream_t st);

}  // namespace ms
