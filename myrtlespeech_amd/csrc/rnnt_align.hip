// Transducer (RNN-T) forced alignment: the Viterbi (max-plus) twin of rnnt_loss.hip's lattice pass, with back-pointers, the
// back-trace and the read-out on the device.  OWN specification (the reference snapshot has no transducer): the comment on
// ms_rnnt_align in include/ms_hotpath.h; tests/rnnt_align_ref.py restates it in numpy.  No MFMA of its own: a scan kernel,
// one workgroup per utterance, on the two skewed planes b = lp(blank), e = lp(y_u) that
//   ms_rnnt_align        flags = 0                     rnnt_loss.hip's normaliser pass (ms::rnnt_normalise_launch), or
//                        flags = MS_RNNT_LOG_PROBS_IN  rnnt_align_gather_kernel below: the two values of a cell as given
//   ms_rnnt_align_joint                                rnnt_score.hip's pack and cells launches (ms::rnnt_score_cells_launch)
// leave in the workspace.
//
//   rnnt_align_kernel   one thread per u, walking the anti-diagonals d = t + u like rnnt_loss_lattice_kernel: d(t-1, u) + b
//                       is the thread's own previous value, d(t, u-1) + e its neighbour's -- a wave shuffle inside a wave, one
//                       LDS word per wave boundary (double-buffered by the parity of d: ONE barrier per diagonal, none when
//                       U1 <= 64); the next diagonal's b / e are loaded before the barrier, which waits for the LDS only.
//                       d lives in registers: there is no alpha / beta lattice.  The back-pointer of a cell is one bit (0: the
//                       blank predecessor, 1: the label predecessor); a wave's 64 of a diagonal are one __ballot word, row d
//                       of the back-pointer table is ceil(U1 / 64) words.  The rows sit in LDS when T + U1 - 1 of them fit
//                       RA_BP_LDS_BYTES, else in the global workspace.  After the walk one lane walks the bits back from
//                       (T_n-1, U_n) -- T_n + U_n - 1 dependent reads, LDS or L2 -- and leaves token_frame / frame_u; the
//                       workgroup then reads the path's log-probabilities out of the planes in parallel and fills the rows
//                       that do not exist.
//
// No workgroup waits on another: no atomics, no spin, no status word; the same inputs give the same bits.
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"
#define RNNT_SCORE_DECLARATIONS_ONLY   // the launches of the scorer, not its kernels
#include "rnnt_score.h"

namespace {

using ms::RL_MAX_U1;
using ms::rl_label_ok;
using ms::rl_lens_ok;
using ms::rl_nan;
using ms::rl_neg_inf;
using ms::rl_skew_rows;

typedef unsigned long long u64;

constexpr size_t RA_BP_LDS_BYTES = 96 * 1024;    // back-pointer rows kept in LDS up to this size (MS_RNNT_ALIGN_BP_LDS_BYTES)
static_assert(RA_BP_LDS_BYTES == MS_RNNT_ALIGN_BP_LDS_BYTES, "the header documents the budget");
constexpr size_t RA_LDS_MAX = 160 * 1024 - 1024; // dynamic LDS of a launch (the kernel keeps a few static words)
static_assert(RA_BP_LDS_BYTES <= RA_LDS_MAX, "LDS of a CU");

inline int ra_waves(int U1) { return ms::cdiv(U1, 64); }
// bytes of one utterance's back-pointer rows: [T + U1 - 1][ceil(U1 / 64)] u64
inline size_t ra_bp_bytes(int T, int U1) { return rl_skew_rows(T, U1) * (size_t)ra_waves(U1) * sizeof(u64); }
inline bool ra_bp_in_lds(int T, int U1) { return ra_bp_bytes(T, U1) <= RA_BP_LDS_BYTES; }
inline size_t ra_bp_ws_bytes(int N, int T, int U1) { return ra_bp_in_lds(T, U1) ? 0 : ms::align_up((size_t)N * ra_bp_bytes(T, U1), 256); }

__device__ __forceinline__ bool ra_poison(float v) { return v != v || v == INFINITY; }

// One thread per cell (n, t, u) of [N, T, U1]: x[n, t, u, blank] and x[n, t, u, y_u] of an existing cell into the skewed
// planes, exactly as given; a NaN or +inf in either marks the cell (NaN in both planes, as the normaliser pass leaves a
// cell whose Z is not finite).
__global__ __launch_bounds__(256) void rnnt_align_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ in_lens,
                                                                const int32_t* __restrict__ targets,
                                                                const int32_t* __restrict__ tgt_lens, float* __restrict__ b_sk,
                                                                float* __restrict__ e_sk, long R, int T, int U1, int V1,
                                                                int blank) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const long q = r / U1;
  const int u = (int)(r - q * U1);
  const int n = (int)(q / T);
  const int t = (int)(q - (long)n * T);
  const int Tn = in_lens[n], Un = tgt_lens[n];
  if (!rl_lens_ok(Tn, Un, T, U1) || t >= Tn || u > Un) return;
  const float* row = x + (size_t)r * V1;
  float bv = row[blank];
  float ev = rl_neg_inf();
  if (u < Un) {
    const int lab = targets[(size_t)n * (U1 - 1) + u];
    if (rl_label_ok(lab, V1, blank)) ev = row[lab];   // (else: the walk reports the utterance)
  }
  if (ra_poison(bv) || ra_poison(ev)) bv = ev = rl_nan();
  const size_t o = ((size_t)n * rl_skew_rows(T, U1) + (size_t)(t + u)) * U1 + u;
  b_sk[o] = bv;
  e_sk[o] = ev;
}

// barrier that waits for this wave's LDS operations only (rnnt_loss_lattice_kernel): __syncthreads() would also wait for the
// loads just issued for the next diagonal
__device__ __forceinline__ void ra_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// An utterance without a path: every integer output -1; the log-probabilities of its own frames / labels `sc` (-inf or NaN), 0
// beyond them.  Tc, Uc: its lengths clamped to the shapes.
__device__ __forceinline__ void ra_write_no_path(float sc, int n, int tid, int nthreads, int Tc, int Uc, int T, int U1,
                                                 float* score, int32_t* token_frame, float* token_logp, int32_t* frame_u,
                                                 float* frame_logp) {
  if (tid == 0) score[n] = sc;
  for (int t = tid; t < T; t += nthreads) {
    frame_u[(size_t)n * T + t] = -1;
    frame_logp[(size_t)n * T + t] = t < Tc ? sc : 0.f;
  }
  for (int u = tid; u < U1 - 1; u += nthreads) {
    token_frame[(size_t)n * (U1 - 1) + u] = -1;
    token_logp[(size_t)n * (U1 - 1) + u] = u < Uc ? sc : 0.f;
  }
}

// blockIdx.x = n; blockDim.x = U1 rounded up to whole waves; MULTI: more than one wave; BP_LDS: the back-pointer rows
// [T + U1 - 1][waves] u64 are the dynamic LDS, else they are this utterance's slice of bp_ws
template <bool MULTI, bool BP_LDS>
__global__ __launch_bounds__(RL_MAX_U1) void rnnt_align_kernel(
    const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets, const int32_t* __restrict__ tgt_lens,
    const float* __restrict__ b_sk, const float* __restrict__ e_sk, u64* __restrict__ bp_ws, float* __restrict__ score,
    int32_t* token_frame, float* __restrict__ token_logp, int32_t* frame_u, float* __restrict__ frame_logp, int T, int U1,
    int V1, int blank) {   // (token_frame / frame_u: written by the back-trace, read back by the read-out)
  extern __shared__ __attribute__((aligned(16))) unsigned char ra_smem[];
  __shared__ float xch[2][RL_MAX_U1 / 64];        // [parity of d][wave]: the value that crosses a wave boundary
  __shared__ int fin[2];                          // the score's bits; 1 when the utterance has a path
  const int n = blockIdx.x;
  const int u = threadIdx.x, lane = u & 63, w = u >> 6;
  const int nthreads = blockDim.x, W = nthreads >> 6;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  const int Tc = min(max(Tn, 0), T), Uc = min(max(Un, 0), U1 - 1);
  int invalid = rl_lens_ok(Tn, Un, T, U1) ? 0 : 1;
  if (!invalid && u < Un && !rl_label_ok(targets[(size_t)n * (U1 - 1) + u], V1, blank)) invalid = 1;
  if (MULTI) {
    if (u < 2 * (RL_MAX_U1 / 64)) (&xch[0][0])[u] = rl_neg_inf();
    invalid = __syncthreads_or(invalid);          // (also: the -inf above are in place)
  } else {
    invalid = __ballot(invalid != 0) != 0ull;
  }
  if (invalid) {                                  // the caller's error: no cell is read
    ra_write_no_path(rl_neg_inf(), n, u, nthreads, Tc, Uc, T, U1, score, token_frame, token_logp, frame_u, frame_logp);
    return;
  }
  u64* bp = BP_LDS ? reinterpret_cast<u64*>(ra_smem) : bp_ws + (size_t)n * rl_skew_rows(T, U1) * W;
  const int D = Tn + Un;                          // anti-diagonals 0 .. D - 1; D <= T + U1 - 1 rows of the skewed planes
  const int uu = min(u, U1 - 1);                  // (threads past U1 load an in-bounds word they never use)
  const size_t plane0 = (size_t)n * rl_skew_rows(T, U1) * U1;
  const float* bs = b_sk + plane0 + uu;
  const float* es = e_sk + plane0 + uu;
  const bool has_e = u < Un;
  // `own` is d(t-1, u) + b(t-1, u), `pass` (handed to thread u + 1) is d(t, u) + e(t, u); d(0, 0) = 0 comes out of a virtual
  // blank predecessor 0 -- its back-pointer bit is 0 and is never followed.
  float own = (u == 0) ? 0.f : rl_neg_inf();
  float pass = rl_neg_inf();
  int bad = 0;                                    // a NaN or +inf b / e in an existing cell of this thread's column
  float b_next = bs[0], e_next = es[0];
  for (int d = 0; d < D; ++d) {
    const int t = d - u;
    const bool valid = u <= Un && t >= 0 && t < Tn;
    const float bc = valid ? b_next : rl_neg_inf();
    const float ec = (valid && has_e) ? e_next : rl_neg_inf();
    if (d + 1 < D) {                              // the next diagonal's values: in flight across the barrier
      b_next = bs[(size_t)(d + 1) * U1];
      e_next = es[(size_t)(d + 1) * U1];
    }
    bad |= (ra_poison(bc) || ra_poison(ec)) ? 1 : 0;
    float nb = __shfl_up(pass, 1, 64);
    if (lane == 0) nb = (MULTI && w > 0) ? xch[(d + 1) & 1][w - 1] : rl_neg_inf();
    // a tie takes the blank predecessor; in frame 0 there is none
    const bool k = valid && u >= 1 && (t == 0 || nb > own);
    const float v = valid ? (k ? nb : own) : rl_neg_inf();
    own = v + bc;
    pass = v + ec;
    const u64 word = __ballot(k);
    if (lane == 0) bp[(size_t)d * W + w] = word;
    if (MULTI) {
      if (lane == 63) xch[d & 1][w] = pass;
      ra_lds_barrier();
    }
  }
  // own of thread U_n = d(T_n-1, U_n) + b(T_n-1, U_n): the score
  if (MULTI) {
    bad = __syncthreads_or(bad);                  // (also: the back-pointer rows are visible to the lane that walks them)
  } else {
    bad = __ballot(bad != 0) != 0ull;
    __syncthreads();
  }
  if (u == Un) {
    const float sc = bad ? rl_nan() : own;
    fin[0] = __float_as_int(sc);
    fin[1] = (!bad && sc != rl_neg_inf()) ? 1 : 0;
  }
  __syncthreads();
  const float sc = __int_as_float(fin[0]);
  if (!fin[1]) {
    ra_write_no_path(sc, n, u, nthreads, Tc, Uc, T, U1, score, token_frame, token_logp, frame_u, frame_logp);
    return;
  }
  int32_t* tf = token_frame + (size_t)n * (U1 - 1);
  int32_t* fu = frame_u + (size_t)n * T;
  if (u == 0) {
    // back-trace: D - 1 steps from (T_n-1, U_n) to (0, 0).  On a finite path the bits keep (t, u) inside the lattice; the two
    // borders are enforced all the same, so that no index can leave it.
    score[n] = sc;
    int t = Tn - 1, c = Un;
    fu[t] = c;                                    // the final blank
#ifdef RA_PROBE_NO_BACKTRACE
    // MEASUREMENT BUILD ONLY (tools/rnnt_align_time.py --probe-lib): the same walk and read-out without the serial chain --
    // the path is not traced (every label "emitted" in frame 0), wrong results
    for (int i = 0; i < Tn - 1; ++i) fu[i] = Un;
    for (int i = 0; i < Un; ++i) tf[i] = 0;
#else
    for (int i = 0; i < D - 1; ++i) {
      const u64 word = bp[(size_t)(t + c) * W + (c >> 6)];
      const bool k = t == 0 || (c > 0 && ((word >> (c & 63)) & 1ull));
      if (k) {
        --c;
        tf[c] = t;                                // label c is emitted in frame t: (t, c) -> (t, c + 1)
      } else {
        --t;
        fu[t] = c;                                // the blank of frame t is taken at c
      }
    }
#endif
  }
  __syncthreads();                                // (also: token_frame / frame_u of the path are visible to the workgroup)
  for (int t = u; t < T; t += nthreads) {
    float lp = 0.f;
    if (t < Tn) {
      const int c = fu[t];
      lp = b_sk[plane0 + (size_t)(t + c) * U1 + c];
    } else {
      fu[t] = -1;
    }
    frame_logp[(size_t)n * T + t] = lp;
  }
  for (int c = u; c < U1 - 1; c += nthreads) {
    float lp = 0.f;
    if (c < Un) {
      const int t = tf[c];
      lp = e_sk[plane0 + (size_t)(t + c) * U1 + c];
    } else {
      tf[c] = -1;
    }
    token_logp[(size_t)n * (U1 - 1) + c] = lp;
  }
}

int ra_launch(const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, const float* b_sk, const float* e_sk,
              u64* bp_ws, float* score, int32_t* token_frame, float* token_logp, int32_t* frame_u, float* frame_logp, int N, int T,
              int U1, int V1, int blank, hipStream_t st) {
  static ms::DeviceOnce attr_once;
  if (attr_once.need()) {
    MS_HIP(hipFuncSetAttribute((const void*)rnnt_align_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RA_LDS_MAX));
    MS_HIP(hipFuncSetAttribute((const void*)rnnt_align_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RA_LDS_MAX));
    attr_once.done();
  }
  const int threads = ra_waves(U1) * 64;
  const bool in_lds = ra_bp_in_lds(T, U1);
  const size_t lds = in_lds ? ra_bp_bytes(T, U1) : 0;
#define RA_WALK(MULTI, BP_LDS)                                                                                            \
  hipLaunchKernelGGL((rnnt_align_kernel<MULTI, BP_LDS>), dim3(N), dim3(threads), lds, st, in_lens, targets, tgt_lens, b_sk, \
                     e_sk, bp_ws, score, token_frame, token_logp, frame_u, frame_logp, T, U1, V1, blank)
  if (threads > 64) {
    if (in_lds) RA_WALK(true, true);
    else RA_WALK(true, false);
  } else {
    if (in_lds) RA_WALK(false, true);
    else RA_WALK(false, false);
  }
#undef RA_WALK
  MS_LAUNCH_CHECK();
  return MS_OK;
}

}  // namespace

extern "C" size_t ms_rnnt_align_workspace_bytes(int N, int T, int U1, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || V1 <= 0) return 0;
  // the b and the e plane, skewed; the normalisers' Z [N, T, U1] (scratch of the logits mode); + the back-pointer rows
  // [N][T + U1 - 1][ceil(U1 / 64)] u64 when they do not fit the LDS budget
  return 2 * ms::rl_skew_plane_bytes(N, T, U1) + ms::align_up((size_t)N * T * U1 * sizeof(float), 256) + ra_bp_ws_bytes(N, T, U1);
}

extern "C" int ms_rnnt_align(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                             float* score, int32_t* token_frame, float* token_logp, int32_t* frame_u, float* frame_logp, int N,
                             int T, int U1, int V1, int blank, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(logits && in_lens && tgt_lens && score && frame_u && frame_logp && workspace, "null pointer");
  MS_REQUIRE((targets && token_frame && token_logp) || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  MS_REQUIRE(flags == 0 || flags == MS_RNNT_LOG_PROBS_IN, "flags takes 0 or MS_RNNT_LOG_PROBS_IN");
  MS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (!ms::rl_supported(N, T, U1)) {
    ms::set_error("ms_rnnt_align: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_align_workspace_bytes(N, T, U1, V1)) {
    ms::set_error("ms_rnnt_align: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t plane_bytes = ms::rl_skew_plane_bytes(N, T, U1);
  float* b_sk = (float*)workspace;
  float* e_sk = (float*)((char*)workspace + plane_bytes);
  float* Z = (float*)((char*)workspace + 2 * plane_bytes);
  u64* bp_ws = (u64*)((char*)workspace + 2 * plane_bytes + ms::align_up((size_t)N * T * U1 * sizeof(float), 256));
  if (flags & MS_RNNT_LOG_PROBS_IN) {
    const long R = (long)((size_t)N * T * U1);
    hipLaunchKernelGGL(rnnt_align_gather_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, logits, in_lens, targets,
                       tgt_lens, b_sk, e_sk, R, T, U1, V1, blank);
    MS_LAUNCH_CHECK();
  } else {
    const int rc = ms::rnnt_normalise_launch(logits, in_lens, targets, tgt_lens, Z, b_sk, e_sk, N, T, U1, V1, blank, st);
    if (rc != MS_OK) return rc;
  }
  return ra_launch(in_lens, targets, tgt_lens, b_sk, e_sk, bp_ws, score, token_frame, token_logp, frame_u, frame_logp, N, T, U1,
                   V1, blank, st);
}

extern "C" size_t ms_rnnt_align_joint_workspace_bytes(int N, int T, int U1, int J, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V1 <= 0) return 0;
  // the scorer's workspace (the two skewed planes, w_out packed); + the back-pointer rows past the LDS budget
  return ms::align_up(ms_rnnt_score_workspace_bytes(N, T, U1, J, V1), 256) + ra_bp_ws_bytes(N, T, U1);
}

extern "C" int ms_rnnt_align_joint(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                                   const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* score,
                                   int32_t* token_frame, float* token_logp, int32_t* frame_u, float* frame_logp, int N, int T,
                                   int U1, int J, int V1, int blank, void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && J > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(enc_p && pred_p && w_out && in_lens && tgt_lens && score && frame_u && frame_logp && workspace, "null pointer");
  MS_REQUIRE((targets && token_frame && token_logp) || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  MS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (!ms::rnnt_score_supported(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_align_joint: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_align_joint_workspace_bytes(N, T, U1, J, V1)) {
    ms::set_error("ms_rnnt_align_joint: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rc = ms::rnnt_score_cells_launch(enc_p, pred_p, w_out, b_out, in_lens, targets, tgt_lens, nullptr, N, T, U1, J, V1,
                                             blank, workspace, st);
  if (rc != MS_OK) return rc;
  const float* b_sk = (const float*)workspace;
  const float* e_sk = (const float*)((const char*)workspace + ms::rl_skew_plane_bytes(N, T, U1));
  u64* bp_ws = (u64*)((char*)workspace + ms::align_up(ms_rnnt_score_workspace_bytes(N, T, U1, J, V1), 256));
  return ra_launch(in_lens, targets, tgt_lens, b_sk, e_sk, bp_ws, score, token_frame, token_logp, frame_u, frame_logp, N, T, U1,
                   V1, blank, st);
}
