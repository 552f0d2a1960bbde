// Transducer (RNN-T) loss: forward (normalisers, alpha / beta lattice) and the gradient with respect to the joint's logits.
// OWN specification (the reference snapshot has no transducer): the comment on ms_rnnt_loss_forward in include/ms_hotpath.h;
// tests/rnnt_loss_ref.py restates it in numpy.  No MFMA: two row passes over [N, T, U1, V1] and one scan.
//
//   launch 1  rnnt_loss_normalise_kernel  a group of 8 / 16 / 32 / 64 lanes per cell row (several short rows per wave when
//                                         V1 <= 32, 16-byte loads when V1 is a multiple of 4): Z into the lattice, and the two
//                                         values of the row the recursion needs -- b = lp(blank), e = lp(y_u) -- into two
//                                         transient planes of the workspace
//   launch 2  rnnt_loss_lattice_kernel    2 N workgroups (alpha and beta of an utterance side by side), one thread per u,
//                                         walking the anti-diagonals d = t + u; launched through ms::rnnt_lattice_launch
//                                         (rnnt_loss.h), which ms_rnnt_score (rnnt_score.hip) calls on planes of its own
//   backward  rnnt_loss_grad_kernel       the row pass again: logits, Z, alpha, beta in, the grad row out; zeros for the cells
//                                         that do not exist, in the same launch
//
// The b / e planes are stored SKEWED, [n][t + u][u]: the cells of one anti-diagonal are one contiguous run, so the lattice
// pass reads 4 U1 contiguous bytes per plane and diagonal and never touches a V1-sized row.
// Lattice pass: alpha(t-1, u) (beta(t+1, u)) is the thread's own previous value; alpha(t, u-1) (beta(t, u+1)) is its
// neighbour's previous value -- a wave shuffle inside a wave, one LDS word per wave boundary (double-buffered by the parity
// of d, so ONE barrier per diagonal, and none at all when U1 <= 64).  The next diagonal's b / e are loaded before the
// barrier, which waits for the LDS only.  No workgroup waits on another: nothing spins, nothing can time out.
#include <math.h>

#include "common.h"
#include "rnnt_loss.h"

namespace {

// (shared with rnnt_score.hip: rnnt_loss.h)
using ms::RL_MAX_U1;
using ms::rl_label_ok;
using ms::rl_lens_ok;
using ms::rl_nan;
using ms::rl_neg_inf;
using ms::rl_skew_rows;
using ms::rl_supported;

constexpr int RL_ROW_THREADS = 256;

template <int G>
__device__ __forceinline__ float rl_group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float rl_group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// row r = (n T + t) U1 + u of the [N, T, U1] cell grid, one per group of G lanes
template <int G>
__device__ __forceinline__ bool rl_row_of_group(long R, int T, int U1, long& r, int& n, int& t, int& u, int& gl) {
  gl = threadIdx.x & (G - 1);
  r = (long)blockIdx.x * (RL_ROW_THREADS / G) + (threadIdx.x / G);
  if (r >= R) return false;
  const long q = r / U1;
  u = (int)(r - q * U1);
  n = (int)(q / T);
  t = (int)(q - (long)n * T);
  return true;
}

// Z of every existing cell; b and e of it into the skewed planes.  expf in its hardware form (the arguments are differences
// to the row's maximum), the precise logf once per row; b and e are formed as (x - max) - log(sum), which does not carry the
// rounding of Z = max + log(sum) into the recursion.
template <int G, bool VEC>
__global__ __launch_bounds__(RL_ROW_THREADS) void rnnt_loss_normalise_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ tgt_lens, float* __restrict__ Z, float* __restrict__ b_sk, float* __restrict__ e_sk, long R,
    int T, int U1, int V1, int blank) {
  long r;
  int n, t, u, gl;
  if (!rl_row_of_group<G>(R, T, U1, r, n, t, u, gl)) return;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  if (!rl_lens_ok(Tn, Un, T, U1) || t >= Tn || u > Un) return;
  const float* row = x + (size_t)r * V1;
  float m = rl_neg_inf();
  float sum = 0.f;
  if (VEC) {
    const ms::f32x4* row4 = reinterpret_cast<const ms::f32x4*>(row);
    const int V4 = V1 >> 2;
    for (int v = gl; v < V4; v += G) {
      const ms::f32x4 c = row4[v];
      m = fmaxf(fmaxf(m, fmaxf(c.x, c.y)), fmaxf(c.z, c.w));
    }
    m = rl_group_max<G>(m);
    for (int v = gl; v < V4; v += G) {              // (the row again: out of the cache this group has just filled)
      const ms::f32x4 c = row4[v];
      sum += (__expf(c.x - m) + __expf(c.y - m)) + (__expf(c.z - m) + __expf(c.w - m));
    }
  } else {
    for (int v = gl; v < V1; v += G) m = fmaxf(m, row[v]);
    m = rl_group_max<G>(m);
    for (int v = gl; v < V1; v += G) sum += __expf(row[v] - m);
  }
  sum = rl_group_sum<G>(sum);
  if (gl != 0) return;
  const float lse = logf(sum);
  float z = m + lse;
  const bool bad = !(fabsf(z) < INFINITY);         // a NaN or +inf logit, a row of -inf: poisons the utterance
  if (bad) z = rl_nan();
  Z[r] = z;
  float bv = (row[blank] - m) - lse;
  float ev = rl_neg_inf();
  if (u < Un) {
    const int lab = targets[(size_t)n * (U1 - 1) + u];
    if (rl_label_ok(lab, V1, blank)) ev = (row[lab] - m) - lse;   // (else: the lattice pass reports the utterance)
  }
  if (bad) bv = ev = rl_nan();
  const size_t o = ((size_t)n * rl_skew_rows(T, U1) + (size_t)(t + u)) * U1 + u;
  b_sk[o] = bv;
  e_sk[o] = ev;
}

// The running sums of the recursion are float32 PAIRS (h + l, |l| <= ulp(h) / 2): off the likely alignments alpha and beta
// reach magnitudes of several hundred while nll can be of order 1 (a trained model), and a plain float32 sum would round
// by 2^-24 |alpha| at every step -- more than the whole error budget 8 (T_n + U_n) 2^-24 max(1, |nll|) at such cells.  The
// pair keeps the running error at the level of the terms added; the lattice stores h + l rounded once.
struct rl_pair {
  float h, l;
};

// p + b (Knuth's two-sum, then renormalised); a -inf or NaN sum carries no low part
__device__ __forceinline__ rl_pair rl_add(rl_pair p, float b) {
  const float s = p.h + b;
  if (!(fabsf(s) < INFINITY)) return {s, 0.f};
  const float bb = s - p.h;
  const float e = ((p.h - (s - bb)) + (b - bb)) + p.l;
  const float h = s + e;
  return {h, e - (h - s)};
}

// log(exp(a) + exp(b)) for a, b in {NaN, -inf, finite}: -inf for two -inf, NaN if either is NaN (fmaxf / fminf drop a NaN,
// so the -inf case hands back the OTHER argument and the general case goes through the difference).  exp and log in their
// hardware forms: the argument of exp is <= 0 (up to a low part) and the sum lies in [1, 2], absolute error ~1e-7.
__device__ __forceinline__ rl_pair rl_logaddexp(rl_pair a, rl_pair b) {
  if (fminf(a.h, b.h) == rl_neg_inf()) return a.h == rl_neg_inf() ? b : a;
  const bool ge = a.h >= b.h;
  const rl_pair hi = ge ? a : b, lo = ge ? b : a;
  const float d = (lo.h - hi.h) + (lo.l - hi.l);
  return rl_add(hi, __logf(1.f + __expf(d)));
}

__device__ __forceinline__ float rl_value(rl_pair p) { return p.h + p.l; }

// barrier that waits for this wave's LDS operations only: __syncthreads() would also wait for the loads just issued for the
// next diagonal (ctc_align_kernel)
__device__ __forceinline__ void rl_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// blockIdx.x = 2 n + (0: alpha, 1: beta); blockDim.x = U1 rounded up to whole waves; MULTI: more than one wave
template <bool MULTI>
__global__ __launch_bounds__(RL_MAX_U1) void rnnt_loss_lattice_kernel(
    const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets, const int32_t* __restrict__ tgt_lens,
    const float* __restrict__ b_sk, const float* __restrict__ e_sk, float* __restrict__ alpha, float* __restrict__ beta,
    float* __restrict__ nll, int T, int U1, int V1, int blank) {
  __shared__ rl_pair xch[2][RL_MAX_U1 / 64];      // [parity of d][wave]: the value that crosses a wave boundary
  const int n = blockIdx.x >> 1, backward = blockIdx.x & 1;
  const int u = threadIdx.x, lane = u & 63, w = u >> 6;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  int invalid = rl_lens_ok(Tn, Un, T, U1) ? 0 : 1;
  if (!invalid && u < Un && !rl_label_ok(targets[(size_t)n * (U1 - 1) + u], V1, blank)) invalid = 1;
  if (MULTI) {
    if (u < 2 * (RL_MAX_U1 / 64)) (&xch[0][0])[u] = rl_pair{rl_neg_inf(), 0.f};
    invalid = __syncthreads_or(invalid);          // (also: the -inf above are in place)
  } else {
    invalid = __ballot(invalid != 0) != 0ull;
  }
  if (invalid) {
    if (!backward && u == 0) nll[n] = INFINITY;
    return;
  }
  const int D = Tn + Un;                          // anti-diagonals 0 .. D - 1; D <= T + U1 - 1 rows of the skewed planes
  const int uu = min(u, U1 - 1);                  // (threads past U1 load an in-bounds word they never use)
  const float* bs = b_sk + (size_t)n * rl_skew_rows(T, U1) * U1 + uu;
  const float* es = e_sk + (size_t)n * rl_skew_rows(T, U1) * U1 + uu;
  float* out = (backward ? beta : alpha) + (size_t)n * T * U1 + u;
  const bool has_e = u < Un;
  const int d0 = backward ? D - 1 : 0, step = backward ? -1 : 1;
  // forward: `own` is alpha(t-1, u) + b(t-1, u), `pass` (handed to thread u + 1) is alpha(t, u) + e(t, u); alpha(0, 0) = 0 comes
  // out of a virtual predecessor 0.  backward: own = pass = beta of the previous diagonal; beta(T_n-1, U_n) = b comes out of a
  // virtual successor 0.
  const rl_pair none = {rl_neg_inf(), 0.f};
  rl_pair own = (u == (backward ? Un : 0)) ? rl_pair{0.f, 0.f} : none;
  rl_pair pass = none;
  float b_next = bs[(size_t)d0 * U1], e_next = es[(size_t)d0 * U1];
  for (int i = 0, d = d0; i < D; ++i, d += step) {
    const int t = d - u;
    const bool valid = u <= Un && t >= 0 && t < Tn;
    const float bc = valid ? b_next : rl_neg_inf();
    const float ec = (valid && has_e) ? e_next : rl_neg_inf();
    if (i + 1 < D) {                              // the next diagonal's values: in flight across the barrier
      b_next = bs[(size_t)(d + step) * U1];
      e_next = es[(size_t)(d + step) * U1];
    }
    rl_pair nb;
    if (!backward) {
      nb = {__shfl_up(pass.h, 1, 64), __shfl_up(pass.l, 1, 64)};
      if (lane == 0) nb = (MULTI && w > 0) ? xch[(d + 1) & 1][w - 1] : none;
    } else {
      nb = {__shfl_down(pass.h, 1, 64), __shfl_down(pass.l, 1, 64)};
      if (lane == 63) nb = (MULTI && u + 1 < (int)blockDim.x) ? xch[(d + 1) & 1][w + 1] : none;
    }
    rl_pair v;
    if (!backward) {
      v = valid ? rl_logaddexp(own, nb) : none;
      own = rl_add(v, bc);
      pass = rl_add(v, ec);
    } else {
      v = valid ? rl_logaddexp(rl_add(own, bc), rl_add(nb, ec)) : none;
      own = v;
      pass = v;
    }
    if (valid) out[(size_t)t * U1] = rl_value(v);
    if (MULTI) {
      if (lane == (backward ? 0 : 63)) xch[d & 1][w] = pass;
      rl_lds_barrier();
    }
  }
  if (!backward && u == Un) nll[n] = -rl_value(own);   // own = alpha(T_n-1, U_n) + b(T_n-1, U_n) = ll
}

template <int G, bool VEC>
__global__ __launch_bounds__(RL_ROW_THREADS) void rnnt_loss_grad_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ in_lens, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ tgt_lens, const float* __restrict__ nll, const float* __restrict__ Z,
    const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ grad_nll,
    float* __restrict__ grad, long R, int T, int U1, int V1, int blank) {
  long r;
  int n, t, u, gl;
  if (!rl_row_of_group<G>(R, T, U1, r, n, t, u, gl)) return;
  const int Tn = in_lens[n], Un = tgt_lens[n];
  const float nl = nll[n];
  const float* row = x + (size_t)r * V1;
  float* grow = grad + (size_t)r * V1;
  const bool exists = rl_lens_ok(Tn, Un, T, U1) && t < Tn && u <= Un;
  if (!exists || !(fabsf(nl) < INFINITY)) {
    // a cell that does not exist, an impossible transcript (+inf): zeros; a poisoned utterance (NaN): NaN in its cells
    const float fill = (exists && nl != nl) ? rl_nan() : 0.f;
    if (VEC) {
      ms::f32x4* g4 = reinterpret_cast<ms::f32x4*>(grow);
      const ms::f32x4 f4 = {fill, fill, fill, fill};
      for (int v = gl; v < (V1 >> 2); v += G) g4[v] = f4;
    } else {
      for (int v = gl; v < V1; v += G) grow[v] = fill;
    }
    return;
  }
  const float z = Z[r], a = alpha[r], g = grad_nll[n];
  const float c = (a + beta[r]) + nl;                                    // alpha + beta - ll
  // the successor through the blank: beta(t+1, u); past the last frame only (T_n-1, U_n) has one, the end itself
  const float tb = (t + 1 < Tn) ? beta[r + U1] : (u == Un ? 0.f : rl_neg_inf());
  const float kb = __expf(((row[blank] - z) + (a + tb)) + nl);
  int lab = -1;
  float ke = 0.f;
  if (u < Un) {
    const int l = targets[(size_t)n * (U1 - 1) + u];
    if (rl_label_ok(l, V1, blank)) {              // (nll is finite only when every label is; the index is checked all the same)
      lab = l;
      ke = __expf(((row[l] - z) + (a + beta[r + 1])) + nl);
    }
  }
  if (VEC) {
    const ms::f32x4* row4 = reinterpret_cast<const ms::f32x4*>(row);
    ms::f32x4* g4 = reinterpret_cast<ms::f32x4*>(grow);
    for (int v4 = gl; v4 < (V1 >> 2); v4 += G) {
      const ms::f32x4 xv = row4[v4];
      ms::f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = 4 * v4 + j;
        float val = __expf((xv[j] - z) + c);
        if (v == blank) val -= kb;
        if (v == lab) val -= ke;
        o[j] = g * val;
      }
      g4[v4] = o;
    }
  } else {
    for (int v = gl; v < V1; v += G) {
      float val = __expf((row[v] - z) + c);
      if (v == blank) val -= kb;
      if (v == lab) val -= ke;
      grow[v] = g * val;
    }
  }
}

inline int rl_group(int V1, bool vec) {
  const int per_lane = vec ? 4 : 1;
  return V1 <= 8 * per_lane ? 8 : V1 <= 16 * per_lane ? 16 : V1 <= 32 * per_lane ? 32 : 64;
}

// launches KERNEL<G, VEC> over R rows with the group width that suits V1
#define RL_ROW_LAUNCH(KERNEL, R, V1, vec, st, ...)                                                                       \
  do {                                                                                                                   \
    const int g_ = rl_group(V1, vec);                                                                                    \
    const dim3 grid_((unsigned)(((R) + RL_ROW_THREADS / g_ - 1) / (RL_ROW_THREADS / g_)));                               \
    const dim3 block_(RL_ROW_THREADS);                                                                                   \
    if (vec) {                                                                                                           \
      if (g_ == 8) hipLaunchKernelGGL((KERNEL<8, true>), grid_, block_, 0, st, __VA_ARGS__);                             \
      else if (g_ == 16) hipLaunchKernelGGL((KERNEL<16, true>), grid_, block_, 0, st, __VA_ARGS__);                      \
      else if (g_ == 32) hipLaunchKernelGGL((KERNEL<32, true>), grid_, block_, 0, st, __VA_ARGS__);                      \
      else hipLaunchKernelGGL((KERNEL<64, true>), grid_, block_, 0, st, __VA_ARGS__);                                    \
    } else {                                                                                                             \
      if (g_ == 8) hipLaunchKernelGGL((KERNEL<8, false>), grid_, block_, 0, st, __VA_ARGS__);                            \
      else if (g_ == 16) hipLaunchKernelGGL((KERNEL<16, false>), grid_, block_, 0, st, __VA_ARGS__);                     \
      else if (g_ == 32) hipLaunchKernelGGL((KERNEL<32, false>), grid_, block_, 0, st, __VA_ARGS__);                     \
      else hipLaunchKernelGGL((KERNEL<64, false>), grid_, block_, 0, st, __VA_ARGS__);                                   \
    }                                                                                                                    \
  } while (0)

inline bool rl_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int ms::rnnt_lattice_launch(const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, const float* b_sk,
                            const float* e_sk, float* alpha, float* beta, float* nll, int N, int T, int U1, int V1, int blank,
                            hipStream_t st) {
  const int threads = ms::cdiv(U1, 64) * 64;
  if (threads > 64)
    hipLaunchKernelGGL(rnnt_loss_lattice_kernel<true>, dim3(2 * N), dim3(threads), 0, st, in_lens, targets, tgt_lens, b_sk, e_sk,
                       alpha, beta, nll, T, U1, V1, blank);
  else
    hipLaunchKernelGGL(rnnt_loss_lattice_kernel<false>, dim3(2 * N), dim3(64), 0, st, in_lens, targets, tgt_lens, b_sk, e_sk,
                       alpha, beta, nll, T, U1, V1, blank);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

int ms::rnnt_normalise_launch(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                              float* Z, float* b_sk, float* e_sk, int N, int T, int U1, int V1, int blank, hipStream_t st) {
  const long R = (long)((size_t)N * T * U1);
  const bool vec = (V1 % 4 == 0) && rl_aligned16(logits);
  RL_ROW_LAUNCH(rnnt_loss_normalise_kernel, R, V1, vec, st, logits, in_lens, targets, tgt_lens, Z, b_sk, e_sk, R, T, U1, V1,
                blank);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" size_t ms_rnnt_loss_lattice_bytes(int N, int T, int U1) {
  if (N <= 0 || T <= 0 || U1 <= 0) return 0;
  return (size_t)3 * N * T * U1 * sizeof(float);
}

extern "C" size_t ms_rnnt_loss_workspace_bytes(int N, int T, int U1, int V1) {
  if (N <= 0 || T <= 0 || U1 <= 0 || V1 <= 0) return 0;
  // the b and the e plane, skewed: [N][T + U1 - 1][U1] floats each
  return 2 * ms::align_up((size_t)N * rl_skew_rows(T, U1) * U1 * sizeof(float), 256);
}

extern "C" int ms_rnnt_loss_forward(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                                    float* nll, float* lattice, int N, int T, int U1, int V1, int blank, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(logits && in_lens && tgt_lens && nll && lattice && workspace, "null pointer");
  MS_REQUIRE(targets || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  if (!rl_supported(N, T, U1)) {
    ms::set_error("ms_rnnt_loss_forward: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < ms_rnnt_loss_workspace_bytes(N, T, U1, V1)) {
    ms::set_error("ms_rnnt_loss_forward: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t plane = (size_t)N * T * U1;
  float* Z = lattice;
  float* alpha = lattice + plane;
  float* beta = lattice + 2 * plane;
  float* b_sk = (float*)workspace;
  float* e_sk = (float*)((char*)workspace + ms::align_up((size_t)N * rl_skew_rows(T, U1) * U1 * sizeof(float), 256));
  const int rc = ms::rnnt_normalise_launch(logits, in_lens, targets, tgt_lens, Z, b_sk, e_sk, N, T, U1, V1, blank, st);
  if (rc != MS_OK) return rc;
  return ms::rnnt_lattice_launch(in_lens, targets, tgt_lens, b_sk, e_sk, alpha, beta, nll, N, T, U1, V1, blank, st);
}

extern "C" int ms_rnnt_loss_backward(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                                     const float* nll, const float* lattice, const float* grad_nll, float* grad, int N, int T,
                                     int U1, int V1, int blank, void* stream) {
  MS_REQUIRE(N > 0 && T > 0 && U1 > 0 && V1 > 0, "bad shape");
  MS_REQUIRE(logits && in_lens && tgt_lens && nll && lattice && grad_nll && grad, "null pointer");
  MS_REQUIRE(targets || U1 == 1, "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V1, "blank out of range");
  if (!rl_supported(N, T, U1)) {
    ms::set_error("ms_rnnt_loss_backward: supported up to U1 = 1024 (and N T U1 below 2^33 cells)");
    return MS_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t plane = (size_t)N * T * U1;
  const long R = (long)plane;
  const bool vec = (V1 % 4 == 0) && rl_aligned16(logits) && rl_aligned16(grad);
  RL_ROW_LAUNCH(rnnt_loss_grad_kernel, R, V1, vec, st, logits, in_lens, targets, tgt_lens, nll, lattice, lattice + plane,
                lattice + 2 * plane, grad_nll, grad, R, T, U1, V1, blank);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
