// Backward of the masked convolutions (groups == 1) and of the lookahead convolution.  OWN specification: the comment on
// ms_maskconv_backward_data in include/ms_hotpath.h; tests/conv_backward_cases.py restates it in float64 numpy.
//
// Both convolution gradients are implicit GEMMs on v_mfma_f32_32x32x2_f32 with float32 accumulation: a gradient under a
// mean-reduced loss sits far below fp16's normal range, where the hi + lo planes of the forward kernels lose what the split
// exists to keep.  A workgroup is ONE wave with four independent accumulators (the instruction's issue interval and its
// dependent latency are both 64 cycles, so four chains keep a SIMD's matrix pipe full); operands come from global memory
// through the caches, except the weight gradient's A operand, which is staged through 8 KB of LDS to turn a gather into
// row reads.  The gate g = dy where the saved OUTPUT is strictly inside the clamp (or there is no clamp), +0 elsewhere, is
// applied while dy is loaded.  Masked frames, padding, and rows / columns / k past an
// extent are LOAD PREDICATES: the element is never read, the operand is a literal 0.
//
// ROUTING.  There is one route per gradient and it serves every groups == 1 geometry; channel counts that are no multiple of 32
// leave rows (or columns) of a tile unused:
//   data gradient   rows = 32 input channels, columns = 128 input frames of ONE residue class ti = r (mod ST) of one (n, fi),
//                   k = (co, kf, kt).  A residue class sees a dense sub-filter: the kt with (r + pad_t - kt DT) % ST == 0; the
//                   kf that do not hit an output row (parity under SF, or outside [0, Fout)) are skipped, both per wave.
//   weight gradient rows = 32 output channels, columns = 128 consecutive elements of the flattened (ci, kf, kt) filter axis
//                   followed by ONE extra column of ones whose sum is db, k = the flattened (n, fo, to) axis.  k is cut into
//                   slices of CBW_SLICE (a constant: the count depends on the arguments only, never on the device), partials
//                   go to the workspace and a second launch adds them in ascending slice order.  Consecutive columns are
//                   consecutive kt of a (ci, kf), so a wave's B operand reads overlapping shifts of the same x rows.
// No atomics anywhere: the same bits on every run and every device.
//
// The lookahead gradients are HBM / L2-bound sliding sums on the vector ALU, one thread per output element, taps guarded by
// k < ctx and t + k < T and summed in a fixed order.
#include "common.h"

namespace ms {

constexpr int CBW_SLICE = 8192;     // k = (n, fo, to) elements per slice of the weight gradient (tests/conv_backward_cases.py names it)
constexpr int CBW_KC = 64;          // k elements staged at a time (one per lane); CBW_SLICE is a multiple
constexpr int CB_ACC = 4;           // independent 32 x 32 accumulators per wave
constexpr int CB_COLS = 32 * CB_ACC;

struct ConvGeom {
  int N, Cin, Fin, Tin, Cout, Fout, Tout, KF, KT, SF, ST, DF, DT, pad_f, pad_t;
  int act;
  float lo, hi;
};

__device__ __forceinline__ float gated(const float* __restrict__ dy, const float* __restrict__ y, size_t idx, int act, float lo,
                                       float hi) {
  const float d = dy[idx];
  if (act == MS_ACT_NONE) return d;
  const float v = y[idx];
  return (v > lo && v < hi) ? d : 0.f;
}

__device__ __forceinline__ int live_frames(const int32_t* lens, int n, int T) {
  return lens ? min(max(lens[n], 0), T) : T;
}

// grid.x = N * Fin * ST * ceil(Cin / 32) * ceil(ceil(Tin / ST) / 128), one wave each.
__global__ __launch_bounds__(64) void conv_bwd_data_kernel(const float* __restrict__ w, const float* __restrict__ y,
                                                           const float* __restrict__ dy, const int32_t* __restrict__ lens,
                                                           float* __restrict__ dx, const ConvGeom g, int ci_tiles, int j_tiles) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int jt = b % j_tiles; b /= j_tiles;
  const int cit = b % ci_tiles; b /= ci_tiles;
  const int r = b % g.ST; b /= g.ST;
  const int fi = b % g.Fin;
  const int n = b / g.Fin;
  const int ci = cit * 32 + l31;      // this lane's row of the A operand
  const int j0 = jt * CB_COLS;
  f32x16 acc[CB_ACC];
#pragma unroll
  for (int q = 0; q < CB_ACC; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

  // the output channel pair is the OUTER loop: a lane then walks the KF KT taps of one (co, ci) filter, which are contiguous,
  // so a cache line of w serves 32 consecutive products (tap-outer order re-fetched every line of the bank per tap)
  for (int c0 = 0; c0 < g.Cout; c0 += 2) {
    const int co = c0 + half;
    const bool a_live = ci < g.Cin && co < g.Cout;
    const float* __restrict__ wf = w + ((size_t)min(co, g.Cout - 1) * g.Cin + min(ci, g.Cin - 1)) * g.KF * g.KT;
    const size_t gplane = ((size_t)n * g.Cout + min(co, g.Cout - 1)) * g.Fout;
    for (int kf = 0; kf < g.KF; ++kf) {
      const int nf = fi + g.pad_f - kf * g.DF;
      if (nf < 0 || (g.SF != 1 && nf % g.SF != 0)) continue;
      const int fo = nf / g.SF;
      if (fo >= g.Fout) continue;
      const size_t grow = (gplane + fo) * g.Tout;
      for (int kt = 0; kt < g.KT; ++kt) {
        const int nt = r + g.pad_t - kt * g.DT;
        if (g.ST != 1 && ((nt % g.ST) + g.ST) % g.ST != 0) continue;
        const int to0 = nt / g.ST + j0 + l31;      // (exact: nt is a multiple of ST) the output frame of this lane's first column
        const float a = a_live ? wf[kf * g.KT + kt] : 0.f;
        float bv[CB_ACC];
#pragma unroll
        for (int q = 0; q < CB_ACC; ++q) {
          const int to = to0 + 32 * q;
          bv[q] = 0.f;
          if (co < g.Cout && to >= 0 && to < g.Tout) bv[q] = gated(dy, y, grow + to, g.act, g.lo, g.hi);
        }
#pragma unroll
        for (int q = 0; q < CB_ACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[q], acc[q], 0, 0, 0);
      }
    }
  }
  const int len = live_frames(lens, n, g.Tin);
#pragma unroll
  for (int q = 0; q < CB_ACC; ++q) {
    const int ti = r + g.ST * (j0 + 32 * q + l31);
    if (ti >= g.Tin) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = cit * 32 + mfma32_row(i, lane);
      if (row < g.Cin) dx[(((size_t)n * g.Cin + row) * g.Fin + fi) * g.Tin + ti] = ti < len ? acc[q][i] : 0.f;
    }
  }
}

// grid = (ceil((Cin KF KT + 1) / 128), ceil(Cout / 32), slices), one wave each.  part is [slices][Cout][Cin KF KT + 1].
__global__ __launch_bounds__(64) void conv_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, const int32_t* __restrict__ lens,
                                                             float* __restrict__ part, const ConvGeom g, long long K) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int ncols = g.Cin * g.KF * g.KT;       // column `ncols` is the column of ones
  __shared__ float gs[32][CBW_KC + 1];         // [output channel of the tile][k of the chunk]; the pad spreads a column's rows over the banks
  const long long k_begin = (long long)blockIdx.z * CBW_SLICE;
  const long long k_end = min(k_begin + CBW_SLICE, K);
  // this lane's column of each accumulator: the x plane it reads and its tap offsets
  int col[CB_ACC], off_f[CB_ACC], off_t[CB_ACC];
  size_t plane[CB_ACC];
#pragma unroll
  for (int q = 0; q < CB_ACC; ++q) {
    col[q] = blockIdx.x * CB_COLS + 32 * q + l31;
    const int c = min(col[q], ncols - 1);
    const int kt = c % g.KT, kf = (c / g.KT) % g.KF, ci = c / (g.KT * g.KF);
    off_f[q] = kf * g.DF - g.pad_f;
    off_t[q] = kt * g.DT - g.pad_t;
    plane[q] = (size_t)ci * g.Fin * g.Tin;
  }
  f32x16 acc[CB_ACC];
#pragma unroll
  for (int q = 0; q < CB_ACC; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

  const size_t co_stride = (size_t)g.Fout * g.Tout;
  for (long long kc = k_begin; kc < k_end; kc += CBW_KC) {
    // stage the gated gradient of the tile's 32 output channels at k = kc .. kc + 63: lanes walk k, which is contiguous in dy
    // (rows of 64 consecutive floats), where the MFMA's own A layout -- a lane per channel -- is a gather of 32 cache lines
    {
      const long long k = kc + lane;
      const long long row = k / g.Tout;
      const int to = (int)(k - row * g.Tout);
      const int n = (int)(row / g.Fout);
      const int fo = (int)(row - (long long)n * g.Fout);
      const size_t base = ((size_t)n * g.Cout * g.Fout + fo) * g.Tout + to;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) {
        const int c = blockIdx.y * 32 + r;
        float v = 0.f;
        if (k < k_end && c < g.Cout) v = gated(dy, y, base + c * co_stride, g.act, g.lo, g.hi);
        gs[r][lane] = v;
      }
    }
    __syncthreads();
    // this lane half's 32 k of the chunk, walked with carries
    long long k = kc + 32 * half;
    const long long row = k / g.Tout;
    int to = (int)(k - row * g.Tout);
    int n = (int)(row / g.Fout);
    int fo = (int)(row - (long long)n * g.Fout);
#pragma unroll 4
    for (int e = 0; e < 32; ++e, ++k) {
      const bool live = k < k_end;
      const float a = gs[l31][32 * half + e];      // (0 past k_end and past Cout)
      float bv[CB_ACC] = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        const int len = live_frames(lens, n, g.Tin);
        const size_t xn = (size_t)n * g.Cin * g.Fin * g.Tin;
#pragma unroll
        for (int q = 0; q < CB_ACC; ++q) {
          const int fi = fo * g.SF + off_f[q], ti = to * g.ST + off_t[q];
          if (col[q] < ncols) {
            if (fi >= 0 && fi < g.Fin && ti >= 0 && ti < len) bv[q] = x[xn + plane[q] + (size_t)fi * g.Tin + ti];
          } else if (col[q] == ncols) {
            bv[q] = 1.f;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < CB_ACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[q], acc[q], 0, 0, 0);
      if (++to == g.Tout) {
        to = 0;
        if (++fo == g.Fout) {
          fo = 0;
          ++n;
        }
      }
    }
    __syncthreads();      // the next chunk rewrites gs
  }
  float* out = part + (size_t)blockIdx.z * g.Cout * (ncols + 1);
#pragma unroll
  for (int q = 0; q < CB_ACC; ++q) {
    if (col[q] > ncols) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = blockIdx.y * 32 + mfma32_row(i, lane);
      if (r < g.Cout) out[(size_t)r * (ncols + 1) + col[q]] = acc[q][i];
    }
  }
}

// dw[co, c] (and db[co] from the column of ones) = the slices' partials added in ascending slice order.
__global__ __launch_bounds__(256) void conv_bwd_weight_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                     float* __restrict__ db, int Cout, int ncols, int slices) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)Cout * (ncols + 1);
  if (idx >= total) return;
  float s = part[idx];
  for (int i = 1; i < slices; ++i) s += part[(size_t)i * total + idx];
  const int co = (int)(idx / (ncols + 1)), c = (int)(idx % (ncols + 1));
  if (c < ncols) dw[(size_t)co * ncols + c] = s;
  else if (db) db[co] = s;
}

// dx[n, f, t] = sum_{k <= min(t, ctx - 1)} w[f, k] g[n, f, t - k], k ascending.  `f_fast`: consecutive threads walk f (a
// feature-contiguous layout), else t.
__global__ __launch_bounds__(256) void lookahead_bwd_data_kernel(const float* __restrict__ w, const float* __restrict__ y,
                                                                 const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                                 int F, int T, int ctx, long xs_n, long xs_f, long xs_t,
                                                                 long ys_n, long ys_f, long ys_t, int act, float lo, float hi,
                                                                 int f_fast) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * F * T) return;
  int n, f, t;
  if (f_fast) {
    f = (int)(idx % F);
    t = (int)((idx / F) % T);
  } else {
    t = (int)(idx % T);
    f = (int)((idx / T) % F);
  }
  n = (int)(idx / ((size_t)F * T));
  const int taps = min(t, ctx - 1);
  float s = 0.f;
  for (int k = 0; k <= taps; ++k)
    s += w[(size_t)f * ctx + k] * gated(dy, y, (size_t)(n * ys_n + f * ys_f + (long)(t - k) * ys_t), act, lo, hi);
  dx[n * xs_n + f * xs_f + t * xs_t] = s;
}

// dw[f, k] = sum_n sum_{t: t + k < T} g[n, f, t] x[n, f, t + k], n then t ascending.  One thread per (f, k); threadIdx.x walks f.
__global__ __launch_bounds__(256) void lookahead_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   const float* __restrict__ dy, float* __restrict__ dw, int N,
                                                                   int F, int T, int ctx, long xs_n, long xs_f, long xs_t,
                                                                   long ys_n, long ys_f, long ys_t, int act, float lo, float hi) {
  const int f = blockIdx.x * 64 + (threadIdx.x & 63);
  const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (f >= F || k >= ctx) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n)
    for (int t = 0; t + k < T; ++t)
      s += gated(dy, y, (size_t)(n * ys_n + f * ys_f + t * ys_t), act, lo, hi) * x[n * xs_n + f * xs_f + (long)(t + k) * xs_t];
  dw[(size_t)f * ctx + k] = s;
}

static bool conv_geom_ok(const ConvGeom& g) {
  return g.N > 0 && g.Cin > 0 && g.Fin > 0 && g.Tin > 0 && g.Cout > 0 && g.Fout > 0 && g.Tout > 0 && g.KF > 0 && g.KT > 0 &&
         g.SF > 0 && g.ST > 0 && g.DF > 0 && g.DT > 0 && g.pad_f >= 0 && g.pad_t >= 0 &&
         (g.act == MS_ACT_NONE || g.act == MS_ACT_CLAMP) &&
         // (no output position may lie wholly to the left of / above the input: Fout and Tout belong to this geometry)
         (long long)(g.Fout - 1) * g.SF - g.pad_f < g.Fin && (long long)(g.Tout - 1) * g.ST - g.pad_t < g.Tin &&
         (long long)g.Cin * g.KF * g.KT < (1ll << 30);
}

static long long conv_k(const ConvGeom& g) { return (long long)g.N * g.Fout * g.Tout; }

}  // namespace ms

extern "C" size_t ms_maskconv_backward_workspace_bytes(int N, int Cin, int Cout, int Fout, int Tout, int KF, int KT) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || Fout <= 0 || Tout <= 0 || KF <= 0 || KT <= 0) return 0;
  const long long K = (long long)N * Fout * Tout;
  const size_t slices = (size_t)((K + ms::CBW_SLICE - 1) / ms::CBW_SLICE);
  return ms::align_up(slices * (size_t)Cout * ((size_t)Cin * KF * KT + 1) * sizeof(float), 256);
}

extern "C" int ms_maskconv_backward_data(const float* w, const float* y, const float* dy, const int32_t* lens, float* dx, int N,
                                         int Cin, int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST,
                                         int DF, int DT, int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi,
                                         void* stream) {
  ms::ProfScope prof_span(MS_PROF_CONV, (hipStream_t)stream);
  const ms::ConvGeom g{N, Cin, Fin, Tin, Cout, Fout, Tout, KF, KT, SF, ST, DF, DT, pad_f_l, pad_t_l, act, act_lo, act_hi};
  MS_REQUIRE(w && dy && dx && (y || act == MS_ACT_NONE), "null pointer");
  MS_REQUIRE(ms::conv_geom_ok(g), "bad geometry");
  const int ci_tiles = ms::cdiv(Cin, 32), j_tiles = ms::cdiv(ms::cdiv(Tin, ST), ms::CB_COLS);
  const long long blocks = (long long)N * Fin * ST * ci_tiles * j_tiles;
  MS_REQUIRE(blocks < (1ll << 31), "too many tiles for one launch");
  hipLaunchKernelGGL(ms::conv_bwd_data_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, w, y, dy, lens, dx, g,
                     ci_tiles, j_tiles);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_maskconv_backward_weight(const float* x, const float* y, const float* dy, const int32_t* lens, float* dw,
                                           float* db, int N, int Cin, int Fin, int Tin, int Cout, int Fout, int Tout, int KF,
                                           int KT, int SF, int ST, int DF, int DT, int pad_f_l, int pad_t_l, int act,
                                           float act_lo, float act_hi, void* workspace, size_t workspace_bytes, void* stream) {
  ms::ProfScope prof_span(MS_PROF_CONV, (hipStream_t)stream);
  const ms::ConvGeom g{N, Cin, Fin, Tin, Cout, Fout, Tout, KF, KT, SF, ST, DF, DT, pad_f_l, pad_t_l, act, act_lo, act_hi};
  MS_REQUIRE(x && dy && dw && (y || act == MS_ACT_NONE), "null pointer");
  MS_REQUIRE(ms::conv_geom_ok(g), "bad geometry");
  const long long K = ms::conv_k(g);
  const long long slices = (K + ms::CBW_SLICE - 1) / ms::CBW_SLICE;
  const int ncols = Cin * KF * KT;
  MS_REQUIRE(slices <= 65535 && ms::cdiv(Cout, 32) <= 65535, "too many slices for one launch");
  if (!workspace || workspace_bytes < ms_maskconv_backward_workspace_bytes(N, Cin, Cout, Fout, Tout, KF, KT)) {
    ms::set_error(std::string(__func__) + ": workspace too small");
    return MS_ERR_WORKSPACE;
  }
  float* part = (float*)workspace;
  hipLaunchKernelGGL(ms::conv_bwd_weight_kernel, dim3(ms::cdiv(ncols + 1, ms::CB_COLS), ms::cdiv(Cout, 32), (unsigned)slices),
                     dim3(64), 0, (hipStream_t)stream, x, y, dy, lens, part, g, K);
  MS_LAUNCH_CHECK();
  const size_t total = (size_t)Cout * (ncols + 1);
  hipLaunchKernelGGL(ms::conv_bwd_weight_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     part, dw, db, Cout, ncols, (int)slices);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_lookahead_backward(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, int N,
                                     int F, int T, int ctx, long xs_n, long xs_f, long xs_t, long ys_n, long ys_f, long ys_t,
                                     int act, float act_lo, float act_hi, void* stream) {
  ms::ProfScope prof_span(MS_PROF_OTHER, (hipStream_t)stream);
  MS_REQUIRE(w && dy && (dx || dw) && (x || !dw) && (y || act == MS_ACT_NONE), "null pointer");
  MS_REQUIRE(N > 0 && F > 0 && T > 0 && ctx > 0, "bad shape");
  MS_REQUIRE(act == MS_ACT_NONE || act == MS_ACT_CLAMP, "bad act");
  MS_REQUIRE((long long)N * F * T < (1ll << 39) && ctx <= 4 * 65535, "dimension exceeds grid limits");
  if (dx) {
    const size_t total = (size_t)N * F * T;
    hipLaunchKernelGGL(ms::lookahead_bwd_data_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, y,
                       dy, dx, N, F, T, ctx, xs_n, xs_f, xs_t, ys_n, ys_f, ys_t, act, act_lo, act_hi, xs_f == 1 ? 1 : 0);
    MS_LAUNCH_CHECK();
  }
  if (dw) {
    hipLaunchKernelGGL(ms::lookahead_bwd_weight_kernel, dim3(ms::cdiv(F, 64), ms::cdiv(ctx, 4)), dim3(256), 0, (hipStream_t)stream,
                       x, y, dy, dw, N, F, T, ctx, xs_n, xs_f, xs_t, ys_n, ys_f, ys_t, act, act_lo, act_hi);
    MS_LAUNCH_CHECK();
  }
  return MS_OK;
}
