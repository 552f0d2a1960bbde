// Backward through time of one torch.nn.LSTM layer, unidirectional or bidirectional (gate order i, f, g, o; weights in torch
// layout, no packed copy), and the embedding backward beside it.  OWN specification: the comment on ms_lstm_recompute in
// include/ms_hotpath.h; tests/lstm_backward_ref.py restates it in float64 numpy, tests/bilstm_backward_ref.py the reverse
// direction (the same cell walked from lens[n] - 1 down to 0).
//
// The forward kernels (rnn.hip) save no gates.  ms_lstm_recompute rebuilds them from what the forward returns: every
// h_{t-1} is known, so the pre-activations of ALL steps are two batch products over T*N rows on the exact float32 MFMA
// GEMM of gemm.hip, and a scan (one thread per (n, j), c in a register) applies the cell.
//
// ms_lstm_backward_steps is the recurrence: ONE launch per step from t = max_len - 1 down to 0 and one more for d_h0.
// Stream order is the only dependency between steps -- no grid barrier, no spin wait, nothing persistent.  A workgroup
// owns LB_JT hidden units for every n at every step, so d_b and the carried dc are plain read-modify-writes: no atomics,
// the same bits on every run.  The product dh = dG_{t+1} w_hh (K = 4H) runs on v_mfma_f32_32x32x2_f32: gate gradients sit
// below fp16's normal range, where the hi + lo planes used elsewhere lose what the split exists to keep.  w_hh [4H, H] is
// contiguous in j, so a wave's B operand is 32 consecutive floats of a row, read as stored.
//
// ms_lstm_backward_steps_bidir is the same kernel on a (ceil(H / 32), 2) grid: blockIdx.y picks a direction's argument block,
// launch s serves t = max_len - 1 - s of the forward direction and t = s of the reverse one.  The two are independent, so a
// latency-bound loop of 2 (max_len + 1) launches becomes max_len + 1, with every promise above kept.
#include "common.h"

namespace ms {

int linear_launch(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act, float lo,
                  float hi, hipStream_t stream);   // gemm.hip: the kernel behind ms_linear_forward

constexpr int LB_JT = 32;      // hidden units per workgroup (one MFMA tile of columns)
constexpr int LB_NT = 32;      // batch rows per pass (one MFMA tile of rows); a workgroup walks ceil(N / 32) passes
constexpr int LB_WAVES = 8;    // the K = 4H extent is dealt to the waves in k-octets; partial tiles are added in wave order
constexpr int LB_THREADS = 64 * LB_WAVES;
constexpr int LB_ROWG = LB_THREADS / LB_JT;   // row groups of the elementwise phase: thread (unit, group) serves rows group + LB_ROWG i
constexpr int LB_PS = LB_JT + 1;

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ int seq_len(const int32_t* lens, int n, int T) {
  return lens ? min(max(lens[n], 0), T) : T;
}

// gates [T,N,4H] (activated) and c [T,N,H] for t < len[n]; rows past the length are left alone.  The scan visits a
// sequence's steps in the direction's own order: t = 0 .. len - 1, or (reverse) t = len - 1 .. 0.  p2 row t holds the product
// with the direction's previous output (h[t - 1], reverse h[t + 1]) and row `h0_row` (0, reverse T - 1: the one row that
// product leaves free) the product with h0, which the first step visited takes instead.
__global__ __launch_bounds__(256) void lstm_scan_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const float* __restrict__ b_hh, const float* __restrict__ c0,
                                                        const int32_t* __restrict__ lens, float* __restrict__ gates,
                                                        float* __restrict__ c, int T, int N, int H, int have_h0, int reverse) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * H) return;
  const int n = (int)(idx / H), j = (int)(idx % H);
  const int len = seq_len(lens, n, T);
  const int h0_row = reverse ? T - 1 : 0;
  float cprev = c0 ? c0[idx] : 0.f;
  for (int s = 0; s < len; ++s) {
    const int t = reverse ? len - 1 - s : s;
    const size_t base = ((size_t)t * N + n) * 4 * H + j;
    const size_t rbase = ((size_t)(s == 0 ? h0_row : t) * N + n) * 4 * H + j;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // (first step from a zero state: the recurrent product is 0 and only its bias remains)
      const float rec = (s == 0 && !have_h0) ? (b_hh ? b_hh[g * H + j] : 0.f) : p2[rbase + (size_t)g * H];
      pre[g] = p1[base + (size_t)g * H] + rec;
    }
    const float gi = sigmoid_exact(pre[0]), gf = sigmoid_exact(pre[1]), gg = tanhf(pre[2]), go = sigmoid_exact(pre[3]);
    const float cc = gf * cprev + gi * gg;
    gates[base] = gi;
    gates[base + (size_t)H] = gf;
    gates[base + (size_t)2 * H] = gg;
    gates[base + (size_t)3 * H] = go;
    c[((size_t)t * N + n) * H + j] = cc;
    cprev = cc;
  }
}

// One direction's share of a step launch.  Forward (reverse == 0) walks t downward and `dg_prev` is dG_{t+1}; reverse walks t
// upward and it is dG_{t-1}: in both it is the step the launch before this one wrote, or NULL at the first launch (nothing has
// flowed in yet).  t == -1 is the last launch: the product alone, written to d_h0.
struct LbDir {
  const float* gates;      // [T, N, 4H]
  const float* c;          // [T, N, H]
  const float* c0;         // [N, H] or NULL
  const float* w_hh;       // [4H, H]
  const float* d_out;      // this direction's first column of the output gradient; rows are `ldo` apart
  const float* d_hn;       // [N, H] or NULL
  const float* d_cn;       // [N, H] or NULL
  const float* dg_prev;    // [N, 4H] or NULL
  float* dG;               // [T, N, 4H]
  float* d_h0;             // [N, H]
  float* dc_buf;           // [N, H]: dc carried between the launches; what the last live step leaves is d_c0
  float* d_b;              // [4H]
  int t;
  int reverse;
};
struct LbStep {
  LbDir dir[2];            // blockIdx.y picks one
};

// One step of the backward recurrence for the directions of `step`.  grid = (ceil(H / LB_JT), directions).
__global__ __launch_bounds__(LB_THREADS) void lstm_bwd_step_kernel(const LbStep step, const int32_t* __restrict__ lens, int ldo,
                                                                   int T, int N, int H, int first) {
  __shared__ float part[LB_WAVES][LB_NT][LB_PS];
  __shared__ float red[LB_ROWG][4][LB_JT];
  const LbDir& d = step.dir[blockIdx.y];
  const float* __restrict__ gates = d.gates;
  const float* __restrict__ c = d.c;
  const float* __restrict__ c0 = d.c0;
  const float* __restrict__ w_hh = d.w_hh;
  const float* __restrict__ d_out = d.d_out;
  const float* __restrict__ d_hn = d.d_hn;
  const float* __restrict__ d_cn = d.d_cn;
  const float* __restrict__ dg_prev = d.dg_prev;
  float* __restrict__ dG = d.dG;
  float* __restrict__ d_h0 = d.d_h0;
  float* __restrict__ dc_buf = d.dc_buf;
  float* __restrict__ d_b = d.d_b;
  const int t = d.t, reverse = d.reverse;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int j0 = blockIdx.x * LB_JT;
  const size_t K4 = (size_t)4 * H;
  const int ej = j0 + (tid & 31);       // the unit this thread serves in the elementwise phase
  const int erow = tid >> 5;            // ... and its rows erow + LB_ROWG i of a pass
  // the reverse direction's d_h0 is the product with each sequence's OWN last row of dG
  const bool own_rows = reverse && t < 0;
  const bool product = dg_prev != nullptr || own_rows;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < N; r0 += LB_NT) {
    if (product) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int arow = r0 + l31;
      const int bcol = j0 + l31;
      const float* ap = nullptr;        // this lane's row of the A operand (NULL: a row of zeros)
      if (arow < N) {
        if (own_rows) {
          const int len = seq_len(lens, arow, T);
          if (len > 0) ap = dG + ((size_t)(len - 1) * N + arow) * K4;
        } else {
          ap = dg_prev + (size_t)arow * K4;
        }
      }
      const int noct = (H + 1) / 2;     // k-octets: 4H / 8 rounded up
      for (int q = wave; q < noct; q += LB_WAVES) {
        const int kq = 2 * q + half;    // this lane half's k-quad; quads exist for kq < H
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (kq < H) {
          if (ap != nullptr) a = *reinterpret_cast<const f32x4*>(ap + (size_t)4 * kq);
          if (bcol < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = w_hh[((size_t)4 * kq + e) * H + bcol];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) part[wave][mfma32_row(r, lane)][l31] = acc[r];
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < LB_NT / LB_ROWG; ++i) {
      const int rr = erow + LB_ROWG * i;
      const int n = r0 + rr;
      if (n >= N || ej >= H) continue;
      float dh = 0.f;
      if (product) {
#pragma unroll
        for (int w = 0; w < LB_WAVES; ++w) dh += part[w][rr][tid & 31];
      }
      const size_t nj = (size_t)n * H + ej;
      if (t < 0) {
        d_h0[nj] = dh;
        continue;
      }
      const int len = seq_len(lens, n, T);
      const size_t grow = ((size_t)t * N + n) * K4 + ej;
      if (t >= len) {
        dG[grow] = 0.f;
        dG[grow + (size_t)H] = 0.f;
        dG[grow + (size_t)2 * H] = 0.f;
        dG[grow + (size_t)3 * H] = 0.f;
        continue;
      }
      const size_t tnj = ((size_t)t * N + n) * H + ej;
      dh += d_out[((size_t)t * N + n) * ldo + ej];
      // the step at which the final states' gradients enter: the one the direction's forward ended on
      const bool last = reverse ? (t == 0) : (t == len - 1);
      if (last && d_hn) dh += d_hn[nj];
      float dc = last ? (d_cn ? d_cn[nj] : 0.f) : dc_buf[nj];
      const float gi = gates[grow], gf = gates[grow + (size_t)H], gg = gates[grow + (size_t)2 * H], go = gates[grow + (size_t)3 * H];
      float cprev;
      if (reverse) cprev = t + 1 < len ? c[tnj + (size_t)N * H] : (c0 ? c0[nj] : 0.f);
      else cprev = t > 0 ? c[tnj - (size_t)N * H] : (c0 ? c0[nj] : 0.f);
      const float tc = tanhf(c[tnj]);
      dc += dh * go * (1.f - tc * tc);
      const float dgi = dc * gg * gi * (1.f - gi);
      const float dgf = dc * cprev * gf * (1.f - gf);
      const float dgg = dc * gi * (1.f - gg * gg);
      const float dgo = dh * tc * go * (1.f - go);
      dc_buf[nj] = dc * gf;
      dG[grow] = dgi;
      dG[grow + (size_t)H] = dgf;
      dG[grow + (size_t)2 * H] = dgg;
      dG[grow + (size_t)3 * H] = dgo;
      bsum[0] += dgi;
      bsum[1] += dgf;
      bsum[2] += dgg;
      bsum[3] += dgo;
    }
    __syncthreads();      // the next pass rewrites `part`
  }
  if (t < 0) return;
  // column sums of this step's dG for the workgroup's units: row groups added in a fixed order, then the running d_b
#pragma unroll
  for (int g = 0; g < 4; ++g) red[erow][g][tid & 31] = bsum[g];
  __syncthreads();
  if (tid < 4 * LB_JT) {
    const int g = tid >> 5, jj = tid & 31;
    if (j0 + jj < H) {
      float s = red[0][g][jj];
#pragma unroll
      for (int r = 1; r < LB_ROWG; ++r) s += red[r][g][jj];
      const size_t o = (size_t)g * H + j0 + jj;
      d_b[o] = first ? s : d_b[o] + s;
    }
  }
}

// d_table[v, :] = sum over r with clamp(idx[r]) == v of d_out[r, :], in the order of r.  grid = V1.
__global__ __launch_bounds__(128) void embedding_backward_kernel(const float* __restrict__ d_out, const int32_t* __restrict__ idx,
                                                                 float* __restrict__ d_table, int R, int D, int V1) {
  const int v = blockIdx.x;
  for (int k = threadIdx.x; k < D; k += blockDim.x) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) {
      const int i = min(max(idx[r], 0), V1 - 1);      // embedding_kernel's rule (rnnt.hip)
      if (i == v) s += d_out[(size_t)r * D + k];
    }
    d_table[(size_t)v * D + k] = s;
  }
}

}  // namespace ms

extern "C" size_t ms_lstm_recompute_workspace_bytes(int T, int N, int H) {
  if (T <= 0 || N <= 0 || H <= 0) return 0;
  return 2 * ms::align_up((size_t)T * N * 4 * H * sizeof(float), 256);
}

extern "C" int ms_lstm_recompute_dir(const float* x, const float* h, const float* h0, const float* c0, const int32_t* lens,
                                     const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* gates,
                                     float* c, int T, int N, int In, int H, int reverse, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
  MS_REQUIRE(x && h && w_ih && w_hh && gates && c, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && In > 0 && H > 0, "bad shape");
  MS_REQUIRE(reverse == 0 || reverse == 1, "reverse must be 0 or 1");
  MS_REQUIRE((size_t)T * N < ((size_t)1 << 31) / 4 / (size_t)H, "T N 4H exceeds the GEMM's int extents");
  MS_REQUIRE(workspace != nullptr, "null workspace");
  if (workspace_bytes < ms_lstm_recompute_workspace_bytes(T, N, H)) {
    ms::set_error("ms_lstm_recompute: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t plane = ms::align_up((size_t)T * N * 4 * H * sizeof(float), 256) / sizeof(float);
  const size_t row = (size_t)N * 4 * H;
  float* p1 = (float*)workspace;
  float* p2 = p1 + plane;
  int rc = ms::linear_launch(x, w_ih, b_ih, p1, T * N, In, 4 * H, MS_ACT_NONE, 0.f, 0.f, st);
  if (rc != MS_OK) return rc;
  if (h0 != nullptr) {      // the row the shifted product below leaves free: 0, or T - 1 in the reverse direction
    rc = ms::linear_launch(h0, w_hh, b_hh, p2 + (reverse ? (size_t)(T - 1) * row : 0), N, H, 4 * H, MS_ACT_NONE, 0.f, 0.f, st);
    if (rc != MS_OK) return rc;
  }
  if (T > 1) {      // rows t >= 1 of the recurrent plane come from h[t - 1]; reverse: rows t <= T - 2 from h[t + 1]
    rc = ms::linear_launch(h + (reverse ? (size_t)N * H : 0), w_hh, b_hh, p2 + (reverse ? 0 : row), (T - 1) * N, H, 4 * H,
                           MS_ACT_NONE, 0.f, 0.f, st);
    if (rc != MS_OK) return rc;
  }
  const size_t cells = (size_t)N * H;
  hipLaunchKernelGGL(ms::lstm_scan_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p1, p2, b_hh, c0, lens, gates,
                     c, T, N, H, h0 != nullptr ? 1 : 0, reverse);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_lstm_recompute(const float* x, const float* h, const float* h0, const float* c0, const int32_t* lens,
                                 const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* gates,
                                 float* c, int T, int N, int In, int H, void* workspace, size_t workspace_bytes, void* stream_) {
  return ms_lstm_recompute_dir(x, h, h0, c0, lens, w_ih, w_hh, b_ih, b_hh, gates, c, T, N, In, H, 0, workspace, workspace_bytes,
                               stream_);
}

extern "C" int ms_lstm_backward_steps(const float* gates, const float* c, const float* c0, const float* w_hh,
                                      const float* d_out, const float* d_hn, const float* d_cn, const int32_t* lens,
                                      int max_len, float* dG, float* d_h0, float* d_c0, float* d_b, int T, int N, int H,
                                      void* stream_) {
  MS_REQUIRE(gates && c && w_hh && d_out && dG && d_h0 && d_c0 && d_b, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && H > 0, "bad shape");
  MS_REQUIRE(max_len >= 1 && max_len <= T, "max_len outside [1, T]");
  MS_REQUIRE(lens != nullptr || max_len == T, "without lens every sequence has T steps: max_len must be T");
  MS_REQUIRE(((uintptr_t)dG & 15) == 0, "dG must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  const size_t row = (size_t)N * 4 * H;
  if (max_len < T) MS_HIP(hipMemsetAsync(dG + (size_t)max_len * row, 0, (size_t)(T - max_len) * row * sizeof(float), st));
  const dim3 grid((unsigned)ms::cdiv(H, ms::LB_JT));
  ms::LbStep step = {};
  step.dir[0] = ms::LbDir{gates, c, c0, w_hh, d_out, d_hn, d_cn, nullptr, dG, d_h0, d_c0, d_b, 0, 0};
  for (int t = max_len - 1; t >= -1; --t) {
    const int first = (t == max_len - 1) ? 1 : 0;
    // (T == 1 or max_len == 1: the d_h0 launch follows the first step directly and still reads dG_0)
    step.dir[0].dg_prev = (first && t >= 0) ? nullptr : dG + (size_t)(t + 1) * row;
    step.dir[0].t = t;
    hipLaunchKernelGGL(ms::lstm_bwd_step_kernel, grid, dim3(ms::LB_THREADS), 0, st, step, lens, H, T, N, H, first);
  }
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_lstm_backward_steps_bidir(const float* gates, const float* c, const float* c0, const float* w_hh_fwd,
                                            const float* w_hh_rev, const float* d_out, const float* d_hn, const float* d_cn,
                                            const int32_t* lens, int max_len, float* dG, float* d_h0, float* d_c0, float* d_b,
                                            int T, int N, int H, void* stream_) {
  MS_REQUIRE(gates && c && w_hh_fwd && w_hh_rev && d_out && dG && d_h0 && d_c0 && d_b, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && H > 0, "bad shape");
  MS_REQUIRE(max_len >= 1 && max_len <= T, "max_len outside [1, T]");
  MS_REQUIRE(lens != nullptr || max_len == T, "without lens every sequence has T steps: max_len must be T");
  // (both halves of dG are read in 16-byte quads: T N 4H floats apart, so one test covers them)
  MS_REQUIRE(((uintptr_t)dG & 15) == 0, "dG must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  const size_t row = (size_t)N * 4 * H;
  const size_t nh = (size_t)N * H;
  const size_t plane = (size_t)T * row;       // one direction of gates / dG; c is plane / 4
  float* dG_rev = dG + plane;
  if (max_len < T) {
    const size_t bytes = (size_t)(T - max_len) * row * sizeof(float);
    MS_HIP(hipMemsetAsync(dG + (size_t)max_len * row, 0, bytes, st));
    MS_HIP(hipMemsetAsync(dG_rev + (size_t)max_len * row, 0, bytes, st));
  }
  const dim3 grid((unsigned)ms::cdiv(H, ms::LB_JT), 2);
  ms::LbStep step;
  step.dir[0] = ms::LbDir{gates, c, c0, w_hh_fwd, d_out, d_hn, d_cn, nullptr, dG, d_h0, d_c0, d_b, 0, 0};
  step.dir[1] = ms::LbDir{gates + plane, c + plane / 4, c0 ? c0 + nh : nullptr, w_hh_rev, d_out + H, d_hn ? d_hn + nh : nullptr,
                          d_cn ? d_cn + nh : nullptr, nullptr, dG_rev, d_h0 + nh, d_c0 + nh, d_b + (size_t)4 * H, 0, 1};
  // launch s: the forward direction's step max_len - 1 - s beside the reverse direction's step s; launch max_len: both d_h0
  for (int s = 0; s <= max_len; ++s) {
    const bool tail = s == max_len;
    step.dir[0].t = tail ? -1 : max_len - 1 - s;
    step.dir[1].t = tail ? -1 : s;
    step.dir[0].dg_prev = s == 0 ? nullptr : dG + (size_t)(max_len - s) * row;
    step.dir[1].dg_prev = s == 0 ? nullptr : dG_rev + (size_t)(s - 1) * row;      // (not read by the d_h0 launch: own rows)
    hipLaunchKernelGGL(ms::lstm_bwd_step_kernel, grid, dim3(ms::LB_THREADS), 0, st, step, lens, 2 * H, T, N, H, s == 0 ? 1 : 0);
  }
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_embedding_backward(const float* d_out, const int32_t* idx, float* d_table, int R, int D, int V1,
                                     void* stream) {
  MS_REQUIRE(d_out && idx && d_table, "null pointer");
  MS_REQUIRE(R > 0 && D > 0 && V1 > 0, "bad shape");
  hipLaunchKernelGGL(ms::embedding_backward_kernel, dim3(V1), dim3(128), 0, (hipStream_t)stream, d_out, idx, d_table, R, D, V1);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
