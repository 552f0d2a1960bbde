// Backward through time of one torch.nn.GRU layer, unidirectional or bidirectional (gate order r, z, n; weights in torch layout,
// no packed copy).  OWN specification: the comment on ms_gru_recompute in include/ms_hotpath.h; tests/gru_backward_ref.py
// restates it in float64 numpy, the reverse direction as the same cell walked from lens[n] - 1 down to 0.
//
// The forward kernels (rnn.hip) save no gates.  ms_gru_recompute rebuilds them from what the forward returns: every h_prev is
// known, so the pre-activations of ALL steps are two batch products over T*N rows on the exact float32 MFMA GEMM of gemm.hip,
// and ONE elementwise kernel over (t, n, j) applies the cell -- unlike the LSTM recompute nothing is carried, so there is no scan.
//
// ms_gru_backward_steps is the recurrence, modelled on lstm_backward.hip and keeping its promises: ONE launch per step and one
// more for d_h0, on a (ceil(H / 32), ndir) grid -- launch s serves t = max_len - 1 - s of direction 0 and t = s of the reverse
// direction.  Stream order is the only dependency between the launches: no grid barrier, no spin wait, nothing persistent.  A
// workgroup owns GB_JT hidden units for every n at every step, so the bias sums and the carried z dh are plain
// read-modify-writes: no atomics, the same bits on every run.  The product dGh w_hh (K = 3H) runs on v_mfma_f32_32x32x2_f32:
// gate gradients sit below fp16's normal range, so there are no split planes.  Two things differ from the LSTM kernel: 3H is a
// multiple of 4 only when H is, so a row of the A operand is read in 16-byte quads only where rows are that aligned (scalar
// loads otherwise) and the last k-quad may be partial -- its missing elements are zeros in registers, never loads; and the
// cell reads h_prev where the LSTM reads c_prev.
#include "common.h"

namespace ms {

int linear_launch(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act, float lo,
                  float hi, hipStream_t stream);   // gemm.hip: the kernel behind ms_linear_forward

constexpr int GB_JT = 32;      // hidden units per workgroup (one MFMA tile of columns)
constexpr int GB_NT = 32;      // batch rows per pass (one MFMA tile of rows); a workgroup walks ceil(N / 32) passes
constexpr int GB_WAVES = 8;    // the K = 3H extent is dealt to the waves in k-octets; partial tiles are added in wave order
constexpr int GB_THREADS = 64 * GB_WAVES;
constexpr int GB_ROWG = GB_THREADS / GB_JT;   // row groups of the elementwise phase: thread (unit, group) serves rows group + GB_ROWG i
constexpr int GB_PS = GB_JT + 1;

__device__ __forceinline__ float gru_sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ int gru_seq_len(const int32_t* lens, int n, int T) {
  return lens ? min(max(lens[n], 0), T) : T;
}

// gates [T,N,3H] (activated r, z, n) and q [T,N,H] = h_prev w_hn^T + b_hn for t < len[n]; rows past the length are left alone.
// p2 row t holds the product with the direction's previous output (h[t - 1], reverse h[t + 1]) and row `h0_row` (0, reverse
// T - 1: the one row that product leaves free) the product with h0, which the step a sequence starts on takes instead.
__global__ __launch_bounds__(256) void gru_cell_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                       const float* __restrict__ b_hh, const int32_t* __restrict__ lens,
                                                       float* __restrict__ gates, float* __restrict__ q, int T, int N, int H,
                                                       int have_h0, int reverse) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)T * N * H) return;
  const int j = (int)(idx % H);
  const size_t tn = idx / H;
  const int n = (int)(tn % N), t = (int)(tn / N);
  const int len = gru_seq_len(lens, n, T);
  if (t >= len) return;
  const bool start = reverse ? (t == len - 1) : (t == 0);
  const size_t base = tn * 3 * H + j;
  const size_t rbase = ((size_t)(start ? (reverse ? T - 1 : 0) : t) * N + n) * 3 * H + j;
  float rec[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    // (a start from a zero state: the recurrent product is 0 and only its bias remains)
    rec[g] = (start && !have_h0) ? (b_hh ? b_hh[g * H + j] : 0.f) : p2[rbase + (size_t)g * H];
  }
  const float r = gru_sigmoid_exact(p1[base] + rec[0]);
  const float z = gru_sigmoid_exact(p1[base + (size_t)H] + rec[1]);
  const float nn = tanhf(p1[base + (size_t)2 * H] + r * rec[2]);
  gates[base] = r;
  gates[base + (size_t)H] = z;
  gates[base + (size_t)2 * H] = nn;
  q[idx] = rec[2];
}

// One direction's share of a step launch.  Forward (reverse == 0) walks t downward and `dg_prev` is dGh_{t+1}; reverse walks t
// upward and it is dGh_{t-1}: in both it is the step the launch before this one wrote, or NULL at the first launch (nothing has
// flowed in yet).  t == -1 is the last launch: the carried z dh plus the product, written to d_h0.
struct GbDir {
  const float* gates;      // [T, N, 3H]
  const float* q;          // [T, N, H]
  const float* h;          // [T, N, H]: the direction's output (h_prev is read from it)
  const float* h0;         // [N, H] or NULL
  const float* w_hh;       // [3H, H]
  const float* d_out;      // this direction's first column of the output gradient; rows are `ldo` apart
  const float* d_hn;       // [N, H] or NULL
  const float* dg_prev;    // [N, 3H] or NULL
  float* dGi;              // [T, N, 3H]
  float* dGh;              // [T, N, 3H]
  float* d_h0;             // [N, H]: z dh carried between the launches; the last launch adds the product
  float* d_b_ih;           // [3H]
  float* d_b_hh;           // [3H]
  int t;
  int reverse;
  int vec;                 // rows of dGh are 16-byte aligned: the A operand is read in quads
};
struct GbStep {
  GbDir dir[2];            // blockIdx.y picks one
};

// One step of the backward recurrence for the directions of `step`.  grid = (ceil(H / GB_JT), directions).
__global__ __launch_bounds__(GB_THREADS) void gru_bwd_step_kernel(const GbStep step, const int32_t* __restrict__ lens, int ldo,
                                                                  int T, int N, int H, int first) {
  __shared__ float part[GB_WAVES][GB_NT][GB_PS];
  __shared__ float red[GB_ROWG][4][GB_JT];
  const GbDir& d = step.dir[blockIdx.y];
  const float* __restrict__ gates = d.gates;
  const float* __restrict__ qp = d.q;
  const float* __restrict__ h = d.h;
  const float* __restrict__ h0 = d.h0;
  const float* __restrict__ w_hh = d.w_hh;
  const float* __restrict__ d_out = d.d_out;
  const float* __restrict__ d_hn = d.d_hn;
  const float* __restrict__ dg_prev = d.dg_prev;
  float* __restrict__ dGi = d.dGi;
  float* __restrict__ dGh = d.dGh;
  float* __restrict__ d_h0 = d.d_h0;
  const int t = d.t, reverse = d.reverse, vec = d.vec;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int j0 = blockIdx.x * GB_JT;
  const int K3 = 3 * H;
  const int ej = j0 + (tid & 31);       // the unit this thread serves in the elementwise phase
  const int erow = tid >> 5;            // ... and its rows erow + GB_ROWG i of a pass
  // the reverse direction's d_h0 is the product with each sequence's OWN last row of dGh
  const bool own_rows = reverse && t < 0;
  const bool product = dg_prev != nullptr || own_rows;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < N; r0 += GB_NT) {
    if (product) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int arow = r0 + l31;
      const int bcol = j0 + l31;
      const float* ap = nullptr;        // this lane's row of the A operand (NULL: a row of zeros)
      if (arow < N) {
        if (own_rows) {
          const int len = gru_seq_len(lens, arow, T);
          if (len > 0) ap = dGh + ((size_t)(len - 1) * N + arow) * K3;
        } else {
          ap = dg_prev + (size_t)arow * K3;
        }
      }
      const int nquad = (K3 + 3) / 4;   // k-quads; the last one is partial when 3H is no multiple of 4
      const int noct = (nquad + 1) / 2;
      for (int o = wave; o < noct; o += GB_WAVES) {
        const int k0 = 4 * (2 * o + half);      // this lane half's k-quad
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (k0 < K3) {
          if (ap != nullptr) {
            if (vec && k0 + 3 < K3) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(ap + k0);
              a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) if (k0 + e < K3) a[e] = ap[k0 + e];
            }
          }
          if (bcol < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (k0 + e < K3) b[e] = w_hh[(size_t)(k0 + e) * H + bcol];
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
    for (int i = 0; i < GB_NT / GB_ROWG; ++i) {
      const int rr = erow + GB_ROWG * i;
      const int n = r0 + rr;
      if (n >= N || ej >= H) continue;
      float dh = 0.f;
      if (product) {
#pragma unroll
        for (int w = 0; w < GB_WAVES; ++w) dh += part[w][rr][tid & 31];
      }
      const size_t nj = (size_t)n * H + ej;
      const int len = gru_seq_len(lens, n, T);
      if (t < 0) {
        d_h0[nj] = len > 0 ? d_h0[nj] + dh : 0.f;
        continue;
      }
      const size_t grow = ((size_t)t * N + n) * K3 + ej;
      if (t >= len) {
        dGi[grow] = 0.f;
        dGi[grow + (size_t)H] = 0.f;
        dGi[grow + (size_t)2 * H] = 0.f;
        dGh[grow] = 0.f;
        dGh[grow + (size_t)H] = 0.f;
        dGh[grow + (size_t)2 * H] = 0.f;
        continue;
      }
      const size_t tnj = ((size_t)t * N + n) * H + ej;
      dh += d_out[((size_t)t * N + n) * ldo + ej];
      // the step at which the final state's gradient enters and nothing is carried in: the one the direction's forward ended on
      const bool last = reverse ? (t == 0) : (t == len - 1);
      dh += last ? (d_hn ? d_hn[nj] : 0.f) : d_h0[nj];
      const float gr = gates[grow], gz = gates[grow + (size_t)H], gn = gates[grow + (size_t)2 * H];
      const float qv = qp[tnj];
      float hprev;
      if (reverse) hprev = t + 1 < len ? h[tnj + (size_t)N * H] : (h0 ? h0[nj] : 0.f);
      else hprev = t > 0 ? h[tnj - (size_t)N * H] : (h0 ? h0[nj] : 0.f);
      const float omz = 1.f - gz;
      const float da_n = dh * omz * (1.f - gn * gn);
      const float da_z = dh * (hprev - gn) * gz * omz;
      const float da_r = da_n * qv * gr * (1.f - gr);
      const float da_nr = da_n * gr;
      d_h0[nj] = dh * gz;
      dGi[grow] = da_r;
      dGi[grow + (size_t)H] = da_z;
      dGi[grow + (size_t)2 * H] = da_n;
      dGh[grow] = da_r;
      dGh[grow + (size_t)H] = da_z;
      dGh[grow + (size_t)2 * H] = da_nr;
      bsum[0] += da_r;
      bsum[1] += da_z;
      bsum[2] += da_n;
      bsum[3] += da_nr;
    }
    __syncthreads();      // the next pass rewrites `part`
  }
  if (t < 0) return;
  // column sums of this step's dGi / dGh for the workgroup's units: row groups added in a fixed order, then the running sums
#pragma unroll
  for (int g = 0; g < 4; ++g) red[erow][g][tid & 31] = bsum[g];
  __syncthreads();
  if (tid < 4 * GB_JT) {
    const int g = tid >> 5, jj = tid & 31;
    if (j0 + jj < H) {
      float s = red[0][g][jj];
#pragma unroll
      for (int r = 1; r < GB_ROWG; ++r) s += red[r][g][jj];
      const size_t u = (size_t)j0 + jj;
      // sums 0, 1 (r, z) belong to both biases, 2 to b_ih's n block, 3 (da_n r) to b_hh's
      if (g < 3) {
        const size_t o = (size_t)g * H + u;
        d.d_b_ih[o] = first ? s : d.d_b_ih[o] + s;
      }
      if (g != 2) {
        const size_t o = (size_t)(g == 3 ? 2 : g) * H + u;
        d.d_b_hh[o] = first ? s : d.d_b_hh[o] + s;
      }
    }
  }
}

}  // namespace ms

extern "C" size_t ms_gru_recompute_workspace_bytes(int T, int N, int H) {
  if (T <= 0 || N <= 0 || H <= 0) return 0;
  return 2 * ms::align_up((size_t)T * N * 3 * H * sizeof(float), 256);
}

extern "C" int ms_gru_recompute(const float* x, const float* h, const float* h0, const int32_t* lens, const float* w_ih,
                                const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* q, int T, int N,
                                int In, int H, int reverse, void* workspace, size_t workspace_bytes, void* stream_) {
  MS_REQUIRE(x && h && w_ih && w_hh && gates && q, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && In > 0 && H > 0, "bad shape");
  MS_REQUIRE(reverse == 0 || reverse == 1, "reverse must be 0 or 1");
  MS_REQUIRE((size_t)T * N < ((size_t)1 << 31) / 3 / (size_t)H, "T N 3H exceeds the GEMM's int extents");
  MS_REQUIRE(workspace != nullptr, "null workspace");
  if (workspace_bytes < ms_gru_recompute_workspace_bytes(T, N, H)) {
    ms::set_error("ms_gru_recompute: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t plane = ms::align_up((size_t)T * N * 3 * H * sizeof(float), 256) / sizeof(float);
  const size_t row = (size_t)N * 3 * H;
  float* p1 = (float*)workspace;
  float* p2 = p1 + plane;
  int rc = ms::linear_launch(x, w_ih, b_ih, p1, T * N, In, 3 * H, MS_ACT_NONE, 0.f, 0.f, st);
  if (rc != MS_OK) return rc;
  if (h0 != nullptr) {      // the row the shifted product below leaves free: 0, or T - 1 in the reverse direction
    rc = ms::linear_launch(h0, w_hh, b_hh, p2 + (reverse ? (size_t)(T - 1) * row : 0), N, H, 3 * H, MS_ACT_NONE, 0.f, 0.f, st);
    if (rc != MS_OK) return rc;
  }
  if (T > 1) {      // rows t >= 1 of the recurrent plane come from h[t - 1]; reverse: rows t <= T - 2 from h[t + 1]
    rc = ms::linear_launch(h + (reverse ? (size_t)N * H : 0), w_hh, b_hh, p2 + (reverse ? 0 : row), (T - 1) * N, H, 3 * H,
                           MS_ACT_NONE, 0.f, 0.f, st);
    if (rc != MS_OK) return rc;
  }
  const size_t cells = (size_t)T * N * H;
  hipLaunchKernelGGL(ms::gru_cell_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p1, p2, b_hh, lens, gates, q, T,
                     N, H, h0 != nullptr ? 1 : 0, reverse);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_gru_backward_steps(const float* gates, const float* q, const float* h, const float* h0, const float* w_hh_fwd,
                                     const float* w_hh_rev, const float* d_out, const float* d_hn, const int32_t* lens,
                                     int max_len, float* dGi, float* dGh, float* d_h0, float* d_b_ih, float* d_b_hh, int T, int N,
                                     int H, int ndir, void* stream_) {
  MS_REQUIRE(ndir == 1 || ndir == 2, "ndir must be 1 or 2");
  MS_REQUIRE(gates && q && h && w_hh_fwd && d_out && dGi && dGh && d_h0 && d_b_ih && d_b_hh, "null pointer");
  MS_REQUIRE(ndir == 1 || w_hh_rev != nullptr, "null w_hh_rev with ndir == 2");
  MS_REQUIRE(T > 0 && N > 0 && H > 0, "bad shape");
  MS_REQUIRE((size_t)T * N < ((size_t)1 << 31) / 3 / (size_t)H, "T N 3H exceeds the int extents");
  MS_REQUIRE(max_len >= 1 && max_len <= T, "max_len outside [1, T]");
  MS_REQUIRE(lens != nullptr || max_len == T, "without lens every sequence has T steps: max_len must be T");
  hipStream_t st = (hipStream_t)stream_;
  const size_t row = (size_t)N * 3 * H;
  const size_t nh = (size_t)N * H;
  const size_t plane = (size_t)T * row;       // one direction of gates / dGi / dGh; q and h are plane / 3
  if (max_len < T) {
    const size_t bytes = (size_t)(T - max_len) * row * sizeof(float);
    for (int d = 0; d < ndir; ++d) {
      MS_HIP(hipMemsetAsync(dGi + d * plane + (size_t)max_len * row, 0, bytes, st));
      MS_HIP(hipMemsetAsync(dGh + d * plane + (size_t)max_len * row, 0, bytes, st));
    }
  }
  // (a direction's plane starts T N 3H floats after the first: with H % 4 == 0 one alignment test covers both)
  const int vec = (H % 4 == 0 && ((uintptr_t)dGh & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)ms::cdiv(H, ms::GB_JT), (unsigned)ndir);
  ms::GbStep step = {};
  step.dir[0] = ms::GbDir{gates, q, h, h0, w_hh_fwd, d_out, d_hn, nullptr, dGi, dGh, d_h0, d_b_ih, d_b_hh, 0, 0, vec};
  if (ndir == 2) {
    step.dir[1] = ms::GbDir{gates + plane, q + plane / 3, h + plane / 3, h0 ? h0 + nh : nullptr, w_hh_rev, d_out + H,
                            d_hn ? d_hn + nh : nullptr, nullptr, dGi + plane, dGh + plane, d_h0 + nh, d_b_ih + (size_t)3 * H,
                            d_b_hh + (size_t)3 * H, 0, 1, vec};
  }
  // launch s: the forward direction's step max_len - 1 - s beside the reverse direction's step s; launch max_len: the d_h0 products
  for (int s = 0; s <= max_len; ++s) {
    const bool tail = s == max_len;
    step.dir[0].t = tail ? -1 : max_len - 1 - s;
    step.dir[1].t = tail ? -1 : s;
    step.dir[0].dg_prev = s == 0 ? nullptr : dGh + (size_t)(max_len - s) * row;
    // (not read by the d_h0 launch: own rows)
    step.dir[1].dg_prev = (s == 0 || ndir == 1) ? nullptr : dGh + plane + (size_t)(s - 1) * row;
    hipLaunchKernelGGL(ms::gru_bwd_step_kernel, grid, dim3(ms::GB_THREADS), 0, st, step, lens, ndir * H, T, N, H, s == 0 ? 1 : 0);
  }
  MS_LAUNCH_CHECK();
  return MS_OK;
}
