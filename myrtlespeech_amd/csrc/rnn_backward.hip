// Backward through time of one torch.nn.LSTM layer (gate order i, f, g, o) or one torch.nn.GRU layer (r, z, n), unidirectional
// or bidirectional, weights in torch layout and read as stored (no packed copy).  OWN specification: the comments on
// ms_lstm_recompute and ms_gru_recompute in include/ms_hotpath.h; tests/lstm_backward_ref.py, tests/bilstm_backward_ref.py and
// tests/gru_backward_ref.py restate it in float64 numpy, the reverse direction as the same cell walked from lens[n] - 1 down to 0.
//
// The forward kernels (rnn.hip) save no gates.  ms_lstm_recompute[_dir] / ms_gru_recompute rebuild them from what the forward
// returns: every h_prev is known, so the pre-activations of ALL steps are two batch products over T*N rows on the exact float32
// MFMA GEMM of gemm.hip (recompute_products), and one elementwise kernel applies the cell.  The LSTM's is a scan (one thread per
// (n, j), c in a register); the GRU carries nothing, so its kernel runs over (t, n, j).
//
// ms_lstm_backward_steps[_bidir] / ms_gru_backward_steps are the recurrence: ONE launch of rnn_bwd_step_kernel per step and one
// more for d_h0, on a (ceil(H / 32), ndir) grid -- launch s serves t = max_len - 1 - s of direction 0 and t = s of the reverse
// direction, which are independent.  Stream order is the only dependency between the launches: no grid barrier, no spin wait,
// nothing persistent.  A workgroup owns RB_JT hidden units for every n at every step, so the bias sums and the state carried
// between the launches (the LSTM's dc, the GRU's z dh) are plain read-modify-writes: no atomics, the same bits on every run.
// The product dh = dG_prev w_hh (K = G H, G = 4 or 3 gates) runs on v_mfma_f32_32x32x2_f32: gate gradients sit below fp16's
// normal range, where the hi + lo planes used elsewhere lose what the split exists to keep.  w_hh [G H, H] is contiguous in j,
// so a wave's B operand is 32 consecutive floats of a row, read as stored.  The kernel is one template around a cell policy
// (LstmCell, GruCell, HardLstmCell): the policy holds the cell's arithmetic and its argument block, the template everything else.
// ms_hard_lstm_recompute / ms_hard_lstm_backward_steps are HardLSTM's pair (hard sigmoid / hard tanh, no lengths): the same
// products, a scan that keeps the PRE-CLAMP gate values, and the step kernel around HardLstmCell (tests/hard_lstm_backward_ref.py).
#include "common.h"

namespace ms {

int linear_launch(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act, float lo,
                  float hi, hipStream_t stream);   // gemm.hip: the kernel behind ms_linear_forward

constexpr int RB_JT = 32;      // hidden units per workgroup (one MFMA tile of columns)
constexpr int RB_NT = 32;      // batch rows per pass (one MFMA tile of rows); a workgroup walks ceil(N / 32) passes
constexpr int RB_WAVES = 8;    // the K = G H extent is dealt to the waves in k-octets; partial tiles are added in wave order
constexpr int RB_THREADS = 64 * RB_WAVES;
constexpr int RB_ROWG = RB_THREADS / RB_JT;   // row groups of the elementwise phase: thread (unit, group) serves rows group + RB_ROWG i
constexpr int RB_PS = RB_JT + 1;

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ int seq_len(const int32_t* lens, int n, int T) {
  return lens ? min(max(lens[n], 0), T) : T;
}

// ---- recompute ----------------------------------------------------------------------------------------------------------------

static size_t recompute_plane_bytes(int G, int T, int N, int H) { return align_up((size_t)T * N * G * H * sizeof(float), 256); }

// The two pre-activation planes of a direction, [T N, G H] each (the halves of the workspace): p1 = x w_ih^T + b_ih, and p2 whose row t holds
// the product with the direction's previous output (h[t - 1], reverse h[t + 1]) and whose row `h0_row` (0, reverse T - 1: the
// one row that product leaves free) holds the product with h0, which the step a sequence starts on takes instead.
static int recompute_products(int G, const float* x, const float* h, const float* h0, const float* w_ih, const float* w_hh,
                              const float* b_ih, const float* b_hh, int T, int N, int In, int H, int reverse,
                              float* p1, float* p2, hipStream_t st) {
  const size_t row = (size_t)N * G * H;
  int rc = linear_launch(x, w_ih, b_ih, p1, T * N, In, G * H, MS_ACT_NONE, 0.f, 0.f, st);
  if (rc != MS_OK) return rc;
  if (h0 != nullptr) {
    rc = linear_launch(h0, w_hh, b_hh, p2 + (reverse ? (size_t)(T - 1) * row : 0), N, H, G * H, MS_ACT_NONE, 0.f, 0.f, st);
    if (rc != MS_OK) return rc;
  }
  if (T > 1) {      // rows t >= 1 of the recurrent plane come from h[t - 1]; reverse: rows t <= T - 2 from h[t + 1]
    rc = linear_launch(h + (reverse ? (size_t)N * H : 0), w_hh, b_hh, p2 + (reverse ? 0 : row), (T - 1) * N, H, G * H, MS_ACT_NONE,
                       0.f, 0.f, st);
  }
  return rc;
}

// gates [T,N,4H] (activated) and c [T,N,H] for t < len[n]; rows past the length are left alone.  The scan visits a
// sequence's steps in the direction's own order: t = 0 .. len - 1, or (reverse) t = len - 1 .. 0; the first step visited takes
// p2's `h0_row`.
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

// The hard cell's pre-clamp gate value fl(fl(0.2f a) + 0.5f): TWO roundings, as the reference's two torch ops make them.  Two
// statements, so the build (which contracts inside one expression only) cannot fuse them: at a = -2.5 the fused form is
// -7.45e-9, outside the clamp, where the two-op form is exactly 0, inside it -- and the backward's gate is decided there.
__device__ __forceinline__ float hard_pre(float a) {
  const float m = 0.2f * a;
  return m + 0.5f;
}

// The hard cell (HardLSTM: no lengths, every sequence has T steps).  gates [T,N,4H] holds the PRE-CLAMP values z_i, z_f, a_g, z_o
// -- the activated gate does not say whether a 0 came from exactly 0 (gradient passes) or from below (it does not) -- and c
// [T,N,H] the unclamped cell state.  Steps in the direction's own order, the first one visited takes p2's `h0_row`.
__global__ __launch_bounds__(256) void hard_lstm_scan_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                             const float* __restrict__ b_hh, const float* __restrict__ c0,
                                                             float* __restrict__ gates, float* __restrict__ c, int T, int N, int H,
                                                             int have_h0, int reverse) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * H) return;
  const int n = (int)(idx / H), j = (int)(idx % H);
  const int h0_row = reverse ? T - 1 : 0;
  float cprev = c0 ? c0[idx] : 0.f;
  for (int s = 0; s < T; ++s) {
    const int t = reverse ? T - 1 - s : s;
    const size_t base = ((size_t)t * N + n) * 4 * H + j;
    const size_t rbase = ((size_t)(s == 0 ? h0_row : t) * N + n) * 4 * H + j;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // (first step from a zero state: the recurrent product is 0 and only its bias remains)
      const float rec = (s == 0 && !have_h0) ? (b_hh ? b_hh[g * H + j] : 0.f) : p2[rbase + (size_t)g * H];
      pre[g] = p1[base + (size_t)g * H] + rec;
    }
    const float zi = hard_pre(pre[0]), zf = hard_pre(pre[1]), ag = pre[2], zo = hard_pre(pre[3]);
    const float cc = act_clamp(zf, 0.f, 1.f) * cprev + act_clamp(zi, 0.f, 1.f) * act_clamp(ag, -1.f, 1.f);
    gates[base] = zi;
    gates[base + (size_t)H] = zf;
    gates[base + (size_t)2 * H] = ag;
    gates[base + (size_t)3 * H] = zo;
    c[((size_t)t * N + n) * H + j] = cc;
    cprev = cc;
  }
}

// gates [T,N,3H] (activated r, z, n) and q [T,N,H] = h_prev w_hn^T + b_hn for t < len[n]; rows past the length are left alone.
// The step a sequence starts on (t = 0, reverse t = len - 1) takes p2's `h0_row`.
__global__ __launch_bounds__(256) void gru_cell_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                       const float* __restrict__ b_hh, const int32_t* __restrict__ lens,
                                                       float* __restrict__ gates, float* __restrict__ q, int T, int N, int H,
                                                       int have_h0, int reverse) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)T * N * H) return;
  const int j = (int)(idx % H);
  const size_t tn = idx / H;
  const int n = (int)(tn % N), t = (int)(tn / N);
  const int len = seq_len(lens, n, T);
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
  const float r = sigmoid_exact(p1[base] + rec[0]);
  const float z = sigmoid_exact(p1[base + (size_t)H] + rec[1]);
  const float nn = tanhf(p1[base + (size_t)2 * H] + r * rec[2]);
  gates[base] = r;
  gates[base + (size_t)H] = z;
  gates[base + (size_t)2 * H] = nn;
  q[idx] = rec[2];
}

// ---- the step kernel ----------------------------------------------------------------------------------------------------------

// What every cell's share of a step launch holds, per direction.  Forward (reverse == 0) walks t downward and `dg_prev` is the
// product plane's row t + 1; reverse walks t upward and it is row t - 1: in both it is the step the launch before this one
// wrote, or NULL at the first launch (nothing has flowed in yet).  t == -1 is the last launch: the product alone, for d_h0.
struct RbDir {
  const float* gates;      // [T, N, G H]
  const float* w_hh;       // [G H, H]
  const float* d_out;      // this direction's first column of the output gradient; rows are `ldo` apart
  const float* d_hn;       // [N, H] or NULL
  const float* dg_prev;    // [N, G H] or NULL
  float* dgh;              // [T, N, G H]: the gate gradients the product reads (the LSTM's dG, the GRU's dGh)
  float* d_h0;             // [N, H]
  int t;
  int reverse;
  int vec;                 // rows of dgh are 16-byte aligned: the A operand is read in quads (always, where G H is a multiple of 4)
};

// A cell policy supplies G, its argument block `Dir` (RbDir and what only this cell reads and writes) and, for the element
// (n, unit) a thread serves -- nj = n H + unit, grow = its first gate's place in a [T, N, G H] plane, tnj in a [T, N, H] one --
//   tail      the last launch (t == -1): d_h0 from the product dh
//   zero_row  a row past its sequence's length: exact zeros in every gate-gradient plane
//   live_row  a live row: the cell's backward from dh = product + d_out, writing the gate gradients and the carried state and
//             adding the row to the four column sums `bsum`
//   store_sum column sum g of unit u, into the running bias gradients
// Each arithmetic statement stands as one expression: the build contracts a * b + c inside an expression only.

struct LstmCell {
  static constexpr int G = 4;
  struct Dir : RbDir {
    const float* c;          // [T, N, H]
    const float* c0;         // [N, H] or NULL
    const float* d_cn;       // [N, H] or NULL
    float* dc_buf;           // [N, H]: dc carried between the launches; what the last live step leaves is d_c0
    float* d_b;              // [4H]
  };

  __device__ __forceinline__ static void tail(const Dir& d, size_t nj, int, float dh) { d.d_h0[nj] = dh; }

  __device__ __forceinline__ static void zero_row(const Dir& d, size_t grow, int H) {
    float* __restrict__ dG = d.dgh;
    dG[grow] = 0.f;
    dG[grow + (size_t)H] = 0.f;
    dG[grow + (size_t)2 * H] = 0.f;
    dG[grow + (size_t)3 * H] = 0.f;
  }

  __device__ __forceinline__ static void live_row(const Dir& d, float dh, bool last, int len, size_t grow, size_t tnj, size_t nj,
                                                  int N, int H, float (&bsum)[4]) {
    const float* __restrict__ gates = d.gates;
    const float* __restrict__ c = d.c;
    const float* __restrict__ c0 = d.c0;
    const float* __restrict__ d_hn = d.d_hn;
    const float* __restrict__ d_cn = d.d_cn;
    float* __restrict__ dG = d.dgh;
    float* __restrict__ dc_buf = d.dc_buf;
    const int t = d.t;
    if (last && d_hn) dh += d_hn[nj];
    float dc = last ? (d_cn ? d_cn[nj] : 0.f) : dc_buf[nj];
    const float gi = gates[grow], gf = gates[grow + (size_t)H], gg = gates[grow + (size_t)2 * H], go = gates[grow + (size_t)3 * H];
    float cprev;
    if (d.reverse) cprev = t + 1 < len ? c[tnj + (size_t)N * H] : (c0 ? c0[nj] : 0.f);
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

  __device__ __forceinline__ static void store_sum(const Dir& d, int g, size_t u, int H, float s, int first) {
    const size_t o = (size_t)g * H + u;
    d.d_b[o] = first ? s : d.d_b[o] + s;
  }
};

// The hard cell against the LSTM: `gates` holds the pre-clamp values (hard_lstm_scan_kernel), from which both the gate's value
// and its derivative's gate come.  P (torch.clamp: the CLOSED interval passes) and Q (torch.nn.Hardtanh: the OPEN one) are
// selects, never multiplies by 0 or 1, and a NaN compares false.  The statements follow torch autograd's own operations one
// rounding each -- a product, the select, then the hard sigmoid's 0.2 -- so nothing here is contracted.
struct HardLstmCell : LstmCell {
  __device__ __forceinline__ static void live_row(const Dir& d, float dh, bool last, int len, size_t grow, size_t tnj, size_t nj,
                                                  int N, int H, float (&bsum)[4]) {
    const float* __restrict__ gates = d.gates;
    const float* __restrict__ c = d.c;
    const float* __restrict__ c0 = d.c0;
    const float* __restrict__ d_hn = d.d_hn;
    const float* __restrict__ d_cn = d.d_cn;
    float* __restrict__ dG = d.dgh;
    float* __restrict__ dc_buf = d.dc_buf;
    const int t = d.t;
    if (last && d_hn) dh += d_hn[nj];
    float dc = last ? (d_cn ? d_cn[nj] : 0.f) : dc_buf[nj];
    const float zi = gates[grow], zf = gates[grow + (size_t)H], ag = gates[grow + (size_t)2 * H], zo = gates[grow + (size_t)3 * H];
    float cprev;
    if (d.reverse) cprev = t + 1 < len ? c[tnj + (size_t)N * H] : (c0 ? c0[nj] : 0.f);
    else cprev = t > 0 ? c[tnj - (size_t)N * H] : (c0 ? c0[nj] : 0.f);
    const float cc = c[tnj];
    const float gi = act_clamp(zi, 0.f, 1.f), gf = act_clamp(zf, 0.f, 1.f), gg = act_clamp(ag, -1.f, 1.f);
    const float go = act_clamp(zo, 0.f, 1.f), tc = act_clamp(cc, -1.f, 1.f);
    const bool p_i = zi >= 0.f && zi <= 1.f, p_f = zf >= 0.f && zf <= 1.f, p_o = zo >= 0.f && zo <= 1.f;
    const bool q_g = ag > -1.f && ag < 1.f, q_c = cc > -1.f && cc < 1.f;
    const float dtc = dh * go;
    const float dcs = q_c ? dtc : 0.f;
    dc = dc + dcs;
    const float di = dc * gg;
    const float df = dc * cprev;
    const float dg = dc * gi;
    const float dO = dh * tc;
    const float dgi = p_i ? di * 0.2f : 0.f;
    const float dgf = p_f ? df * 0.2f : 0.f;
    const float dgg = q_g ? dg : 0.f;
    const float dgo = p_o ? dO * 0.2f : 0.f;
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
};

// The GRU against the LSTM: 3H is a multiple of 4 only when H is, so the product's last k-quad may be partial and its rows
// unaligned (RbDir::vec); the cell reads h_prev where the LSTM reads c_prev; d_h0 itself carries z dh between the launches and
// the last launch adds the product.
struct GruCell {
  static constexpr int G = 3;
  struct Dir : RbDir {
    const float* q;          // [T, N, H]
    const float* h;          // [T, N, H]: the direction's output (h_prev is read from it)
    const float* h0;         // [N, H] or NULL
    float* dGi;              // [T, N, 3H]
    float* d_b_ih;           // [3H]
    float* d_b_hh;           // [3H]
  };

  __device__ __forceinline__ static void tail(const Dir& d, size_t nj, int len, float dh) {
    d.d_h0[nj] = len > 0 ? d.d_h0[nj] + dh : 0.f;
  }

  __device__ __forceinline__ static void zero_row(const Dir& d, size_t grow, int H) {
    float* __restrict__ dGi = d.dGi;
    float* __restrict__ dGh = d.dgh;
    dGi[grow] = 0.f;
    dGi[grow + (size_t)H] = 0.f;
    dGi[grow + (size_t)2 * H] = 0.f;
    dGh[grow] = 0.f;
    dGh[grow + (size_t)H] = 0.f;
    dGh[grow + (size_t)2 * H] = 0.f;
  }

  __device__ __forceinline__ static void live_row(const Dir& d, float dh, bool last, int len, size_t grow, size_t tnj, size_t nj,
                                                  int N, int H, float (&bsum)[4]) {
    const float* __restrict__ gates = d.gates;
    const float* __restrict__ qp = d.q;
    const float* __restrict__ h = d.h;
    const float* __restrict__ h0 = d.h0;
    const float* __restrict__ d_hn = d.d_hn;
    float* __restrict__ dGi = d.dGi;
    float* __restrict__ dGh = d.dgh;
    float* __restrict__ d_h0 = d.d_h0;
    const int t = d.t;
    // (at the step the direction's forward ended on nothing is carried in)
    dh += last ? (d_hn ? d_hn[nj] : 0.f) : d_h0[nj];
    const float gr = gates[grow], gz = gates[grow + (size_t)H], gn = gates[grow + (size_t)2 * H];
    const float qv = qp[tnj];
    float hprev;
    if (d.reverse) hprev = t + 1 < len ? h[tnj + (size_t)N * H] : (h0 ? h0[nj] : 0.f);
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

  // sums 0, 1 (r, z) belong to both biases, 2 to b_ih's n block, 3 (da_n r) to b_hh's
  __device__ __forceinline__ static void store_sum(const Dir& d, int g, size_t u, int H, float s, int first) {
    if (g < 3) {
      const size_t o = (size_t)g * H + u;
      d.d_b_ih[o] = first ? s : d.d_b_ih[o] + s;
    }
    if (g != 2) {
      const size_t o = (size_t)(g == 3 ? 2 : g) * H + u;
      d.d_b_hh[o] = first ? s : d.d_b_hh[o] + s;
    }
  }
};

template <class Cell>
struct RbStep {
  typename Cell::Dir dir[2];      // blockIdx.y picks one
};

// One step of the backward recurrence for the directions of `step`.  grid = (ceil(H / RB_JT), directions).
template <class Cell>
__global__ __launch_bounds__(RB_THREADS) void rnn_bwd_step_kernel(const RbStep<Cell> step, const int32_t* __restrict__ lens, int ldo,
                                                                  int T, int N, int H, int first) {
  __shared__ float part[RB_WAVES][RB_NT][RB_PS];
  __shared__ float red[RB_ROWG][4][RB_JT];
  // K = G H a multiple of 4 for every H: each k-quad is whole and (the entry refuses an unaligned plane) one 16-byte load
  constexpr bool whole = Cell::G % 4 == 0;
  const typename Cell::Dir& d = step.dir[blockIdx.y];
  const float* __restrict__ w_hh = d.w_hh;
  const float* __restrict__ d_out = d.d_out;
  const float* __restrict__ dg_prev = d.dg_prev;
  const int t = d.t, reverse = d.reverse, vec = d.vec;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int j0 = blockIdx.x * RB_JT;
  const int K = Cell::G * H;
  const int ej = j0 + (tid & 31);       // the unit this thread serves in the elementwise phase
  const int erow = tid >> 5;            // ... and its rows erow + RB_ROWG i of a pass
  // the reverse direction's d_h0 is the product with each sequence's OWN last row of the plane
  const bool own_rows = reverse && t < 0;
  const bool product = dg_prev != nullptr || own_rows;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < N; r0 += RB_NT) {
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
          if (len > 0) ap = d.dgh + ((size_t)(len - 1) * N + arow) * K;
        } else {
          ap = dg_prev + (size_t)arow * K;
        }
      }
      const int nquad = (K + 3) / 4;    // k-quads; the last one is partial when K is no multiple of 4
      const int noct = (nquad + 1) / 2;
      for (int o = wave; o < noct; o += RB_WAVES) {
        const int kq = 2 * o + half;            // this lane half's k-quad; quads exist for kq < nquad
        const int ke = 4 * kq;                  // its first element: the bounds of a partial quad are tested on ints,
        const size_t k0 = (size_t)4 * kq;       // the addresses are formed from size_t (pointers the loop increments)
        float a[4] = {0.f, 0.f, 0.f, 0.f};      // (what a partial quad lacks stays zero in registers, never a load)
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (kq < nquad) {
          if (ap != nullptr) {
            if (whole || (vec && ke + 3 < K)) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(ap + k0);
              a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) if (ke + e < K) a[e] = ap[k0 + e];
            }
          }
          if (bcol < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (whole || ke + e < K) b[e] = w_hh[(k0 + e) * H + bcol];
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
    for (int i = 0; i < RB_NT / RB_ROWG; ++i) {
      const int rr = erow + RB_ROWG * i;
      const int n = r0 + rr;
      if (n >= N || ej >= H) continue;
      float dh = 0.f;
      if (product) {
#pragma unroll
        for (int w = 0; w < RB_WAVES; ++w) dh += part[w][rr][tid & 31];
      }
      const size_t nj = (size_t)n * H + ej;
      const int len = seq_len(lens, n, T);
      if (t < 0) {
        Cell::tail(d, nj, len, dh);
        continue;
      }
      const size_t grow = ((size_t)t * N + n) * K + ej;
      if (t >= len) {
        Cell::zero_row(d, grow, H);
        continue;
      }
      const size_t tnj = ((size_t)t * N + n) * H + ej;
      dh += d_out[((size_t)t * N + n) * ldo + ej];
      // the step at which the final states' gradients enter: the one the direction's forward ended on
      const bool last = reverse ? (t == 0) : (t == len - 1);
      Cell::live_row(d, dh, last, len, grow, tnj, nj, N, H, bsum);
    }
    __syncthreads();      // the next pass rewrites `part`
  }
  if (t < 0) return;
  // column sums of this step's gate gradients for the workgroup's units: row groups added in a fixed order, then the running sums
#pragma unroll
  for (int g = 0; g < 4; ++g) red[erow][g][tid & 31] = bsum[g];
  __syncthreads();
  if (tid < 4 * RB_JT) {
    const int g = tid >> 5, jj = tid & 31;
    if (j0 + jj < H) {
      float s = red[0][g][jj];
#pragma unroll
      for (int r = 1; r < RB_ROWG; ++r) s += red[r][g][jj];
      Cell::store_sum(d, g, (size_t)j0 + jj, H, s, first);
    }
  }
}

// The launches of a layer's backward recurrence.  `step` holds the directions' blocks (dir[1] unused with ndir == 1); t and
// dg_prev are set here.  Launch s: direction 0's step max_len - 1 - s beside the reverse direction's step s; launch max_len:
// the d_h0 products (with max_len == 1 it follows the first step directly and still reads row 0).  Steps >= max_len have no
// launch: the entries zero their rows of the gate-gradient planes first, and ask for the launches' error afterwards.
template <class Cell>
static void bwd_steps_launch(RbStep<Cell>& step, int ndir, const int32_t* lens, int max_len, int T, int N, int H, hipStream_t st) {
  const size_t row = (size_t)N * Cell::G * H;
  const dim3 grid((unsigned)cdiv(H, RB_JT), (unsigned)ndir);
  for (int s = 0; s <= max_len; ++s) {
    const bool tail = s == max_len;
    step.dir[0].t = tail ? -1 : max_len - 1 - s;
    step.dir[1].t = tail ? -1 : s;
    step.dir[0].dg_prev = s == 0 ? nullptr : step.dir[0].dgh + (size_t)(max_len - s) * row;
    // (not read by the d_h0 launch: own rows)
    step.dir[1].dg_prev = (s == 0 || ndir == 1) ? nullptr : step.dir[1].dgh + (size_t)(s - 1) * row;
    hipLaunchKernelGGL(rnn_bwd_step_kernel<Cell>, grid, dim3(RB_THREADS), 0, st, step, lens, ndir * H, T, N, H, s == 0 ? 1 : 0);
  }
}

// ms_lstm_backward_steps (ndir == 1, w_hh_rev unused), ms_lstm_backward_steps_bidir and (Cell = HardLstmCell)
// ms_hard_lstm_backward_steps: direction-major arguments.
template <class Cell>
static void lstm_bwd_steps(int ndir, const float* gates, const float* c, const float* c0, const float* w_hh_fwd,
                           const float* w_hh_rev, const float* d_out, const float* d_hn, const float* d_cn, const int32_t* lens,
                           int max_len, float* dG, float* d_h0, float* d_c0, float* d_b, int T, int N, int H, hipStream_t st) {
  const size_t nh = (size_t)N * H;
  const size_t plane = (size_t)T * N * 4 * H;      // one direction of gates / dG; c is plane / 4
  RbStep<Cell> step = {};
  step.dir[0] = LstmCell::Dir{{gates, w_hh_fwd, d_out, d_hn, nullptr, dG, d_h0, 0, 0, 1}, c, c0, d_cn, d_c0, d_b};
  if (ndir == 2) {
    step.dir[1] = LstmCell::Dir{{gates + plane, w_hh_rev, d_out + H, d_hn ? d_hn + nh : nullptr, nullptr, dG + plane, d_h0 + nh, 0, 1, 1},
                                c + plane / 4, c0 ? c0 + nh : nullptr, d_cn ? d_cn + nh : nullptr, d_c0 + nh, d_b + (size_t)4 * H};
  }
  bwd_steps_launch(step, ndir, lens, max_len, T, N, H, st);
}

}  // namespace ms

extern "C" size_t ms_lstm_recompute_workspace_bytes(int T, int N, int H) {
  if (T <= 0 || N <= 0 || H <= 0) return 0;
  return 2 * ms::recompute_plane_bytes(4, T, N, H);
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
  float* p1 = (float*)workspace;
  float* p2 = p1 + ms::recompute_plane_bytes(4, T, N, H) / sizeof(float);
  const int rc = ms::recompute_products(4, x, h, h0, w_ih, w_hh, b_ih, b_hh, T, N, In, H, reverse, p1, p2, st);
  if (rc != MS_OK) return rc;
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
  ms::lstm_bwd_steps<ms::LstmCell>(1, gates, c, c0, w_hh, nullptr, d_out, d_hn, d_cn, lens, max_len, dG, d_h0, d_c0, d_b, T, N, H,
                                   st);
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
  float* dG_rev = dG + (size_t)T * row;
  if (max_len < T) {
    const size_t bytes = (size_t)(T - max_len) * row * sizeof(float);
    MS_HIP(hipMemsetAsync(dG + (size_t)max_len * row, 0, bytes, st));
    MS_HIP(hipMemsetAsync(dG_rev + (size_t)max_len * row, 0, bytes, st));
  }
  ms::lstm_bwd_steps<ms::LstmCell>(2, gates, c, c0, w_hh_fwd, w_hh_rev, d_out, d_hn, d_cn, lens, max_len, dG, d_h0, d_c0, d_b, T, N,
                                   H, st);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_hard_lstm_recompute(const float* x, const float* h, const float* h0, const float* c0, const float* w_ih,
                                      const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* c, int T, int N,
                                      int In, int H, int reverse, void* workspace, size_t workspace_bytes, void* stream_) {
  MS_REQUIRE(x && h && w_ih && w_hh && gates && c, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && In > 0 && H > 0, "bad shape");
  MS_REQUIRE(reverse == 0 || reverse == 1, "reverse must be 0 or 1");
  MS_REQUIRE((size_t)T * N < ((size_t)1 << 31) / 4 / (size_t)H, "T N 4H exceeds the GEMM's int extents");
  MS_REQUIRE(workspace != nullptr, "null workspace");
  if (workspace_bytes < ms_lstm_recompute_workspace_bytes(T, N, H)) {
    ms::set_error("ms_hard_lstm_recompute: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream_;
  float* p1 = (float*)workspace;
  float* p2 = p1 + ms::recompute_plane_bytes(4, T, N, H) / sizeof(float);
  const int rc = ms::recompute_products(4, x, h, h0, w_ih, w_hh, b_ih, b_hh, T, N, In, H, reverse, p1, p2, st);
  if (rc != MS_OK) return rc;
  const size_t cells = (size_t)N * H;
  hipLaunchKernelGGL(ms::hard_lstm_scan_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p1, p2, b_hh, c0, gates, c,
                     T, N, H, h0 != nullptr ? 1 : 0, reverse);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_hard_lstm_backward_steps(const float* gates, const float* c, const float* c0, const float* w_hh_fwd,
                                           const float* w_hh_rev, const float* d_out, const float* d_hn, const float* d_cn, float* dA,
                                           float* d_h0, float* d_c0, float* d_b, int T, int N, int H, int ndir, void* stream_) {
  MS_REQUIRE(ndir == 1 || ndir == 2, "ndir must be 1 or 2");
  MS_REQUIRE(gates && c && w_hh_fwd && d_out && dA && d_h0 && d_c0 && d_b, "null pointer");
  MS_REQUIRE(ndir == 1 || w_hh_rev != nullptr, "null w_hh_rev with ndir == 2");
  MS_REQUIRE(T > 0 && N > 0 && H > 0, "bad shape");
  MS_REQUIRE((size_t)T * N < ((size_t)1 << 31) / 4 / (size_t)H, "T N 4H exceeds the int extents");
  // (both halves of dA are read in 16-byte quads: T N 4H floats apart, so one test covers them)
  MS_REQUIRE(((uintptr_t)dA & 15) == 0, "dA must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  // (no lengths: every sequence has T steps, so no row of dA is left to a memset)
  ms::lstm_bwd_steps<ms::HardLstmCell>(ndir, gates, c, c0, w_hh_fwd, w_hh_rev, d_out, d_hn, d_cn, nullptr, T, dA, d_h0, d_c0, d_b, T, N,
                                       H, st);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" size_t ms_gru_recompute_workspace_bytes(int T, int N, int H) {
  if (T <= 0 || N <= 0 || H <= 0) return 0;
  return 2 * ms::recompute_plane_bytes(3, T, N, H);
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
  float* p1 = (float*)workspace;
  float* p2 = p1 + ms::recompute_plane_bytes(3, T, N, H) / sizeof(float);
  const int rc = ms::recompute_products(3, x, h, h0, w_ih, w_hh, b_ih, b_hh, T, N, In, H, reverse, p1, p2, st);
  if (rc != MS_OK) return rc;
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
  ms::RbStep<ms::GruCell> step = {};
  step.dir[0] = ms::GruCell::Dir{{gates, w_hh_fwd, d_out, d_hn, nullptr, dGh, d_h0, 0, 0, vec}, q, h, h0, dGi, d_b_ih, d_b_hh};
  if (ndir == 2) {
    step.dir[1] = ms::GruCell::Dir{{gates + plane, w_hh_rev, d_out + H, d_hn ? d_hn + nh : nullptr, nullptr, dGh + plane, d_h0 + nh, 0,
                                    1, vec},
                                   q + plane / 3, h + plane / 3, h0 ? h0 + nh : nullptr, dGi + plane, d_b_ih + (size_t)3 * H,
                                   d_b_hh + (size_t)3 * H};
  }
  ms::bwd_steps_launch(step, ndir, lens, max_len, T, N, H, st);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
