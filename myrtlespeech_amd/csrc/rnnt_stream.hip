// RNN-T greedy decode advanced one chunk of encoder rows at a time (oracle/rnnt_oracle.py::greedy_decode, its frame loop cut
// between frames).  OWN specification, like everything under the RNN-T label: the comment on ms_rnnt_greedy_stream_step in
// include/ms_hotpath.h; tests/rnnt_stream_ref.py restates it in numpy.
//
//   ms_rnnt_greedy_stream_state_bytes / _workspace_bytes / _begin / _step
//
// What a stream carries between two pushes lives in `state` on the device:
//   int32 header[16]        [0] sticky overflow word, [1] iterations launched since _begin (a record for tools), rest reserved
//   int32 per_stream[N][4]  {labels so far, frames seen, reserved, reserved}
//   float h[N][L][H], c[N][L][H]   the predictor's LSTM state after the stream's prefix
//   float pred_p[N][J]             w_pred . h_top: the prefix as the joint sees it
// Nothing about a frame is carried: a frame never spans two pushes, so the per-frame label quota starts at zero in every step.
//
// The step is the event-driven loop of the greedy ms_rnnt_decode (rnnt_decode.hip): the prediction only changes after a label,
// so up to 32 pending frames of a stream are scored against its current prediction at once.  One iteration =
//   rnnt_stream_score_scan_kernel   one workgroup per stream: A = tanh(enc_p[frame] + pred_p) of its <= 32 pending frames as
//                                   fp16 hi + lo fragments in LDS, x = A . w_out on MFMA (f16x3, w_out packed in operand order
//                                   once per step by rnnt_score.h's pack kernel), column block by column block with a running
//                                   (max, first index) per frame and lane; then the frames are walked to the first non-blank,
//                                   the label is appended and a predictor step requested.  No log-softmax, no logit buffer.
//   rnnt_stream_pred_layer_kernel   per LSTM layer: the gates of every stream that just emitted, float32 FMA straight from the
//                                   torch-layout weights (4 B per weight and step, read once for all requesting streams; the
//                                   step is a weight pull, not arithmetic), and the cell
//   rnnt_stream_pred_proj_kernel    pred_p = w_pred . h_top of those streams; the new h replaces the old one
// i.e. 2 + L launches per iteration and about (labels of the busiest stream + blocks of 32 blank frames) iterations per push.
// The iteration count depends on the data, so the step BLOCKS the host: it polls a device counter of finished streams through
// a small pinned ring a few iterations behind the queue, and runs at most rows * max_symbols + ceil(rows / 32) + 1 iterations
// whatever the device reports.  No kernel waits on another workgroup: no spin, no status word.
//
// Determinism: a (frame, prefix) pair's logits are formed by the same operations wherever the frame sits in its block of 32
// (MFMA rows are independent; rows that do not exist are zeros) and whichever streams share the launch; a predictor step's sums
// run over k in one fixed order per (stream, unit).  Transcripts and emission frames therefore do not depend on the chunking.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "rnnt_loss.h"
#include "rnnt_score.h"

namespace {

constexpr int GS_HDR_INTS = 16;      // 64 bytes: overflow word, iteration record, room to grow
constexpr int GS_STREAM_INTS = 4;    // per stream: label count, frames seen, two reserved
constexpr int GS_FRAMES = 32;        // pending frames scored per stream and iteration: the M of one 32x32 MFMA tile
constexpr int GS_SLAB_KS = 64;       // K steps of 16 held in LDS at once: 64 x 2 planes x 64 lanes x 16 B = 128 KiB (J <= 1024)
constexpr int GS_SB = 8;             // streams whose sums one wave of the predictor kernels carries at once
constexpr int GS_LIST = 1024;        // requesting streams listed in LDS at once

struct GsState {
  size_t ints, h, c, pp, total;
};
GsState gs_state(int N, int H, int L, int J) {
  GsState s{};
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += ms::align_up(bytes, 256); return at; };
  s.ints = take(((size_t)GS_HDR_INTS + (size_t)N * GS_STREAM_INTS) * 4);
  s.h = take((size_t)N * L * H * 4);
  s.c = take((size_t)N * L * H * 4);
  s.pp = take((size_t)N * J * 4);
  s.total = o;
  return s;
}

struct GsWork {
  size_t packed, rows, pos, nsym, req, base, done, hn, total;
};
GsWork gs_work(int N, int V1, int H, int L, int J) {
  GsWork w{};
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += ms::align_up(bytes, 256); return at; };
  w.packed = take(ms::rs_packed_bytes(J, V1));
  w.rows = take((size_t)N * 4);     // rows of this push that exist for the stream
  w.pos = take((size_t)N * 4);      // the stream's current row of the push
  w.nsym = take((size_t)N * 4);     // labels emitted on that row so far
  w.req = take((size_t)N * 4);      // predictor request: the label just emitted, or -1
  w.base = take((size_t)N * 4);     // frames seen before this push
  w.done = take(4);                 // streams that have used up their rows
  w.hn = take((size_t)N * L * H * 4);   // the step's new h of every layer (the old one is still being read)
  w.total = o;
  return w;
}

__device__ __forceinline__ float gs_wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void rnnt_stream_begin_kernel(int32_t* __restrict__ ints, float* __restrict__ h,
                                                                float* __restrict__ c, int32_t* __restrict__ req, int N,
                                                                size_t lh, int blank) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)GS_HDR_INTS + (size_t)N * GS_STREAM_INTS) ints[i] = 0;
  if (i < (size_t)N) req[i] = i == 0 ? blank : -1;          // the start step is taken once, by stream 0
  if (i < lh) {                                             // stream 0's zero state; the others get its result
    h[i] = 0.f;
    c[i] = 0.f;
  }
}

// stream 0's state after the start symbol -> every other stream
__global__ __launch_bounds__(256) void rnnt_stream_broadcast_kernel(float* __restrict__ h, float* __restrict__ c,
                                                                    float* __restrict__ pp, int N, size_t lh, int J) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int i = blockIdx.y + 1; i < N; i += gridDim.y) {
    if (e < lh) {
      h[(size_t)i * lh + e] = h[e];
      c[(size_t)i * lh + e] = c[e];
    }
    if (e < (size_t)J) pp[(size_t)i * J + e] = pp[e];
  }
}

// One block.  The rows of this push that exist per stream, the walk's starting point, "nothing new" in the news table.
__global__ __launch_bounds__(256) void rnnt_stream_step_init_kernel(int32_t* __restrict__ ints, const int32_t* __restrict__ total_lens,
                                                                    const int32_t* __restrict__ chunk_lens,
                                                                    int32_t* __restrict__ rows_i, int32_t* __restrict__ pos,
                                                                    int32_t* __restrict__ nsym, int32_t* __restrict__ req,
                                                                    int32_t* __restrict__ base, int32_t* __restrict__ done,
                                                                    int32_t* __restrict__ fresh, int fresh_stride, int rows,
                                                                    int n, int N) {
  __shared__ int idle;
  if (threadIdx.x == 0) idle = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += 256) {
    if (fresh) fresh[(size_t)i * fresh_stride] = 0;
    req[i] = -1;
    if (i >= n) continue;
    int32_t* s = ints + GS_HDR_INTS + (size_t)i * GS_STREAM_INTS;
    const int seen = s[1];
    const int avail = chunk_lens ? min(max(chunk_lens[i], 0), rows) : min(max(total_lens[i] - seen, 0), rows);
    rows_i[i] = avail;
    pos[i] = 0;
    nsym[i] = 0;
    base[i] = seen;
    s[1] = seen + avail;
    if (avail == 0) atomicAdd(&idle, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) *done = idle;
}

// The streams i < n with a request, in LDS (wave 0 of the caller; `list` holds up to GS_LIST of streams first .. first + GS_LIST - 1).
__device__ __forceinline__ int gs_list_requests(const int32_t* __restrict__ req, int first, int n, int* list, int lane) {
  int cnt = 0;
  const int end = min(n, first + GS_LIST);
  for (int s0 = first; s0 < end; s0 += 64) {
    const int s = s0 + lane;
    const bool a = s < end && req[s] >= 0;
    const unsigned long long mask = __ballot(a);
    if (a) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = s;
    cnt += __popcll(mask);
  }
  return cnt;
}

// One LSTM layer of the predictor step of every requesting stream.  A wave owns ONE hidden unit (its four gate rows) and
// carries the sums of GS_SB streams at a time: lane k-strided float32 FMAs in one fixed order per (stream, unit), a butterfly,
// then lane j applies the cell for the chunk's stream j.  x = embedding[label] (layer 0) or the layer below's new h; the
// recurrent input is the stream's old h, which stays in place until the projection kernel has run; c is the unit's own word.
__global__ __launch_bounds__(256) void rnnt_stream_pred_layer_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                                     const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                                     const float* __restrict__ embedding,
                                                                     const int32_t* __restrict__ req, const float* __restrict__ h,
                                                                     float* __restrict__ c, float* __restrict__ hn, int n, int D,
                                                                     int H, int L, int l, int V1) {
  __shared__ int list[GS_LIST];
  __shared__ int n_list;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * 4 + wave;
  const int In = l == 0 ? D : H;
  const bool vec = ((In | H) & 3) == 0;                       // a property of the model: one summation order per network
  for (int first = 0; first < n; first += GS_LIST) {
    __syncthreads();
    if (wave == 0) {
      const int cnt = gs_list_requests(req, first, n, list, lane);
      if (lane == 0) n_list = cnt;
    }
    __syncthreads();
    const int na = n_list;
    if (u >= H) continue;
    for (int a0 = 0; a0 < na; a0 += GS_SB) {
      const float* xin[GS_SB];
      const float* hrec[GS_SB];
#pragma unroll
      for (int j = 0; j < GS_SB; ++j) {
        const int s = list[min(a0 + j, na - 1)];            // (past the list: a copy of its last stream, never stored)
        if (l == 0) xin[j] = embedding + (size_t)min(max(req[s], 0), V1 - 1) * D;
        else xin[j] = hn + ((size_t)s * L + (l - 1)) * H;
        hrec[j] = h + ((size_t)s * L + l) * H;
      }
      float acc[4][GS_SB];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < GS_SB; ++j) acc[g][j] = 0.f;
      // one segment of the gate rows' dot products: K weights per row against K inputs per stream (VEC: 16-byte loads)
      auto segment = [&](const float* __restrict__ wm, int K, const float* const* xs) {
        if (vec) {
          for (int k = 4 * lane; k < K; k += 256) {
            f32x4 w[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const f32x4*>(wm + ((size_t)g * H + u) * K + k);
#pragma unroll
            for (int j = 0; j < GS_SB; ++j) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(xs[j] + k);
#pragma unroll
              for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[g][j] = fmaf(w[g][e], x[e], acc[g][j]);
            }
          }
        } else {
          for (int k = lane; k < K; k += 64) {
            float w[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = wm[((size_t)g * H + u) * K + k];
#pragma unroll
            for (int j = 0; j < GS_SB; ++j) {
              const float x = xs[j][k];
#pragma unroll
              for (int g = 0; g < 4; ++g) acc[g][j] = fmaf(w[g], x, acc[g][j]);
            }
          }
        }
      };
      segment(w_ih, In, xin);
      segment(w_hh, H, hrec);
      float pre[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < GS_SB; ++j) {
          const float t = gs_wsum(acc[g][j]);
          if (lane == j) pre[g] = t;
        }
      if (lane < GS_SB && a0 + lane < na) {
        const int s = list[a0 + lane];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] += (b_ih ? b_ih[g * H + u] : 0.f) + (b_hh ? b_hh[g * H + u] : 0.f);
        const size_t at = ((size_t)s * L + l) * H + u;
        const float gi = 1.f / (1.f + expf(-pre[0])), gf = 1.f / (1.f + expf(-pre[1]));
        const float gg = tanhf(pre[2]), go = 1.f / (1.f + expf(-pre[3]));
        const float c_new = gf * c[at] + gi * gg;
        c[at] = c_new;
        hn[at] = go * tanhf(c_new);
      }
    }
  }
}

// pred_p = w_pred . h_top of every requesting stream (a wave per joint unit, as above), and the step's new h of every layer
// into the state: no layer kernel of this step reads h any more.
__global__ __launch_bounds__(256) void rnnt_stream_pred_proj_kernel(const float* __restrict__ w_pred, const int32_t* __restrict__ req,
                                                                    const float* __restrict__ hn, float* __restrict__ h,
                                                                    float* __restrict__ pp, int n, int H, int L, int J) {
  __shared__ int list[GS_LIST];
  __shared__ int n_list;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ju = blockIdx.x * 4 + wave;
  const size_t lh = (size_t)L * H;
  for (int first = 0; first < n; first += GS_LIST) {
    __syncthreads();
    if (wave == 0) {
      const int cnt = gs_list_requests(req, first, n, list, lane);
      if (lane == 0) n_list = cnt;
    }
    __syncthreads();
    const int na = n_list;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)na * lh; e += (size_t)gridDim.x * 256) {
      const size_t at = (size_t)list[e / lh] * lh + e % lh;
      h[at] = hn[at];
    }
    if (ju >= J) continue;
    for (int a0 = 0; a0 < na; a0 += GS_SB) {
      const float* x[GS_SB];
#pragma unroll
      for (int j = 0; j < GS_SB; ++j) x[j] = hn + ((size_t)list[min(a0 + j, na - 1)] * L + (L - 1)) * H;
      float acc[GS_SB];
#pragma unroll
      for (int j = 0; j < GS_SB; ++j) acc[j] = 0.f;
      if ((H & 3) == 0) {
        for (int k = 4 * lane; k < H; k += 256) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(w_pred + (size_t)ju * H + k);
#pragma unroll
          for (int j = 0; j < GS_SB; ++j) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x[j] + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = fmaf(w[e], v[e], acc[j]);
          }
        }
      } else {
        for (int k = lane; k < H; k += 64) {
          const float w = w_pred[(size_t)ju * H + k];
#pragma unroll
          for (int j = 0; j < GS_SB; ++j) acc[j] = fmaf(w, x[j][k], acc[j]);
        }
      }
      float mine = 0.f;
#pragma unroll
      for (int j = 0; j < GS_SB; ++j) {
        const float t = gs_wsum(acc[j]);
        if (lane == j) mine = t;
      }
      if (lane < GS_SB && a0 + lane < na) pp[(size_t)list[a0 + lane] * J + ju] = mine;
    }
  }
}

// One iteration of one stream (one workgroup of four waves): see the head of the file.  A_lds holds the fragments of
// A = tanh(enc_p + pred_p) for slab_ks K steps: [K step][hi, lo][lane] x 16 bytes, lane (r, half) = the 8 consecutive k of row
// r that mfma_f32_32x32x16_f16 wants from it, so a wave's operand read is 1 KB contiguous.  J above 16 slab_ks takes several
// slabs and forms them again for every group of four column blocks (as rnnt_score_cells_kernel recomputes its rows).
__global__ __launch_bounds__(256) void rnnt_stream_score_scan_kernel(
    const float* __restrict__ enc_p, const float* __restrict__ pp, const u32x4_* __restrict__ packed,
    const float* __restrict__ b_out, int32_t* __restrict__ ints, const int32_t* __restrict__ rows_i, int32_t* __restrict__ pos,
    int32_t* __restrict__ nsym, int32_t* __restrict__ req, const int32_t* __restrict__ base, int32_t* __restrict__ done,
    int32_t* __restrict__ labels, int32_t* __restrict__ label_frames, int cap, int32_t* __restrict__ fresh, int fresh_stride,
    int n, int J, int V1, int max_symbols, int k_steps, int slab_ks) {
  extern __shared__ __attribute__((aligned(16))) u32x4_ A_lds[];
  __shared__ float bv_s[4][GS_FRAMES];
  __shared__ int bi_s[4][GS_FRAMES];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int avail = rows_i[i], p0 = pos[i], ns0 = nsym[i];
  if (tid == 0) {
    req[i] = -1;
    if (i == 0) ints[1] += 1;
  }
  if (p0 >= avail) return;                                     // (uniform) the stream has used up its rows
  const int m = min(GS_FRAMES, avail - p0);
  const int blank = V1 - 1;
  const int n_slabs = (k_steps + slab_ks - 1) / slab_ks;
  const int n_cb = (V1 + 31) / 32;
  const float* prow = pp + (size_t)i * J;
  const bool vec = (J & 3) == 0;

  auto form = [&](int slab) {
    const int ks0 = slab * slab_ks, nks = min(slab_ks, k_steps - ks0);
    for (int it = tid; it < nks * 64; it += 256) {
      const int ks = it >> 6, ln = it & 63, r = ln & 31, hh = ln >> 5;
      const int k0 = (ks0 + ks) * 16 + 8 * hh;
      float z[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = 0.f;                  // rows that do not exist, k past J: zeros against any weight
      if (r < m) {
        const float* erow = enc_p + ((size_t)(p0 + r) * n + i) * J;
        if (vec && k0 + 8 <= J) {
          const f32x4 e0 = *reinterpret_cast<const f32x4*>(erow + k0), e1 = *reinterpret_cast<const f32x4*>(erow + k0 + 4);
          const f32x4 q0 = *reinterpret_cast<const f32x4*>(prow + k0), q1 = *reinterpret_cast<const f32x4*>(prow + k0 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            z[j] = rs_tanh(e0[j] + q0[j]);
            z[4 + j] = rs_tanh(e1[j] + q1[j]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k0 + j < J) z[j] = rs_tanh(erow[k0 + j] + prow[k0 + j]);
        }
      }
      unsigned hi[8], lo[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (z[j] != z[j]) { hi[j] = 0x7e00u; lo[j] = 0u; }     // a NaN stays one, in this row only
        else ms::plane_split_bounded<true>(z[j], hi[j], lo[j]);
      }
      A_lds[(size_t)(ks * 2) * 64 + ln] = u32x4_{hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
      A_lds[(size_t)(ks * 2 + 1) * 64 + ln] = u32x4_{lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
    }
  };

  // running (max, first index) of this lane's 16 rows over the columns it has seen: column blocks come in ascending order,
  // so a later column replaces the best only if it is greater
  float bv[16];
  int bi[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bv[r] = -INFINITY;
    bi[r] = 0x7fffffff;
  }
  for (int cb0 = 0; cb0 < n_cb; cb0 += 4) {
    const int cb = cb0 + wave;
    const bool active = cb < n_cb;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int slab = 0; slab < n_slabs; ++slab) {
      if (n_slabs > 1 || cb0 == 0) {                           // (uniform)
        __syncthreads();
        form(slab);
        __syncthreads();
      }
      if (!active) continue;
      const int ks0 = slab * slab_ks, nks = min(slab_ks, k_steps - ks0);
      const u32x4_* bp = packed + ((size_t)cb * k_steps + ks0) * 128 + lane;
      for (int ks = 0; ks < nks; ++ks) {
        const u32x4_ ah = A_lds[(size_t)(ks * 2) * 64 + lane], al = A_lds[(size_t)(ks * 2 + 1) * 64 + lane];
        const u32x4_ bh = bp[(size_t)ks * 128], bl = bp[(size_t)ks * 128 + 64];
        acc = ms::mfma_32x32x16<true>(al, bh, acc);
        acc = ms::mfma_32x32x16<true>(ah, bl, acc);
        acc = ms::mfma_32x32x16<true>(ah, bh, acc);
      }
    }
    if (!active) continue;
    const int v = cb * 32 + (lane & 31);
    const bool in = v < V1;
    const float bias = (in && b_out) ? b_out[v] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x = acc[r] + bias;
      if (in && x > bv[r]) { bv[r] = x; bi[r] = v; }
    }
  }
  // the 32 lanes of a row (fixed order; equal values -> the lower index), then the four waves
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv[r], o, 64);
      const int oi = __shfl_xor(bi[r], o, 64);
      if (ov > bv[r] || (ov == bv[r] && oi < bi[r])) { bv[r] = ov; bi[r] = oi; }
    }
    if ((lane & 31) == 0) {
      const int row = ms::mfma32_row(r, lane);
      bv_s[wave][row] = bv[r];
      bi_s[wave][row] = bi[r];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  // ---- the walk: lane c holds frame p0 + c's symbol; blanks advance the frame, the FIRST label is emitted
  int sym = blank;
  if (lane < m) {
    float best = bv_s[0][lane];
    int at = bi_s[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ov = bv_s[w][lane];
      const int oi = bi_s[w][lane];
      if (ov > best || (ov == best && oi < at)) { best = ov; at = oi; }
    }
    sym = at < blank ? at : blank;                             // a row without any number (NaN, all -inf): blank, in bounds
  }
  const unsigned long long labelled = __ballot(lane < m && sym != blank);
  if (labelled == 0ull) {
    if (lane == 0) {
      pos[i] = p0 + m;
      nsym[i] = 0;
      if (p0 + m >= avail) atomicAdd(done, 1);
    }
    return;
  }
  const int c = __ffsll((long long)labelled) - 1;
  const int emitted = __shfl(sym, c, 64);
  if (lane != 0) return;
  int t = p0 + c, ns = (c == 0 ? ns0 : 0) + 1;
  const int frame = base[i] + t;
  if (ns >= max_symbols) {                                     // the frame's quota is used up
    ++t;
    ns = 0;
  }
  int32_t* s = ints + GS_HDR_INTS + (size_t)i * GS_STREAM_INTS;
  const int count = s[0];
  if (count < cap) {
    labels[(size_t)i * cap + count] = emitted;
    if (label_frames) label_frames[(size_t)i * cap + count] = frame;
    if (fresh) {
      int32_t* news = fresh + (size_t)i * fresh_stride;
      const int k = news[0];
      if (1 + k < fresh_stride) news[1 + k] = emitted;
      news[0] = k + 1;
    }
  } else {
    ints[0] = 1;                                               // sticky; every stream that sets it stores the same word
  }
  s[0] = count + 1;
  req[i] = emitted;                                            // the predictor steps even past `cap`: later labels stay right
  pos[i] = t;
  nsym[i] = ns;
  if (t >= avail) atomicAdd(done, 1);
}

// The step polls a device counter through a small pinned ring; allocating pinned memory or freeing it synchronises the whole
// device, so ring and events are made once per (host thread, device) and kept (as rnnt_decode.hip's GreedyPoll).
struct StreamPoll {
  static constexpr int RING = 4;
  int32_t* host = nullptr;
  hipEvent_t ev[RING] = {nullptr, nullptr, nullptr, nullptr};
};
StreamPoll* stream_poll() {
  static thread_local StreamPoll polls[64];
  static thread_local unsigned char made[64];        // 0 = not made, 1 = ready, 2 = failed
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  dev &= 63;
  if (made[dev] == 0) {
    StreamPoll& g = polls[dev];
    bool ok = hipHostMalloc((void**)&g.host, StreamPoll::RING * sizeof(int32_t), hipHostMallocDefault) == hipSuccess;
    for (int k = 0; ok && k < StreamPoll::RING; ++k) ok = hipEventCreateWithFlags(&g.ev[k], hipEventDisableTiming) == hipSuccess;
    made[dev] = ok ? 1 : 2;
  }
  return made[dev] == 1 ? &polls[dev] : nullptr;
}

struct GsNet {
  const float* embedding;
  const float* const* w_ih;
  const float* const* w_hh;
  const float* const* b_ih;
  const float* const* b_hh;
  const float* w_pred;
  int V, D, H, L, J;
};

// the predictor step of the streams i < n with a request (req[i] >= 0): L + 1 launches
int gs_predictor_step(const GsNet& net, const GsState& S, const GsWork& W, char* st, char* ws, int n, hipStream_t s) {
  const int32_t* req = (const int32_t*)(ws + W.req);
  float* h = (float*)(st + S.h);
  float* c = (float*)(st + S.c);
  float* hn = (float*)(ws + W.hn);
  for (int l = 0; l < net.L; ++l) {
    hipLaunchKernelGGL(rnnt_stream_pred_layer_kernel, dim3(ms::cdiv(net.H, 4)), dim3(256), 0, s, net.w_ih[l], net.w_hh[l],
                       net.b_ih[l], net.b_hh[l], net.embedding, req, h, c, hn, n, net.D, net.H, net.L, l, net.V + 1);
    MS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rnnt_stream_pred_proj_kernel, dim3(ms::cdiv(net.J, 4)), dim3(256), 0, s, net.w_pred, req, hn, h,
                     (float*)(st + S.pp), n, net.H, net.L, net.J);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

// MS_OK, or the reason the shape is not served (nothing has been launched)
int gs_check_shape(const char* who, int N, int V, int D, int H, int L, int J) {
  if (L > 8) {
    ms::set_error(std::string(who) + ": at most 8 predictor layers");
    return MS_ERR_UNSUPPORTED;
  }
  const long pack_threads = (long)(ms::rs_col_blocks(V + 1) * ms::rs_k_steps(J) * 64);
  if ((pack_threads + 255) / 256 > 0x7fffffffL) {
    ms::set_error(std::string(who) + ": J x (V + 1) exceeds a launch grid");
    return MS_ERR_UNSUPPORTED;
  }
  (void)N;
  (void)D;
  (void)H;
  return MS_OK;
}

}  // namespace

extern "C" size_t ms_rnnt_greedy_stream_state_bytes(int N, int H, int L, int J) {
  if (N <= 0 || H <= 0 || L <= 0 || J <= 0) return 0;
  return gs_state(N, H, L, J).total;
}

extern "C" size_t ms_rnnt_greedy_stream_workspace_bytes(int N, int V, int D, int H, int L, int J) {
  if (N <= 0 || V <= 0 || D <= 0 || H <= 0 || L <= 0 || J <= 0) return 0;
  return gs_work(N, V + 1, H, L, J).total;
}

extern "C" int ms_rnnt_greedy_stream_begin(void* state, int N, const float* embedding, const float* const* w_ih,
                                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                                           const float* w_pred, const float* w_out, const float* b_out, int V, int D, int H,
                                           int L, int J, void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(state && embedding && w_ih && w_hh && b_ih && b_hh && w_pred && w_out && workspace, "null pointer");
  MS_REQUIRE(N > 0 && V > 0 && D > 0 && H > 0 && L > 0 && J > 0, "bad shape");
  (void)b_out;
  int rc = gs_check_shape(__func__, N, V, D, H, L, J);
  if (rc != MS_OK) return rc;
  for (int l = 0; l < L; ++l) MS_REQUIRE(w_ih[l] && w_hh[l], "null layer weights");
  MS_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "state and workspace must be 16-byte aligned");
  const GsState S = gs_state(N, H, L, J);
  const GsWork W = gs_work(N, V + 1, H, L, J);
  if (workspace_bytes < W.total) {
    ms::set_error("ms_rnnt_greedy_stream_begin: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char *st = (char*)state, *ws = (char*)workspace;
  const size_t lh = (size_t)L * H;
  const size_t words = std::max(std::max(lh, (size_t)J), (size_t)GS_HDR_INTS + (size_t)N * GS_STREAM_INTS);
  hipLaunchKernelGGL(rnnt_stream_begin_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, (int32_t*)(st + S.ints),
                     (float*)(st + S.h), (float*)(st + S.c), (int32_t*)(ws + W.req), N, lh, V);
  MS_LAUNCH_CHECK();
  const GsNet net{embedding, w_ih, w_hh, b_ih, b_hh, w_pred, V, D, H, L, J};
  rc = gs_predictor_step(net, S, W, st, ws, 1, s);              // the start symbol, once: the same for every stream
  if (rc != MS_OK) return rc;
  if (N > 1) {
    hipLaunchKernelGGL(rnnt_stream_broadcast_kernel, dim3((unsigned)((std::max(lh, (size_t)J) + 255) / 256), std::min(N - 1, 1024)),
                       dim3(256), 0, s, (float*)(st + S.h), (float*)(st + S.c), (float*)(st + S.pp), N, lh, J);
    MS_LAUNCH_CHECK();
  }
  return MS_OK;
}

extern "C" int ms_rnnt_greedy_stream_step(const float* enc_p, int rows, int n, const int32_t* total_lens,
                                          const int32_t* chunk_lens, const float* embedding, const float* const* w_ih,
                                          const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                                          const float* w_pred, const float* w_out, const float* b_out, int32_t* labels,
                                          int32_t* label_frames, int cap, int32_t* fresh, void* state, int N, int V, int D,
                                          int H, int L, int J, int max_symbols, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  MS_REQUIRE(enc_p && embedding && w_ih && w_hh && b_ih && b_hh && w_pred && w_out && labels && state && workspace, "null pointer");
  MS_REQUIRE(rows > 0 && N > 0 && n > 0 && n <= N && V > 0 && D > 0 && H > 0 && L > 0 && J > 0 && max_symbols > 0, "bad shape");
  MS_REQUIRE(cap > 0, "label capacity must be positive");
  MS_REQUIRE((total_lens == nullptr) != (chunk_lens == nullptr), "exactly one of total_lens / chunk_lens");
  int rc = gs_check_shape(__func__, N, V, D, H, L, J);
  if (rc != MS_OK) return rc;
  if ((long)rows * max_symbols + 1 > 0x7fffffffL) {
    ms::set_error("ms_rnnt_greedy_stream_step: rows * max_symbols exceeds 31 bits");
    return MS_ERR_UNSUPPORTED;
  }
  for (int l = 0; l < L; ++l) MS_REQUIRE(w_ih[l] && w_hh[l], "null layer weights");
  MS_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)enc_p & 15) == 0,
             "enc_p, state and workspace must be 16-byte aligned");
  const int V1 = V + 1;
  const GsState S = gs_state(N, H, L, J);
  const GsWork W = gs_work(N, V1, H, L, J);
  if (workspace_bytes < W.total) {
    ms::set_error("ms_rnnt_greedy_stream_step: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  StreamPoll* poll = stream_poll();
  if (poll == nullptr) {
    ms::set_error("ms_rnnt_greedy_stream_step: pinned counter ring / events for the end-of-work poll could not be created");
    return MS_ERR_HIP;
  }
  const int k_steps = (int)ms::rs_k_steps(J);
  const int slab_ks = std::min(k_steps, GS_SLAB_KS);
  const size_t lds = (size_t)slab_ks * 2 * 64 * sizeof(u32x4_);
  static ms::DeviceOnce attr_once;
  if (attr_once.need()) {
    MS_HIP(hipFuncSetAttribute((const void*)rnnt_stream_score_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               GS_SLAB_KS * 2 * 64 * (int)sizeof(u32x4_)));
    attr_once.done();
  }
  hipStream_t s = (hipStream_t)stream;
  char *st = (char*)state, *ws = (char*)workspace;
  int32_t* ints = (int32_t*)(st + S.ints);
  int32_t* rows_i = (int32_t*)(ws + W.rows);
  int32_t* pos = (int32_t*)(ws + W.pos);
  int32_t* nsym = (int32_t*)(ws + W.nsym);
  int32_t* req = (int32_t*)(ws + W.req);
  int32_t* base = (int32_t*)(ws + W.base);
  int32_t* done = (int32_t*)(ws + W.done);
  u32x4_* packed = (u32x4_*)(ws + W.packed);
  const int fresh_stride = 1 + rows * max_symbols;
  hipLaunchKernelGGL(rnnt_stream_step_init_kernel, dim3(1), dim3(256), 0, s, ints, total_lens, chunk_lens, rows_i, pos, nsym,
                     req, base, done, fresh, fresh_stride, rows, n, N);
  MS_LAUNCH_CHECK();
  const long pack_threads = (long)(ms::rs_col_blocks(V1) * ms::rs_k_steps(J) * 64);
  hipLaunchKernelGGL(rnnt_score_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, s, w_out, packed, J, V1,
                     k_steps, pack_threads, (long)J, 1L);
  MS_LAUNCH_CHECK();
  const GsNet net{embedding, w_ih, w_hh, b_ih, b_hh, w_pred, V, D, H, L, J};

  // every iteration advances every unfinished stream by one label or by a whole block of blanks, so this bound is never
  // reached unless the device counter cannot be read
  const long max_iters = (long)rows * max_symbols + ms::cdiv(rows, GS_FRAMES) + 1;
  int32_t* host_done = poll->host;
  hipEvent_t* ev = poll->ev;
  constexpr int RING = StreamPoll::RING;
  for (int k = 0; k < RING; ++k) host_done[k] = 0;      // no copy of an earlier call is in flight: every call ends on its last event
  int last_slot = -1;
  long checks = 0;
  rc = MS_OK;
  for (long it = 0; it < max_iters && rc == MS_OK; ++it) {
    hipLaunchKernelGGL(rnnt_stream_score_scan_kernel, dim3(n), dim3(256), lds, s, enc_p, (const float*)(st + S.pp), packed, b_out,
                       ints, rows_i, pos, nsym, req, base, done, labels, label_frames, cap, fresh, fresh_stride, n, J, V1,
                       max_symbols, k_steps, slab_ks);
    if (hipGetLastError() != hipSuccess) { ms::set_error("ms_rnnt_greedy_stream_step: launch failed"); rc = MS_ERR_HIP; break; }
    rc = gs_predictor_step(net, S, W, st, ws, n, s);
    if (rc != MS_OK) break;
    // fetch the counter behind this iteration; look at the one fetched two iterations ago (already complete, or nearly): the
    // queue stays two iterations deep and at most three run past the end, each of them an early exit in every kernel
    const int slot = (int)(checks % RING);
    if (hipMemcpyAsync(&host_done[slot], done, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipEventRecord(ev[slot], s) != hipSuccess) { ms::set_error("ms_rnnt_greedy_stream_step: counter read-back failed"); rc = MS_ERR_HIP; break; }
    last_slot = slot;
    ++checks;
    if (checks > 2) {
      const int old = (int)((checks - 3) % RING);
      if (hipEventSynchronize(ev[old]) == hipSuccess && host_done[old] >= n) break;
    }
  }
  // the pinned words are targets of copies in flight: wait for the last one; ring and events stay with the thread
  if (last_slot >= 0) (void)hipEventSynchronize(ev[last_slot]);
  return rc;
}
