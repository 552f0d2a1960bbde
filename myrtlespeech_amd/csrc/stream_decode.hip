// CTC greedy decode advanced one chunk of logit rows at a time (post_process/ctc_greedy_decoder.py:74-92, whose loop
// this cuts between frames).  NOT reference-derived beyond the rule itself: the reference decodes a whole [T, N, V]
// tensor; a streaming caller gets a few rows per push (16 for a 320 ms chunk behind a stride-2 convolution) and wants
// the labels they add, with the run-length rule applied ACROSS the cut.
//
//   ms_ctc_greedy_stream_state_bytes / _begin / _step   (include/ms_hotpath.h has the contract)
//
// Everything a stream carries between two steps lives in `state` on the device:
//   int32 header[16]        [0] sticky overflow word (a stream had more labels than `cap`), the rest reserved
//   int32 per_stream[N][4]  {arg max of the stream's last existing row (-1: none yet), labels so far, rows seen, reserved}
// and every step reads its running counts from there and writes them back, so the host neither reads a counter nor
// synchronises, and a sequence of steps with a fixed row count is a valid HIP-graph capture.
//
// One wave per stream, one stream per workgroup.  This is latency work (tens of streams x tens of rows): a lane takes a
// row, so a pass of 64 rows needs ONE ballot for the keep mask, one popcount prefix for the labels' places and one
// shuffle for the predecessor -- no LDS, no barrier, no cross-wave scan as ctc_greedy_kernel needs for its 256 frames.
// Alphabets beyond 64 symbols: the wave strides one row at a time (coalesced) with ctc_argmax_wave_kernel's butterfly and
// the row's lane keeps the result; the rest is the same.
#include <algorithm>

#include "common.h"

namespace {

constexpr int STREAM_HDR_INTS = 16;   // 64 bytes: the overflow word and room to grow
constexpr int STREAM_INTS = 4;        // per stream: previous symbol, label count, rows seen, reserved

__global__ __launch_bounds__(64) void ctc_greedy_stream_begin_kernel(int32_t* __restrict__ state, int N) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < STREAM_HDR_INTS) state[i] = 0;
  if (i < N) {
    int32_t* s = state + STREAM_HDR_INTS + (size_t)i * STREAM_INTS;
    s[0] = -1; s[1] = 0; s[2] = 0; s[3] = 0;
  }
}

// arg max of one row by the whole wave, ctc_argmax_wave_kernel's order: NaN before numbers, then the larger value, then
// the lower index (= the first maximum, the first NaN: torch.argmax).  Every lane returns the row's symbol.
__device__ __forceinline__ int wave_row_argmax(const float* __restrict__ row, int V, int lane) {
  float best = 0.f;
  int sym = 0x7fffffff;                                          // a lane without a column never wins
  for (int v = lane; v < V; v += 64) {
    const float c = row[v];
    if (sym == 0x7fffffff || c > best || (c != c && best == best)) { best = c; sym = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int os = __shfl_xor(sym, o, 64);
    const bool mine_nan = best != best, other_nan = ob != ob;
    bool take;
    if (os == 0x7fffffff) take = false;
    else if (sym == 0x7fffffff) take = true;
    else if (mine_nan || other_nan) take = other_nan && (!mine_nan || os < sym);
    else take = ob > best || (ob == best && os < sym);
    if (take) { best = ob; sym = os; }
  }
  return sym;
}

// WIDE: alphabets beyond 64 symbols (see the head of the file).  Grid: N workgroups of one wave; streams [n, N) are not
// part of this step and only report "nothing new".
template <bool WIDE>
__global__ __launch_bounds__(64) void ctc_greedy_stream_kernel(const float* __restrict__ x, int rows, int n, int V, int blank,
                                                               const int32_t* __restrict__ total_lens,
                                                               const int32_t* __restrict__ chunk_lens,
                                                               int32_t* __restrict__ labels, int32_t* __restrict__ label_frames,
                                                               int cap, int32_t* __restrict__ fresh, int32_t* __restrict__ state) {
  const int i = blockIdx.x, lane = threadIdx.x;
  int32_t* news = fresh ? fresh + (size_t)i * (1 + rows) : nullptr;
  if (i >= n) {
    if (news && lane == 0) news[0] = 0;
    return;
  }
  int32_t* s = state + STREAM_HDR_INTS + (size_t)i * STREAM_INTS;
  int carried = s[0];
  const int count0 = s[1], seen = s[2];
  int count = count0;
  const int avail = chunk_lens ? min(max(chunk_lens[i], 0), rows) : min(max(total_lens[i] - seen, 0), rows);
  for (int r0 = 0; r0 < avail; r0 += 64) {
    const int in_pass = min(64, avail - r0);
    const int r = r0 + lane;
    const bool valid = lane < in_pass;
    int sym = -1;
    if (WIDE) {
      for (int k = 0; k < in_pass; ++k) {
        const int a = wave_row_argmax(x + ((size_t)(r0 + k) * n + i) * V, V, lane);
        if (lane == k) sym = a;
      }
    } else if (valid) {
      const float* row = x + ((size_t)r * n + i) * V;
      float best = row[0];
      sym = 0;
      for (int v = 1; v < V; ++v) {
        const float c = row[v];
        if (c > best || (c != c && best == best)) { best = c; sym = v; }
      }
    }
    int prev = __shfl_up(sym, 1, 64);
    if (lane == 0) prev = carried;             // the row before this pass: the previous pass's, or the previous step's
    const bool keep = valid && sym != blank && sym != prev;
    const unsigned long long mask = __ballot(keep);
    const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && at < cap) {
      labels[(size_t)i * cap + at] = sym;
      if (label_frames) label_frames[(size_t)i * cap + at] = seen + r;
      if (news) news[1 + at - count0] = sym;   // at - count0 < rows seen by this step <= rows
    }
    count += __popcll(mask);
    carried = __shfl(sym, in_pass - 1, 64);
  }
  if (lane == 0) {
    s[0] = carried; s[1] = count; s[2] = seen + avail;
    if (count > cap) state[0] = 1;             // sticky; every wave that sets it stores the same word
    if (news) news[0] = min(count, cap) - min(count0, cap);
  }
}

}  // namespace

extern "C" size_t ms_ctc_greedy_stream_state_bytes(int N) {
  if (N <= 0) return 0;
  return ((size_t)STREAM_HDR_INTS + (size_t)N * STREAM_INTS) * sizeof(int32_t);
}

extern "C" int ms_ctc_greedy_stream_begin(void* state, int N, void* stream) {
  MS_REQUIRE(state, "null pointer");
  MS_REQUIRE(N > 0, "bad shape");
  hipLaunchKernelGGL(ctc_greedy_stream_begin_kernel, dim3(ms::cdiv(std::max(N, STREAM_HDR_INTS), 64)), dim3(64), 0,
                     (hipStream_t)stream, (int32_t*)state, N);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

extern "C" int ms_ctc_greedy_stream_step(const float* x, int rows, int n, int V, int blank, const int32_t* total_lens,
                                         const int32_t* chunk_lens, int32_t* labels, int32_t* label_frames, int cap,
                                         int32_t* fresh, void* state, int N, void* stream) {
  MS_REQUIRE(x && labels && state, "null pointer");
  MS_REQUIRE(rows > 0 && V > 0 && N > 0 && n > 0 && n <= N, "bad shape");
  MS_REQUIRE(cap > 0, "label capacity must be positive");
  MS_REQUIRE((total_lens == nullptr) != (chunk_lens == nullptr), "exactly one of total_lens / chunk_lens");
  if (V > 64)
    hipLaunchKernelGGL(ctc_greedy_stream_kernel<true>, dim3(N), dim3(64), 0, (hipStream_t)stream, x, rows, n, V, blank,
                       total_lens, chunk_lens, labels, label_frames, cap, fresh, (int32_t*)state);
  else
    hipLaunchKernelGGL(ctc_greedy_stream_kernel<false>, dim3(N), dim3(64), 0, (hipStream_t)stream, x, rows, n, V, blank,
                       total_lens, chunk_lens, labels, label_frames, cap, fresh, (int32_t*)state);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
