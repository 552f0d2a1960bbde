// CTC forced alignment: the Viterbi (max-plus) twin of ctc.hip's alpha recursion, with back-pointers, the back-trace and the
// token spans on the device.  The specification is the comment on ms_ctc_align in include/ms_hotpath.h; tests/ctc_align_ref.py
// restates it in numpy.  No MFMA: a scan kernel, one workgroup per utterance, like ctc_alpha_kernel.
//
//   launch 1  ctc_align_normalise_kernel  a wave per (frame, utterance): the frame's log-softmax normaliser (logits in) or 0
//                                         (log-probabilities in); NaN where the frame is not usable (non-finite normaliser;
//                                         a NaN / +inf log-probability)
//   launch 2  ctc_align_kernel            frame loop (d in an LDS double buffer, one LDS-only barrier per frame), back-trace
//                                         by one lane, spans and token sums in parallel
//
// States are dealt to the threads with a stride of the workgroup (s = tid + 256 j), not in consecutive runs: the three LDS
// reads of a frame are then conflict-free for any S, and the 64 states of one wave iteration are exactly one "group" of the
// back-pointer row.  A back-pointer is 2 bits; a group's 64 of them are stored as two 64-bit planes (bit 0 of every lane's k,
// bit 1 of every lane's k) that the wave gets from two ballots -- no shuffles, no atomics, one 16-byte store by lane 0.
// A row is ceil(S_max / 64) groups = 16 bytes per 64 states (the same 2 bits per state as 16 per 32-bit word).
// The rows live in LDS when T rows fit AL_BP_LDS_BYTES (the back-trace is then a chain of T LDS reads), else in the global
// workspace (a chain of T L2 round trips).
#include <math.h>

#include "common.h"

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_T = 8192;                      // path [T] in LDS: 32 KB
constexpr int AL_MAX_L = 1023;                      // labels, d double buffer [3][2 L + 1] in LDS: 24 KB
constexpr size_t AL_BP_LDS_BYTES = 96 * 1024;       // back-pointer rows kept in LDS up to this size (MS_CTC_ALIGN_BP_LDS_BYTES)

static_assert(AL_BP_LDS_BYTES == MS_CTC_ALIGN_BP_LDS_BYTES, "the header documents the budget");
constexpr size_t AL_LDS_MAX = 160 * 1024 - 1024;    // dynamic LDS of a launch (the workgroup-wide OR keeps a few static words)
static_assert(AL_BP_LDS_BYTES + (size_t)AL_MAX_T * 4 + (size_t)3 * (2 * AL_MAX_L + 1) * 4 + 16 <= AL_LDS_MAX, "LDS of a CU");

typedef unsigned long long u64;

inline int bp_groups(int S_max) { return (S_max + 63) / 64; }
inline size_t bp_row_bytes(int S_max) { return (size_t)bp_groups(S_max) * 2 * sizeof(u64); }
inline bool bp_in_lds(int T, int S_max) { return (size_t)T * bp_row_bytes(S_max) <= AL_BP_LDS_BYTES; }

__device__ __forceinline__ float al_neg_inf() { return -INFINITY; }
__device__ __forceinline__ float al_nan() { return __uint_as_float(0x7fc00000u); }

// logz[n][t] for t < in_lens[n]: logsumexp_v x[t, n, :] (0 with log-probabilities in); NaN marks a frame that poisons the
// utterance.  The precise expf / logf: this is the device's log-softmax the specification speaks of, off the recursion's chain.
__global__ __launch_bounds__(256) void ctc_align_normalise_kernel(const float* __restrict__ x, const int32_t* __restrict__ in_lens,
                                                                  float* __restrict__ logz_ws, int T, int N, int V,
                                                                  int log_probs_in) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // frame-major: consecutive waves read consecutive rows
  if (f >= (long)T * N) return;
  const int t = (int)(f / N), n = (int)(f - (long)t * N);
  if (t >= min(max(in_lens[n], 0), T)) return;
  const float* row = x + (size_t)f * V;
  float lz;
  if (log_probs_in) {
    int bad = 0;                                                   // (an int in a VGPR, not a loop-carried bool: ctc.hip)
    for (int v = lane; v < V; v += 64) {
      const float c = row[v];
      bad |= (c != c || c == INFINITY) ? 1 : 0;
    }
    lz = (__ballot(bad != 0) != 0ull) ? al_nan() : 0.f;
  } else {
    float m = al_neg_inf();
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    lz = logf(sum) + m;
    if (!(fabsf(lz) < INFINITY)) lz = al_nan();                    // a NaN or +inf logit, a row of -inf
  }
  if (lane == 0) logz_ws[(size_t)n * T + t] = lz;
}

// An utterance without a path: every frame -1, every span (-1, -1), every token log-probability `sc` (-inf or NaN; an
// utterance with no labels has no tokens and gets here with its score 0 when it has no frames either).
__device__ __forceinline__ void al_write_no_path(float sc, int n, int tid, int T, int L, int L_max, float* score,
                                                 int32_t* frame_state, int32_t* token_start, int32_t* token_end,
                                                 float* token_logp) {
  if (tid == 0) score[n] = sc;
  for (int t = tid; t < T; t += AL_THREADS) frame_state[(size_t)n * T + t] = -1;
  for (int i = tid; i < L_max; i += AL_THREADS) {
    token_start[(size_t)n * L_max + i] = -1;
    token_end[(size_t)n * L_max + i] = -1;
    token_logp[(size_t)n * L_max + i] = (i < L) ? sc : 0.f;
  }
}

// LDS: [back-pointer rows [T][G][2] u64 (BP_LDS)] path [T] | ext [S_max] | d double buffer [2][S_max] | fin [2]
template <bool BP_LDS>
__global__ __launch_bounds__(AL_THREADS) void ctc_align_kernel(const float* __restrict__ x, const int32_t* __restrict__ in_lens,
                                                               const int32_t* __restrict__ targets,
                                                               const int32_t* __restrict__ tgt_offsets,
                                                               const int32_t* __restrict__ tgt_lens,
                                                               const float* __restrict__ logz_ws, u64* __restrict__ bp_ws,
                                                               float* __restrict__ score, int32_t* __restrict__ frame_state,
                                                               int32_t* __restrict__ token_start, int32_t* __restrict__ token_end,
                                                               float* __restrict__ token_logp, int T, int N, int V, int L_max,
                                                               int blank) {
  extern __shared__ __attribute__((aligned(16))) unsigned char al_smem[];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S_max = 2 * L_max + 1;
  const int G = (S_max + 63) >> 6;
  u64* bp_lds = reinterpret_cast<u64*>(al_smem);
  u64* bp_glb = bp_ws + (size_t)n * T * G * 2;
  int* path = reinterpret_cast<int*>(al_smem + (BP_LDS ? (size_t)T * G * 16 : 0));   // [T]
  int* ext = path + T;                                                              // [S_max]
  float* d0 = reinterpret_cast<float*>(ext + S_max);                                // [S_max]
  float* d1 = d0 + S_max;                                                           // [S_max]
  int* fin = reinterpret_cast<int*>(d1 + S_max);                                    // [2] final state (-1: none), score bits

  const int Tn = min(max(in_lens[n], 0), T);
  const int Lraw = tgt_lens[n];
  int invalid = (Lraw < 0 || Lraw > L_max) ? 1 : 0;          // (the caller's error; the LDS rows are sized by L_max)
  const int L = min(max(Lraw, 0), L_max);
  const int S = 2 * L + 1;
  const float* logz = logz_ws + (size_t)n * T;
  const int32_t* tg = targets + tgt_offsets[n];

  for (int s = tid; s < S; s += AL_THREADS) {
    int lab = blank;
    if (s & 1) {
      lab = tg[s >> 1];
      // a label outside [0, V) or equal to the blank: no alignment, and no row is ever indexed with it
      if (lab < 0 || lab >= V || lab == blank) { invalid = 1; lab = blank; }
    }
    ext[s] = lab;
    d0[s] = al_neg_inf();
  }
  int bad = 0;
  for (int t = tid; t < Tn; t += AL_THREADS) bad |= (fabsf(logz[t]) < INFINITY) ? 0 : 1;
  // (two votes: __syncthreads_or answers "non-zero for any thread", not the OR of the threads' values)
  const int any_bad = __syncthreads_or(bad);
  const int any_invalid = __syncthreads_or(invalid);
  if (any_bad || any_invalid) {
    al_write_no_path(any_bad ? al_nan() : al_neg_inf(), n, tid, T, L, L_max, score, frame_state, token_start, token_end,
                     token_logp);
    return;
  }
  if (Tn == 0) {
    al_write_no_path(L == 0 ? 0.f : al_neg_inf(), n, tid, T, L, L_max, score, frame_state, token_start, token_end, token_logp);
    return;
  }
  {
    const float* row = x + (size_t)n * V;
    if (tid == 0) d0[0] = row[blank] - logz[0];
    if (tid == 1 && S > 1) d0[1] = row[ext[1]] - logz[0];
  }
  __syncthreads();

  float* cur = d0;
  float* nxt = d1;
  const int J = (S + AL_THREADS - 1) / AL_THREADS;
  // The frame's score of this thread's first state does not depend on the recursion: its two loads are issued one frame
  // AHEAD and meet in the subtraction only where the value is used, so the L2 latency runs under the previous frame's
  // barrier (as in ctc_alpha_kernel).  States past the first 256 load directly.
  const int lab0 = tid < S ? ext[tid] : blank;
  const bool skip0 = (tid & 1) && tid >= 3 && tid < S && lab0 != ext[tid - 2];
  // (the normaliser's index gets a per-lane zero the compiler cannot see through: a uniform address makes it a SCALAR load,
  // whose counter is the LDS reads' -- the frame would wait for it where it is issued)
  int vz;
  asm("v_mov_b32 %0, 0" : "=v"(vz));
  float x_next = 0.f, z_next = 0.f;
  if (Tn > 1 && tid < S) {
    x_next = x[((size_t)1 * N + n) * V + lab0];
    z_next = logz[1 + vz];
  }
  for (int t = 1; t < Tn; ++t) {
    const float* row = x + ((size_t)t * N + n) * V;
    const float x0 = x_next, z0 = z_next;
    if (t + 1 < Tn && tid < S) {
      x_next = x[((size_t)(t + 1) * N + n) * V + lab0];
      z_next = logz[t + 1 + vz];
    }
    for (int j = 0; j < J; ++j) {                     // J is uniform: every lane of a wave reaches the ballots
      const int s = tid + j * AL_THREADS;
      int k = 0;
      if (s < S) {
        bool skip;
        float lp;
        if (j == 0) {
          skip = skip0;
          lp = x0 - z0;
        } else {
          const int lab = ext[s];
          skip = (s & 1) && lab != ext[s - 2];
          lp = row[lab] - logz[t];
        }
        // the three reads issued together (clamped addresses, the values selected afterwards): one LDS latency per frame
        float best = cur[s];
        const float a1 = cur[max(s - 1, 0)], a2 = cur[max(s - 2, 0)];
        if (s >= 1 && a1 > best) { best = a1; k = 1; }
        if (skip && a2 > best) { best = a2; k = 2; }
        nxt[s] = best + lp;
      }
      const u64 lo = __ballot(k & 1), hi = __ballot(k >> 1);
      const int g = w + 4 * j;                        // this wave iteration's states are 64 g .. 64 g + 63
      if (lane == 0 && (g << 6) < S) {                // (g << 6 < S <= S_max: inside the row of G groups)
        if (BP_LDS) {
          bp_lds[((size_t)t * G + g) * 2] = lo;
          bp_lds[((size_t)t * G + g) * 2 + 1] = hi;
        } else {
          bp_glb[((size_t)t * G + g) * 2] = lo;
          bp_glb[((size_t)t * G + g) * 2 + 1] = hi;
        }
      }
    }
    // LDS-only barrier (ctc_alpha_kernel): __syncthreads() would also wait for the loads just issued for the NEXT frame
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's row is in the LDS
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  __syncthreads();   // (also: the back-pointer rows in the global workspace are visible to this workgroup's loads behind it)

  // end rule and back-trace: one lane walks T rows (LDS reads, or L2 round trips out of the workspace)
  if (tid == 0) {
    int fs = S - 1;
    if (S >= 2 && cur[S - 2] > cur[S - 1]) fs = S - 2;
    const float sc = cur[fs];
    fin[1] = __float_as_int(sc);
    if (sc == al_neg_inf()) {
      fin[0] = -1;
    } else {
      fin[0] = fs;
      int s = fs;
      for (int t = Tn - 1; t >= 1; --t) {
        path[t] = s;
        const size_t o = ((size_t)t * G + (s >> 6)) * 2;
        const u64 lo = BP_LDS ? bp_lds[o] : bp_glb[o];
        const u64 hi = BP_LDS ? bp_lds[o + 1] : bp_glb[o + 1];
        const int b = s & 63;
        s -= (int)((lo >> b) & 1ull) + 2 * (int)((hi >> b) & 1ull);
      }
      path[0] = s;
    }
  }
  __syncthreads();
  const float sc = __int_as_float(fin[1]);
  if (fin[0] < 0) {
    al_write_no_path(sc, n, tid, T, L, L_max, score, frame_state, token_start, token_end, token_logp);
    return;
  }
  if (tid == 0) score[n] = sc;

  // spans: a frame starts a token where its state is odd and differs from the previous frame's, and ends one where the next
  // frame's differs.  Every token of a path has frames (only blanks can be skipped), so all L entries get written.
  int* tstart = reinterpret_cast<int*>(d0);   // [L] (the d rows are done with)
  int* tend = reinterpret_cast<int*>(d1);     // [L]
  for (int i = tid; i < L; i += AL_THREADS) { tstart[i] = 0; tend[i] = 0; }   // (never an index made of a d row's bits)
  __syncthreads();
  for (int t = tid; t < T; t += AL_THREADS) {
    int st = -1;
    if (t < Tn) {
      st = path[t];
      if (st & 1) {
        if (t == 0 || path[t - 1] != st) tstart[st >> 1] = t;
        if (t == Tn - 1 || path[t + 1] != st) tend[st >> 1] = t + 1;
      }
    }
    frame_state[(size_t)n * T + t] = st;
  }
  __syncthreads();
  // one lane per token, its frames in ascending order: a fixed summation order
  for (int i = tid; i < L_max; i += AL_THREADS) {
    int a = -1, b = -1;
    float acc = 0.f;
    if (i < L) {
      a = tstart[i];
      b = tend[i];
      const int lab = ext[2 * i + 1];
      acc = x[((size_t)a * N + n) * V + lab] - logz[a];
      for (int t = a + 1; t < b; ++t) acc += x[((size_t)t * N + n) * V + lab] - logz[t];
    }
    token_start[(size_t)n * L_max + i] = a;
    token_end[(size_t)n * L_max + i] = b;
    token_logp[(size_t)n * L_max + i] = acc;
  }
}

size_t al_lds_bytes(int T, int S_max, bool in_lds) {
  return (in_lds ? (size_t)T * bp_row_bytes(S_max) : 0) + (size_t)T * 4 + (size_t)3 * S_max * 4 + 16;
}

}  // namespace

extern "C" size_t ms_ctc_align_workspace_bytes(int T, int N, int V, int S_max) {
  if (T <= 0 || N <= 0 || V <= 0) return 0;
  S_max = S_max < 1 ? 1 : S_max;
  // per-frame normalisers [N][T]; + the back-pointer rows [N][T][ceil(S_max / 64)][2] u64 when they do not fit the LDS budget
  return ms::align_up((size_t)T * N * sizeof(float), 256) +
         (bp_in_lds(T, S_max) ? 0 : ms::align_up((size_t)N * T * bp_row_bytes(S_max), 256));
}

extern "C" int ms_ctc_align(const float* x, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_offsets,
                            const int32_t* tgt_lens, float* score, int32_t* frame_state, int32_t* token_start,
                            int32_t* token_end, float* token_logp, int T, int N, int V, int L_max, int blank, int flags,
                            void* workspace, size_t workspace_bytes, void* stream) {
  MS_REQUIRE(x && in_lens && targets && tgt_offsets && tgt_lens && score && frame_state && workspace, "null pointer");
  MS_REQUIRE(T > 0 && N > 0 && V > 0 && L_max >= 0, "bad shape");
  MS_REQUIRE(L_max == 0 || (token_start && token_end && token_logp), "null pointer");
  MS_REQUIRE(blank >= 0 && blank < V, "blank out of range");
  MS_REQUIRE(flags == 0 || flags == MS_CTC_LOG_PROBS_IN, "flags takes 0 or MS_CTC_LOG_PROBS_IN");
  const long pairs = (long)T * N;
  if (T > AL_MAX_T || L_max > AL_MAX_L || (pairs + 3) / 4 > 0x7fffffffL) {
    ms::set_error("ms_ctc_align: supported up to T = 8192 frames and 1023 labels");
    return MS_ERR_UNSUPPORTED;
  }
  const int S_max = 2 * L_max + 1;
  if (workspace_bytes < ms_ctc_align_workspace_bytes(T, N, V, S_max)) {
    ms::set_error("ms_ctc_align: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  static ms::DeviceOnce attr_once;
  if (attr_once.need()) {
    MS_HIP(hipFuncSetAttribute((const void*)ctc_align_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AL_LDS_MAX));
    MS_HIP(hipFuncSetAttribute((const void*)ctc_align_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AL_LDS_MAX));
    attr_once.done();
  }
  hipStream_t st = (hipStream_t)stream;
  float* logz = (float*)workspace;
  u64* bp_ws = (u64*)((char*)workspace + ms::align_up((size_t)T * N * sizeof(float), 256));
  const int lpi = (flags & MS_CTC_LOG_PROBS_IN) ? 1 : 0;
  hipLaunchKernelGGL(ctc_align_normalise_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, x, in_lens, logz, T, N, V, lpi);
  MS_LAUNCH_CHECK();
  const bool in_lds = bp_in_lds(T, S_max);
  if (in_lds)
    hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(N), dim3(AL_THREADS), al_lds_bytes(T, S_max, true), st, x, in_lens, targets,
                       tgt_offsets, tgt_lens, logz, (u64*)nullptr, score, frame_state, token_start, token_end, token_logp, T, N, V,
                       L_max, blank);
  else
    hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(N), dim3(AL_THREADS), al_lds_bytes(T, S_max, false), st, x, in_lens, targets,
                       tgt_offsets, tgt_lens, logz, bp_ws, score, frame_state, token_start, token_end, token_logp, T, N, V, L_max,
                       blank);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
