// Training step on the device (OWN specification, include/ms_hotpath.h "training: optimizer step"): the global gradient norm,
// the clip, and the fused clip + SGD / Adam update over a LIST of float32 tensors.
//
// How a list reaches a kernel: by value.  The host cuts the list into pages of PAGE tensors; a page -- the device pointers of
// each array, the element counts and the running chunk count -- is the kernel's argument, so there is no device table, no
// upload and no pinned staging that a later call could overwrite under a copy still in flight.  One launch per page: the 48
// parameter tensors of the full-size DeepSpeech2 are one launch.  Tensors with no elements take no slot.
//
// Launch shape: a tensor is cut into chunks of CHUNK = 4096 elements; a page's (tensor, chunk) pairs are numbered in list order
// and a grid capped at MAX_GRID workgroups strides over them (the tensor of a chunk is found by bisection in the page's running
// counts: uniform, scalar loads).  No atomics, no workgroup waits on another, nothing is read back.
//
// Alignment: every base is only 4-byte aligned.  The update kernels key the cut on the PARAMETER's address: the 0..3 elements in
// front of its first 16-byte boundary are the head (scalar, chunk 0), the chunks start at that boundary, and what is left of the
// last quad is the tail (scalar).  Each other array moves in 16-byte quads where its own address at the body's start is 16-byte
// aligned and element by element otherwise -- the same bits either way, every operation is per element.  The norm kernel cuts by
// ELEMENT INDEX alone (quad q of a chunk = elements 4q .. 4q+3), because there the cut decides the order of the additions, and
// that order may depend on the element counts only; a gradient at an odd offset is read element by element into the same quads.
//
// Compiled with -ffp-contract=off (Makefile): every multiply and add below rounds on its own, as the numpy restatement in
// tests/optim_ref.py does.  Square root and division are the plain `sqrtf` and `/`: hipcc's default
// (-fhip-fp32-correctly-rounded-divide-sqrt) expands them to the correctly rounded sequences -- v_sqrt_f32 with its two fma
// corrections, v_div_scale / v_rcp / fma / v_div_fmas / v_div_fixup -- whereas this toolchain's __fsqrt_rn is the bare 1-ulp
// v_sqrt_f32 (it cost one element in 21 000 its last bit against the restatement).
#include "common.h"

namespace {

constexpr int PAGE = 48;          // tensors per launch
constexpr int CHUNK = 4096;       // elements per (tensor, chunk) pair
constexpr int THREADS = 256;
constexpr int MAX_GRID = 2048;
constexpr long long MAX_NUMEL = 1ll << 40;

template <int NARR>
struct Page {
  float* a[NARR][PAGE];
  long long numel[PAGE];
  unsigned cstart[PAGE + 1];      // chunks of the page's tensors before tensor i; [count] = the page's chunks
  unsigned head[PAGE];            // elements in front of the body (update kernels; 0 in the norm's pages)
  unsigned part_base;             // first partial of this page (norm)
  int count;
};

__device__ __forceinline__ int find_tensor(const unsigned* cstart, int count, unsigned c) {
  int lo = 0, hi = count - 1;     // largest i with cstart[i] <= c
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cstart[mid] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ ms::f32x4 load4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const ms::f32x4*>(p);
  ms::f32x4 v;
  v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
  return v;
}
__device__ __forceinline__ void store4(float* p, bool vec, ms::f32x4 v) {
  if (vec) { *reinterpret_cast<ms::f32x4*>(p) = v; return; }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

// c = q where q = max_norm / (norm + 1e-6f) is below 1 or NaN, else 1 (a select, not fminf: a NaN norm poisons the step)
__device__ __forceinline__ float clip_coef(const float* norm, float max_norm) {
  const float q = max_norm / (norm[0] + 1e-6f);
  return (q < 1.0f || q != q) ? q : 1.0f;
}

// ---- norm -----------------------------------------------------------------------------------------------------------------
// partial[part_base + c] = sum of g*g over chunk c: thread u adds the quads u, u + 256, ... in ascending order, each quad as
// ((g0 g0 + g1 g1) + g2 g2) + g3 g3 onto the running sum; the 64 lanes of a wave meet in a butterfly (every lane ends with the
// same bits) and the four waves are added in ascending order.
__device__ __forceinline__ float block_sum(float acc, float* lds) {
  for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = acc;
  __syncthreads();
  float s = lds[0];
  for (int w = 1; w < THREADS / 64; ++w) s = s + lds[w];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(THREADS) void norm_partials_kernel(const Page<1> pg, float* __restrict__ partial) {
  __shared__ float lds[THREADS / 64];
  const unsigned total = pg.cstart[pg.count];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    const int ti = find_tensor(pg.cstart, pg.count, c);
    const long long base = (long long)(c - pg.cstart[ti]) * CHUNK;
    const long long left = pg.numel[ti] - base;
    const int len = left < CHUNK ? (int)left : CHUNK;
    const float* g = pg.a[0][ti] + base;
    const bool vec = aligned16(g);
    const int nq = len >> 2;
    float acc = 0.0f;
    for (int q = threadIdx.x; q < nq; q += THREADS) {
      const ms::f32x4 v = load4(g + 4 * q, vec);
      acc = acc + (((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w);
    }
    if ((int)threadIdx.x == (nq & (THREADS - 1))) {      // the chunk's last 1..3 elements, on the thread whose quad they would be
      float t = 0.0f;
      for (int i = 4 * nq; i < len; ++i) t = t + g[i] * g[i];
      acc = acc + t;
    }
    const float s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[pg.part_base + c] = s;
  }
}

// out[0] = sqrt(sum of the partials), out[1] = 1 where that is NaN or infinite: one workgroup, thread u adds the partials
// u, u + 256, ... in ascending order, then the same meeting as above
__global__ __launch_bounds__(THREADS) void norm_final_kernel(const float* __restrict__ partial, unsigned n, float* __restrict__ out) {
  __shared__ float lds[THREADS / 64];
  float acc = 0.0f;
  for (unsigned i = threadIdx.x; i < n; i += THREADS) acc = acc + partial[i];
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) {
    const float r = sqrtf(s);
    out[0] = r;
    out[1] = (r != r || __builtin_fabsf(r) == __builtin_inff()) ? 1.0f : 0.0f;
  }
}

// ---- element-wise passes ----------------------------------------------------------------------------------------------------
// The shared walk of the clip and the two steps over a page of OP::NARR arrays; array 0 decides the cut (head, quads, tail).
// OP::quad(ptrs, vec, i) does the arithmetic on elements i .. i+3 (vec[k]: array k moves as one 16-byte quad there),
// OP::one(ptrs, i) on element i.
template <class OP>
__device__ __forceinline__ void walk_page(const Page<OP::NARR>& pg, const OP& op) {
  const unsigned total = pg.cstart[pg.count];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    const int ti = find_tensor(pg.cstart, pg.count, c);
    const unsigned ci = c - pg.cstart[ti];
    const long long numel = pg.numel[ti];
    const int head = (int)pg.head[ti];
    float* p[OP::NARR];
#pragma unroll
    for (int k = 0; k < OP::NARR; ++k) p[k] = pg.a[k][ti];
    if (ci == 0 && (int)threadIdx.x < head) op.one(p, (long long)threadIdx.x);
    const long long base = head + (long long)ci * CHUNK;
    const long long left = numel - base;
    if (left <= 0) continue;
    const int len = left < CHUNK ? (int)left : CHUNK;
    bool vec[OP::NARR];
#pragma unroll
    for (int k = 0; k < OP::NARR; ++k) vec[k] = p[k] != nullptr && aligned16(p[k] + base);
    const int nq = len >> 2;
    for (int q = threadIdx.x; q < nq; q += THREADS) op.quad(p, vec, base + 4 * q);
    if ((int)threadIdx.x < len - 4 * nq) op.one(p, base + 4 * nq + threadIdx.x);
  }
}

struct ClipOp {
  static constexpr int NARR = 1;
  float c;
  __device__ __forceinline__ void one(float* const* p, long long i) const { p[0][i] = p[0][i] * c; }
  __device__ __forceinline__ void quad(float* const* p, const bool* vec, long long i) const {
    ms::f32x4 g = load4(p[0] + i, vec[0]);
    g.x = g.x * c; g.y = g.y * c; g.z = g.z * c; g.w = g.w * c;
    store4(p[0] + i, vec[0], g);
  }
};

__global__ __launch_bounds__(THREADS) void clip_kernel(const Page<1> pg, const float* __restrict__ norm, float max_norm) {
  ClipOp op;
  op.c = clip_coef(norm, max_norm);
  walk_page(pg, op);
}

// arrays: 0 p, 1 g, 2 momentum buffer (NULL pointers when momentum == 0)
struct SgdOp {
  static constexpr int NARR = 3;
  float lr, momentum, weight_decay, c;
  bool nesterov, clip;
  __device__ __forceinline__ float step(float p, float g, float& b, bool has_b) const {
    float d = clip ? g * c : g;
    if (weight_decay != 0.0f) d = d + weight_decay * p;
    float u = d;
    if (has_b) {
      b = momentum * b + d;
      u = nesterov ? d + momentum * b : b;
    }
    return p - lr * u;
  }
  __device__ __forceinline__ void one(float* const* p, long long i) const {
    const bool has_b = p[2] != nullptr;
    float b = has_b ? p[2][i] : 0.0f;
    p[0][i] = step(p[0][i], p[1][i], b, has_b);
    if (has_b) p[2][i] = b;
  }
  __device__ __forceinline__ void quad(float* const* p, const bool* vec, long long i) const {
    const bool has_b = p[2] != nullptr;
    ms::f32x4 w = load4(p[0] + i, vec[0]);
    const ms::f32x4 g = load4(p[1] + i, vec[1]);
    ms::f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
    if (has_b) b = load4(p[2] + i, vec[2]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float bj = b[j];
      w[j] = step(w[j], g[j], bj, has_b);
      b[j] = bj;
    }
    store4(p[0] + i, vec[0], w);
    if (has_b) store4(p[2] + i, vec[2], b);
  }
};

__global__ __launch_bounds__(THREADS) void sgd_kernel(const Page<3> pg, float lr, float momentum, float weight_decay, int nesterov,
                                                      const float* __restrict__ norm, float max_norm, int skip_nonfinite) {
  if (skip_nonfinite && norm[1] != 0.0f) return;      // a skipped step writes nothing
  SgdOp op;
  op.lr = lr; op.momentum = momentum; op.weight_decay = weight_decay; op.nesterov = nesterov != 0;
  op.clip = norm != nullptr;
  op.c = op.clip ? clip_coef(norm, max_norm) : 1.0f;
  walk_page(pg, op);
}

// arrays: 0 p, 1 g, 2 exp_avg, 3 exp_avg_sq, 4 max_exp_avg_sq (NULL pointers without amsgrad)
struct AdamOp {
  static constexpr int NARR = 5;
  float beta1, omb1, beta2, omb2, eps, weight_decay, step_size, rsqrt_bc2, c;
  bool clip;
  __device__ __forceinline__ float step(float p, float g, float& m, float& v, float& vmax, bool ams) const {
    float d = clip ? g * c : g;
    if (weight_decay != 0.0f) d = d + weight_decay * p;
    m = beta1 * m + omb1 * d;
    v = beta2 * v + (omb2 * d) * d;
    float w = v;
    if (ams) {
      vmax = (v > vmax || v != v) ? v : vmax;      // a select: a NaN v is taken, a NaN vmax stays
      w = vmax;
    }
    const float den = sqrtf(w) / rsqrt_bc2 + eps;
    return p - step_size * (m / den);
  }
  __device__ __forceinline__ void one(float* const* p, long long i) const {
    const bool ams = p[4] != nullptr;
    float m = p[2][i], v = p[3][i], vmax = ams ? p[4][i] : 0.0f;
    p[0][i] = step(p[0][i], p[1][i], m, v, vmax, ams);
    p[2][i] = m;
    p[3][i] = v;
    if (ams) p[4][i] = vmax;
  }
  __device__ __forceinline__ void quad(float* const* p, const bool* vec, long long i) const {
    const bool ams = p[4] != nullptr;
    ms::f32x4 w = load4(p[0] + i, vec[0]);
    const ms::f32x4 g = load4(p[1] + i, vec[1]);
    ms::f32x4 m = load4(p[2] + i, vec[2]);
    ms::f32x4 v = load4(p[3] + i, vec[3]);
    ms::f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ams) x = load4(p[4] + i, vec[4]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j], vj = v[j], xj = x[j];
      w[j] = step(w[j], g[j], mj, vj, xj, ams);
      m[j] = mj; v[j] = vj; x[j] = xj;
    }
    store4(p[0] + i, vec[0], w);
    store4(p[2] + i, vec[2], m);
    store4(p[3] + i, vec[3], v);
    if (ams) store4(p[4] + i, vec[4], x);
  }
};

__global__ __launch_bounds__(THREADS) void adam_kernel(const Page<5> pg, float beta1, float omb1, float beta2, float omb2, float eps,
                                                       float weight_decay, float step_size, float rsqrt_bc2,
                                                       const float* __restrict__ norm, float max_norm, int skip_nonfinite) {
  if (skip_nonfinite && norm[1] != 0.0f) return;
  AdamOp op;
  op.beta1 = beta1; op.omb1 = omb1; op.beta2 = beta2; op.omb2 = omb2; op.eps = eps; op.weight_decay = weight_decay;
  op.step_size = step_size; op.rsqrt_bc2 = rsqrt_bc2;
  op.clip = norm != nullptr;
  op.c = op.clip ? clip_coef(norm, max_norm) : 1.0f;
  walk_page(pg, op);
}

// ---- host: lists into pages -------------------------------------------------------------------------------------------------
inline unsigned norm_chunks(long long numel) { return (unsigned)((numel + CHUNK - 1) / CHUNK); }

// Fills pages from the lists and hands each to `launch(page)`.  arrays[k] may be NULL (that array is absent: NULL pointers in
// the page).  `by_address`: cut on array 0's alignment (update kernels) instead of the element index (norm).
template <int NARR, class F>
int for_each_page(void* const* const* arrays, const int64_t* numels, int n, bool by_address, F launch) {
  Page<NARR> pg;
  pg.count = 0;
  pg.cstart[0] = 0;
  unsigned part = 0;
  pg.part_base = 0;
  for (int i = 0; i <= n; ++i) {
    if (i < n && numels[i] != 0) {
      const int s = pg.count;
      for (int k = 0; k < NARR; ++k) pg.a[k][s] = arrays[k] ? static_cast<float*>(arrays[k][i]) : nullptr;
      unsigned head = 0;
      if (by_address) head = (unsigned)((4 - ((reinterpret_cast<uintptr_t>(arrays[0][i]) >> 2) & 3)) & 3);
      if ((long long)head > numels[i]) head = (unsigned)numels[i];
      const long long body = numels[i] - head;
      unsigned chunks = norm_chunks(body);
      if (chunks == 0) chunks = 1;      // (a tensor that is all head still needs its chunk 0)
      pg.numel[s] = numels[i];
      pg.head[s] = head;
      pg.cstart[s + 1] = pg.cstart[s] + chunks;
      pg.count = s + 1;
    }
    if (pg.count == PAGE || (i == n && pg.count > 0)) {
      const int rc = launch(pg);
      if (rc != MS_OK) return rc;
      part += pg.cstart[pg.count];
      pg.part_base = part;
      pg.count = 0;
    }
  }
  return MS_OK;
}

template <int NARR>
inline unsigned grid_of(const Page<NARR>& pg) {
  const unsigned total = pg.cstart[pg.count];
  return total < (unsigned)MAX_GRID ? total : (unsigned)MAX_GRID;
}

int check_list(const char* what, void* const* ptrs, const int64_t* numels, int n, bool need) {
  if (ptrs == nullptr) {
    MS_REQUIRE(!need || n == 0, std::string(what) + " is NULL");
    return MS_OK;
  }
  for (int i = 0; i < n; ++i) {
    MS_REQUIRE(numels[i] == 0 || ptrs[i] != nullptr, std::string(what) + " holds a NULL pointer for a tensor with elements");
    MS_REQUIRE((reinterpret_cast<uintptr_t>(ptrs[i]) & 3u) == 0, std::string(what) + " holds a pointer that is not 4-byte aligned");
  }
  return MS_OK;
}

int check_numels(const int64_t* numels, int n) {
  MS_REQUIRE(n >= 0, "n is negative");
  MS_REQUIRE(n == 0 || numels != nullptr, "numels_host is NULL");
  for (int i = 0; i < n; ++i) MS_REQUIRE(numels[i] >= 0 && numels[i] < MAX_NUMEL, "an element count is negative or 2^40 or more");
  return MS_OK;
}

size_t total_partials(const int64_t* numels, int n) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += norm_chunks(numels[i]);
  return total;
}

}  // namespace

extern "C" {

size_t ms_grad_norm_workspace_bytes(const int64_t* numels_host, int n) {
  if (numels_host == nullptr || n <= 0) return 256;
  for (int i = 0; i < n; ++i)
    if (numels_host[i] < 0 || numels_host[i] >= MAX_NUMEL) return 256;
  return ms::align_up(total_partials(numels_host, n) * sizeof(float), 256) + 256;
}

int ms_grad_norm(void* const* grads_host, const int64_t* numels_host, int n, float* norm_out, void* workspace,
                 size_t workspace_bytes, void* stream) {
  int rc = check_numels(numels_host, n);
  if (rc != MS_OK) return rc;
  rc = check_list("grads_host", grads_host, numels_host, n, true);
  if (rc != MS_OK) return rc;
  MS_REQUIRE(norm_out != nullptr && workspace != nullptr, "norm_out or workspace is NULL");
  const size_t total = total_partials(numels_host, n);
  MS_REQUIRE(total < (1ull << 31), "more than 2^31 chunks");
  if (workspace_bytes < ms_grad_norm_workspace_bytes(numels_host, n)) {
    ms::set_error("ms_grad_norm: workspace too small");
    return MS_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  void* const* arrays[1] = {grads_host};
  rc = for_each_page<1>(arrays, numels_host, n, false, [&](const Page<1>& pg) -> int {
    norm_partials_kernel<<<grid_of(pg), THREADS, 0, st>>>(pg, partial);
    MS_LAUNCH_CHECK();
    return MS_OK;
  });
  if (rc != MS_OK) return rc;
  norm_final_kernel<<<1, THREADS, 0, st>>>(partial, (unsigned)total, norm_out);
  MS_LAUNCH_CHECK();
  return MS_OK;
}

int ms_grad_clip(void* const* grads_host, const int64_t* numels_host, int n, const float* norm, float max_norm, void* stream) {
  int rc = check_numels(numels_host, n);
  if (rc != MS_OK) return rc;
  rc = check_list("grads_host", grads_host, numels_host, n, true);
  if (rc != MS_OK) return rc;
  MS_REQUIRE(norm != nullptr, "norm is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  void* const* arrays[1] = {grads_host};
  return for_each_page<1>(arrays, numels_host, n, true, [&](const Page<1>& pg) -> int {
    clip_kernel<<<grid_of(pg), THREADS, 0, st>>>(pg, norm, max_norm);
    MS_LAUNCH_CHECK();
    return MS_OK;
  });
}

int ms_sgd_step(void* const* params_host, void* const* grads_host, void* const* bufs_host, const int64_t* numels_host, int n,
                float lr, float momentum, float weight_decay, int nesterov, const float* norm, float max_norm,
                int skip_nonfinite, void* stream) {
  int rc = check_numels(numels_host, n);
  if (rc != MS_OK) return rc;
  if ((rc = check_list("params_host", params_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("grads_host", grads_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("bufs_host", bufs_host, numels_host, n, false)) != MS_OK) return rc;
  MS_REQUIRE((momentum != 0.0f) == (bufs_host != nullptr) || n == 0, "bufs_host goes with a non-zero momentum, and only with one");
  MS_REQUIRE(!nesterov || momentum != 0.0f, "nesterov needs a momentum");
  MS_REQUIRE(!skip_nonfinite || norm != nullptr, "skip_nonfinite needs norm");
  hipStream_t st = static_cast<hipStream_t>(stream);
  void* const* arrays[3] = {params_host, grads_host, bufs_host};
  return for_each_page<3>(arrays, numels_host, n, true, [&](const Page<3>& pg) -> int {
    sgd_kernel<<<grid_of(pg), THREADS, 0, st>>>(pg, lr, momentum, weight_decay, nesterov, norm, max_norm, skip_nonfinite);
    MS_LAUNCH_CHECK();
    return MS_OK;
  });
}

int ms_adam_step(void* const* params_host, void* const* grads_host, void* const* exp_avg_host, void* const* exp_avg_sq_host,
                 void* const* max_exp_avg_sq_host, const int64_t* numels_host, int n, float beta1, float beta2, float eps,
                 float weight_decay, float step_size, float rsqrt_bc2, const float* norm, float max_norm, int skip_nonfinite,
                 void* stream) {
  int rc = check_numels(numels_host, n);
  if (rc != MS_OK) return rc;
  if ((rc = check_list("params_host", params_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("grads_host", grads_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("exp_avg_host", exp_avg_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("exp_avg_sq_host", exp_avg_sq_host, numels_host, n, true)) != MS_OK) return rc;
  if ((rc = check_list("max_exp_avg_sq_host", max_exp_avg_sq_host, numels_host, n, false)) != MS_OK) return rc;
  MS_REQUIRE(!skip_nonfinite || norm != nullptr, "skip_nonfinite needs norm");
  // (1 - beta) in double, rounded once: the scalar the kernel multiplies by
  const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
  hipStream_t st = static_cast<hipStream_t>(stream);
  void* const* arrays[5] = {params_host, grads_host, exp_avg_host, exp_avg_sq_host, max_exp_avg_sq_host};
  return for_each_page<5>(arrays, numels_host, n, true, [&](const Page<5>& pg) -> int {
    adam_kernel<<<grid_of(pg), THREADS, 0, st>>>(pg, beta1, omb1, beta2, omb2, eps, weight_decay, step_size, rsqrt_bc2, norm,
                                                 max_norm, skip_nonfinite);
    MS_LAUNCH_CHECK();
    return MS_OK;
  });
}

}  // extern "C"
