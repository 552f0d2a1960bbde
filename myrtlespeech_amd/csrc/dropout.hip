// Dropout on the device (OWN specification, include/ms_hotpath.h "training: dropout"): the mask is a pure function of
// (seed, offset, element index, thr) -- Philox4x32-10, counter (q_lo, q_hi, offset_lo, offset_hi) with q = e >> 2, key
// (seed_lo, seed_hi), output word e & 3 -- so there is no generator state on the device and no stored mask: the backward calls
// the same kernel with the same four numbers and gets the same bits.
//
// Launch shape: one lane owns one Philox quad = elements 4q .. 4q+3 of the array; a grid capped at MAX_GRID workgroups strides
// over the quads; the n % 4 elements after the last whole quad are single elements of workgroup 0 (lane t takes word t of quad
// n >> 2).  The cut is by ELEMENT INDEX alone, never by address: a view at an odd element offset gets the same mask.  Each array
// moves as 16-byte quads where its own base is 16-byte aligned and element by element otherwise -- every operation is per
// element, so the bits are the same either way.  A lane reads its quad before it writes it: out may alias x.
//
// The uniform is never converted to float: an element is kept iff its 32-bit word r >= thr (thr in [1, 2^32], compared in 64
// bits, so thr = 2^32 keeps nothing), and the value is ONE float32 multiply x * m with m = scale or +0.0f -- not a select, so a
// NaN or an infinity in a dropped element stays visible (x * 0 = NaN) as in torch.nn.Dropout.
//
// Compiled with -ffp-contract=off (Makefile), as optim.hip is: the results are held bit for bit to tests/dropout_ref.py.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_GRID = 2048;

struct Call {
  unsigned long long thr;      // keep iff r >= thr
  float scale;
  unsigned key0, key1;         // seed_lo, seed_hi
  unsigned off0, off1;         // offset_lo, offset_hi
};

struct u32x4 { unsigned v[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(unsigned long long q, const Call& c) {
  unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = c.off0, c3 = c.off1;
  unsigned k0 = c.key0, k1 = c.key1;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  u32x4 r;
  r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
  return r;
}

__device__ __forceinline__ float mask_of(unsigned r, const Call& c) { return (unsigned long long)r >= c.thr ? c.scale : 0.0f; }

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

// GATE = false: out[e] = x[e] * m[e].  GATE = true: out[e] = (lo < y[e] && y[e] < hi) ? x[e] * m[e] : 0 (x is dy, out is dx;
// neither comparison holds for a NaN y, so such an element gets 0 as in _LinearClampFunction).
template <bool GATE>
__global__ __launch_bounds__(THREADS) void dropout_kernel(const float* x, const float* y, float* out, long long n, float lo, float hi,
                                                          const Call c) {
  const long long nq = n >> 2;
  const bool vx = aligned16(x), vo = aligned16(out), vy = GATE && aligned16(y);
  const long long stride = (long long)gridDim.x * THREADS;
  for (long long q = (long long)blockIdx.x * THREADS + threadIdx.x; q < nq; q += stride) {
    const u32x4 r = philox4x32_10((unsigned long long)q, c);
    ms::f32x4 v = load4(x + 4 * q, vx);
    ms::f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (GATE) g = load4(y + 4 * q, vy);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = v[j] * mask_of(r.v[j], c);
      if constexpr (GATE) v[j] = (lo < g[j] && g[j] < hi) ? d : 0.0f;
      else v[j] = d;
    }
    store4(out + 4 * q, vo, v);
  }
  const int tail = (int)(n - 4 * nq);
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const u32x4 r = philox4x32_10((unsigned long long)nq, c);
    const long long e = 4 * nq + threadIdx.x;
    unsigned word = r.v[0];      // (selects, not an index into r: the words stay in registers)
    if (threadIdx.x == 1) word = r.v[1];
    if (threadIdx.x == 2) word = r.v[2];
    const float d = x[e] * mask_of(word, c);
    if constexpr (GATE) out[e] = (lo < y[e] && y[e] < hi) ? d : 0.0f;
    else out[e] = d;
  }
}

inline unsigned grid_of(long long n) {
  const long long blocks = ((n >> 2) + THREADS - 1) / THREADS;
  return blocks < 1 ? 1u : (blocks < MAX_GRID ? (unsigned)blocks : (unsigned)MAX_GRID);
}

int check_call(int64_t n, uint64_t thr, float scale) {
  MS_REQUIRE(n >= 0, "n is negative");
  MS_REQUIRE(thr != 0, "thr is 0 (p must be above 0)");
  MS_REQUIRE(thr <= (1ull << 32), "thr is above 2^32 (p must be at most 1)");
  MS_REQUIRE(scale >= 0.0f && scale < __builtin_inff(), "scale is negative or not finite");
  return MS_OK;
}

Call make_call(uint64_t thr, float scale, uint64_t seed, uint64_t offset) {
  Call c;
  c.thr = thr;
  c.scale = scale;
  c.key0 = (unsigned)seed; c.key1 = (unsigned)(seed >> 32);
  c.off0 = (unsigned)offset; c.off1 = (unsigned)(offset >> 32);
  return c;
}

}  // namespace

extern "C" {

int ms_dropout_forward(const float* x, float* out, int64_t n, uint64_t thr, float scale, uint64_t seed, uint64_t offset,
                       void* stream) {
  const int rc = check_call(n, thr, scale);
  if (rc != MS_OK) return rc;
  if (n == 0) return MS_OK;
  MS_REQUIRE(x != nullptr && out != nullptr, "x or out is NULL");
  MS_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, "x or out is not 4-byte aligned");
  dropout_kernel<false><<<grid_of(n), THREADS, 0, static_cast<hipStream_t>(stream)>>>(x, nullptr, out, n, 0.0f, 0.0f,
                                                                                       make_call(thr, scale, seed, offset));
  MS_LAUNCH_CHECK();
  return MS_OK;
}

int ms_clamp_dropout_backward(const float* dy, const float* y, float* dx, int64_t n, float lo, float hi, uint64_t thr, float scale,
                              uint64_t seed, uint64_t offset, void* stream) {
  const int rc = check_call(n, thr, scale);
  if (rc != MS_OK) return rc;
  if (n == 0) return MS_OK;
  MS_REQUIRE(dy != nullptr && y != nullptr && dx != nullptr, "dy, y or dx is NULL");
  MS_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dx)) & 3u) == 0,
             "dy, y or dx is not 4-byte aligned");
  dropout_kernel<true><<<grid_of(n), THREADS, 0, static_cast<hipStream_t>(stream)>>>(dy, y, dx, n, lo, hi,
                                                                                      make_call(thr, scale, seed, offset));
  MS_LAUNCH_CHECK();
  return MS_OK;
}

}  // extern "C"
