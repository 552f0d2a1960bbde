// Word-level back-off n-gram language model resident on the device: the packed table (layout: include/ms_hotpath.h,
// "n-gram language model"; packer: myrtlespeech_amd/language_model.py) and the look-ups over it.  Included by beam.hip (the
// LM instantiations of the search kernel) and by ngram_lm.hip (ms_ngram_lm_score, ms_ngram_lm_table_check); both are
// compiled with -ffp-contract=off, and the factor is a chain of float32 multiplies in a fixed order, so both round alike
// and like NGramLanguageModel.factor on the host.
//
// Every probe loop is bounded by the probe count the packer recorded (and ms_ngram_lm_table_check limits to the table's
// size): a damaged table gives a wrong factor, never a kernel that does not end.  Keys are compared in full (64 bits); a
// spelling that is not in the vocabulary but hashes onto a stored key (probability ~ vocabulary / 2^64) is scored as that
// word, by the host walk and the device alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace ms_lm {

constexpr unsigned MAGIC = 0x4D4C534Du;      // "MSLM", little endian
constexpr int HEADER_BYTES = 64;
constexpr int MAX_ORDER = 5;                 // MS_NGRAM_MAX_ORDER
constexpr int HIST = MAX_ORDER - 1;          // word ids a search node carries (the last HIST complete words, -1 = none)
constexpr float NOT_COMPUTED = -1.0f;        // a node's cached factor before its first use (factors are >= 0)

// header words (uint32 each)
enum { H_MAGIC = 0, H_ORDER, H_VOCAB_LOG2, H_NGRAM_LOG2, H_VSEED_LO, H_VSEED_HI, H_NSEED_LO, H_NSEED_HI, H_BOS, H_UNK,
       H_VOCAB_PROBES, H_NGRAM_PROBES, H_VOCAB_OFF, H_NGRAM_OFF, H_BYTES, H_WORDS };

// what the kernels need of a table, made on the host from a header that passed the check (never read from device memory)
struct Tab {
  const uint4* vocab;   // {key lo, key hi, word id, 0}
  const uint4* ngram;   // {key lo, key hi, float32 p ** lm_weight, float32 backoff ** lm_weight}
  unsigned long long vocab_seed, ngram_seed;
  unsigned vocab_mask, ngram_mask;
  int vocab_probes, ngram_probes;
  int order, bos, unk;
};

// ---- the hash (language_model.py: _step / _fin are the same two functions on Python integers masked to 64 bits)
__host__ __device__ __forceinline__ unsigned long long step(unsigned long long h, unsigned x) {
  return (h ^ (unsigned long long)(x + 1u)) * 0x100000001B3ull;
}
__host__ __device__ __forceinline__ unsigned long long fin(unsigned long long h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h ? h : 1ull;      // 0 marks an empty slot
}

// Host: validate the 64 header bytes against the blob's size.  Returns nullptr if fine, else what is wrong.
inline const char* header_problem(const void* header_host, size_t bytes) {
  if (header_host == nullptr) return "null table";
  if (bytes < (size_t)HEADER_BYTES) return "table shorter than its header";
  uint32_t h[16];
  memcpy(h, header_host, sizeof(h));
  if (h[H_MAGIC] != MAGIC) return "wrong magic";
  if (h[H_ORDER] < 1 || h[H_ORDER] > (uint32_t)MAX_ORDER) return "order outside 1 .. 5";
  if (h[H_VOCAB_LOG2] > 27 || h[H_NGRAM_LOG2] > 27) return "slot count is not a power of two below 2^28";
  const size_t vs = (size_t)1 << h[H_VOCAB_LOG2], ns = (size_t)1 << h[H_NGRAM_LOG2];
  if (h[H_BYTES] != bytes) return "recorded size differs from the size given";
  if (h[H_VOCAB_OFF] % 16 || h[H_NGRAM_OFF] % 16 || h[H_VOCAB_OFF] < (uint32_t)HEADER_BYTES || h[H_NGRAM_OFF] < (uint32_t)HEADER_BYTES)
    return "table offset misaligned or inside the header";
  if ((size_t)h[H_VOCAB_OFF] + vs * 16 > bytes || (size_t)h[H_NGRAM_OFF] + ns * 16 > bytes) return "table extends past the end";
  if (h[H_VOCAB_PROBES] < 1 || h[H_VOCAB_PROBES] > vs || h[H_NGRAM_PROBES] < 1 || h[H_NGRAM_PROBES] > ns)
    return "probe bound outside 1 .. slots";
  const int32_t bos = (int32_t)h[H_BOS], unk = (int32_t)h[H_UNK];
  if (bos < -1 || bos >= (int32_t)h[H_WORDS] || unk < 0 || unk >= (int32_t)h[H_WORDS]) return "special word id out of range";
  return nullptr;
}

// Host: the kernel argument for a checked header and the table's device address.
inline Tab make_tab(const void* header_host, const void* table_dev) {
  uint32_t h[16];
  memcpy(h, header_host, sizeof(h));
  Tab t;
  const char* base = (const char*)table_dev;
  t.vocab = (const uint4*)(base + h[H_VOCAB_OFF]);
  t.ngram = (const uint4*)(base + h[H_NGRAM_OFF]);
  t.vocab_seed = (unsigned long long)h[H_VSEED_LO] | ((unsigned long long)h[H_VSEED_HI] << 32);
  t.ngram_seed = (unsigned long long)h[H_NSEED_LO] | ((unsigned long long)h[H_NSEED_HI] << 32);
  t.vocab_mask = (1u << h[H_VOCAB_LOG2]) - 1u;
  t.ngram_mask = (1u << h[H_NGRAM_LOG2]) - 1u;
  t.vocab_probes = (int)h[H_VOCAB_PROBES];
  t.ngram_probes = (int)h[H_NGRAM_PROBES];
  t.order = (int)h[H_ORDER]; t.bos = (int32_t)h[H_BOS]; t.unk = (int32_t)h[H_UNK];
  return t;
}

#if defined(__HIPCC__)
// The probe loops run the recorded number of probes WITHOUT an early exit: the trip count is the same word for every lane, so
// the loop needs no per-lane exit mask (hipcc has misplaced those in this library's kernels before: tools/isa_lanemask_audit.py),
// the loads of one look-up do not depend on each other and go out back to back, and the result is that of the sequential
// walk -- the first slot that holds the key, unless an empty slot comes first.
// MS_LM_WHOLE_SLOT(e): an empty asm that "modifies" the slot's four words -- the slot is fetched whole, by one
// global_load_dwordx4, where it is written.  Left alone hipcc fetches the key first and the value words behind a per-lane
// branch on the comparison: a second dependent round trip, and a conditional block inside the loop.
#define MS_LM_WHOLE_SLOT(e) asm volatile("" : "+v"((e).x), "+v"((e).y), "+v"((e).z), "+v"((e).w))
// id of the word whose running spelling hash is `h` (step() over its symbols from vocab_seed); unknown spelling: <unk>
__device__ __forceinline__ int vocab_id(const Tab& t, unsigned long long h) {
  const unsigned long long key = fin(h);
  const unsigned slot = (unsigned)key & t.vocab_mask;
  int id = t.unk;
  bool open = true;
  for (int i = 0; i < t.vocab_probes; ++i) {
    uint4 e = t.vocab[(slot + (unsigned)i) & t.vocab_mask];
    MS_LM_WHOLE_SLOT(e);
    const unsigned long long k = (unsigned long long)e.x | ((unsigned long long)e.y << 32);
    id = (open && k == key) ? (int)e.z : id;
    open = open && k != key && k != 0ull;
  }
  return id;
}

// n-gram entry under `key`: true and its two factors if stored
__device__ __forceinline__ bool ngram_find(const Tab& t, unsigned long long key, float& pf, float& bf) {
  const unsigned slot = (unsigned)key & t.ngram_mask;
  bool open = true;
  int found = 0;
  pf = 1.0f; bf = 1.0f;
  for (int i = 0; i < t.ngram_probes; ++i) {
    uint4 e = t.ngram[(slot + (unsigned)i) & t.ngram_mask];
    MS_LM_WHOLE_SLOT(e);
    const unsigned long long k = (unsigned long long)e.x | ((unsigned long long)e.y << 32);
    const bool hit = open && k == key;
    pf = hit ? __uint_as_float(e.z) : pf;
    bf = hit ? __uint_as_float(e.w) : bf;
    found = hit ? 1 : found;
    open = open && k != key && k != 0ull;
  }
  // (the answer leaves the loop as a number in a VGPR, not as the loop's lane mask: whoever branches on it compares again there)
  asm volatile("" : "+v"(found));
  return found != 0;
}

// key of the n-gram made of the last `k` entries of hist followed (with_word) by `w`: the ids folded from ngram_seed, then
// the n-gram's order
__device__ __forceinline__ unsigned long long ngram_key(const Tab& t, const int (&hist)[HIST], int k, bool with_word, int w) {
  unsigned long long h = t.ngram_seed;
#pragma unroll
  for (int j = 0; j < HIST; ++j)
    if (j >= HIST - k) h = step(h, (unsigned)hist[j]);
  if (with_word) h = step(h, (unsigned)w);
  return fin(step(h, (unsigned)(k + (with_word ? 1 : 0))));
}

// The factor of the word with spelling hash `word_hash` after the history `hist` (oldest first, -1 = no word): back-off from
// the longest stored context, float32 product from 1 of the back-off factors met and then the probability factor.
__device__ __forceinline__ float factor(const Tab& t, unsigned long long word_hash, const int (&hist)[HIST]) {
  const int w = vocab_id(t, word_hash);
  int kc = 0;
#pragma unroll
  for (int k = 1; k <= HIST; ++k)
    if (k < t.order && kc == k - 1 && hist[HIST - k] >= 0) kc = k;
  // Every level's two look-ups are made by every lane, whether or not the lane's walk gets there: nothing here branches per
  // lane, no look-up waits for another one's answer (the sequential walk is 2 .. 2 x order + 1 DEPENDENT round trips), and the
  // answers are then applied in the walk's order.  k runs over the same values for every lane; a lane joins at its own
  // context length.
  float f = 1.0f;
  int done = 0;      // (with a table from the packer always set in the end: every word id has a unigram)
#pragma unroll
  for (int k = HIST; k >= 0; --k) {      // (unrolled: k is a constant in every copy, the copies beyond the model's order are skipped)
    if (k >= t.order) continue;
    float pf, bf, ctx_pf, ctx_bf = 1.0f;
    const int hit = ngram_find(t, ngram_key(t, hist, k, true, w), pf, bf) ? 1 : 0;
    int ctx_hit = 0;
    if (k > 0) ctx_hit = ngram_find(t, ngram_key(t, hist, k, false, 0), ctx_pf, ctx_bf) ? 1 : 0;
    const int on = (done == 0 && k <= kc) ? 1 : 0;
    const float with_p = f * pf, with_b = f * ctx_bf;
    f = (on & hit) ? with_p : ((on & (hit ^ 1) & ctx_hit) ? with_b : f);
    done |= on & hit;
  }
  return f;
}

// history after the word `id` has been completed
__device__ __forceinline__ void push_word(int (&hist)[HIST], int id) {
#pragma unroll
  for (int j = 0; j + 1 < HIST; ++j) hist[j] = hist[j + 1];
  hist[HIST - 1] = id;
}
#endif

}  // namespace ms_lm
