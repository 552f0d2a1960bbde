// ms_ngram_lm_table_check / ms_ngram_lm_score: the packed n-gram table's host-side validation, and a kernel that scores
// padded prefixes against a table with the very look-ups the beam search uses (ngram_lm.h).  The score kernel is how the
// device walk is tested against NGramLanguageModel.factor without a beam search in the way.  -ffp-contract=off, as beam.hip.
#include "common.h"
#include "ngram_lm.h"

namespace {

// One thread per prefix.  The prefix is tokenised as NGramLanguageModel does: one trailing separator (the `+ (sep,)` of the
// decoder's question) is dropped, words are the runs between separators, the scored word is what follows the last separator.
__global__ __launch_bounds__(256) void ngram_score_kernel(ms_lm::Tab tab, const int32_t* prefixes, const int32_t* prefix_lens,
                                                          float* out, int P, int L, int sep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const int32_t* s = prefixes + (size_t)i * L;
  int n = min(max(prefix_lens[i], 0), L);
  if (n > 0 && s[n - 1] == sep) --n;
  int hist[ms_lm::HIST];
#pragma unroll
  for (int j = 0; j < ms_lm::HIST; ++j) hist[j] = -1;
  hist[ms_lm::HIST - 1] = tab.bos;
  unsigned long long h = tab.vocab_seed;
  int word_len = 0;
  for (int k = 0; k < n; ++k) {
    const int c = s[k];
    if (c == sep) {
      if (word_len > 0) ms_lm::push_word(hist, ms_lm::vocab_id(tab, h));
      h = tab.vocab_seed;
      word_len = 0;
    } else {
      h = ms_lm::step(h, (unsigned)c);
      ++word_len;
    }
  }
  out[i] = word_len > 0 ? ms_lm::factor(tab, h, hist) : 1.0f;
}

}  // namespace

extern "C" int ms_ngram_lm_table_check(const void* blob_host, size_t bytes) {
  const char* bad = ms_lm::header_problem(blob_host, bytes);
  if (bad) {
    ms::set_error(std::string("ms_ngram_lm_table_check: ") + bad);
    return MS_ERR_INVALID;
  }
  return MS_OK;
}

extern "C" int ms_ngram_lm_score(const void* table, const void* header_host, size_t table_bytes, const int32_t* prefixes,
                                 const int32_t* prefix_lens, float* out, int P, int L, int separator, void* stream) {
  MS_REQUIRE(table && prefixes && prefix_lens && out, "null pointer");
  MS_REQUIRE(P > 0 && L > 0, "bad shape");
  const char* bad = ms_lm::header_problem(header_host, table_bytes);
  MS_REQUIRE(bad == nullptr, bad ? bad : "");
  const ms_lm::Tab tab = ms_lm::make_tab(header_host, table);
  hipLaunchKernelGGL(ngram_score_kernel, dim3(ms::cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, tab, prefixes, prefix_lens, out,
                     P, L, separator);
  MS_LAUNCH_CHECK();
  return MS_OK;
}
