// N-gram language model scorer of the beam search: backoff scores of every token (or of a candidate list) for every hypothesis, from
// ARPA tables resident in HBM (tavsr/lm/ngram.py builds them; include/tavsr.h states the layout and the semantics).
//
// One workgroup per hypothesis.  Phase 1: lane j < m (m = context length, at most order - 1) walks the trie along the context's
// suffix of length j + 1 - at most order - 1 binary searches - and leaves the suffix's node and backoff in LDS.  Phase 2: the lanes
// stride over the tokens; each runs down the suffixes, longest first, looking for its word among the node's children.
// Work per hypothesis: (order - 1)^2 + V (order - 1) binary searches over child ranges of at most n_unigrams words; no host read,
// no allocation, no atomics - plain loads and stores on the stream given.
#include "common.h"

namespace tavsr {
namespace {

constexpr int kMaxOrder = TAVSR_NGRAM_MAX_ORDER;

// the node of word `w` among the children of `node` (CSR over one numbering of all nodes; the words of a child range ascend), or -1
__device__ __forceinline__ int find_child(const int32_t* __restrict__ word, const int32_t* __restrict__ child_begin, int node, int w) {
  int lo = child_begin[node];
  const int end = child_begin[node + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (word[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < end && word[lo] == w) ? lo : -1;
}

__global__ __launch_bounds__(256) void ngram_score_kernel(const int32_t* __restrict__ word, const float* __restrict__ logp,
                                                          const float* __restrict__ backoff, const int32_t* __restrict__ child_begin,
                                                          int n_unigrams, int order, int bos_word, float unk_logp,
                                                          const int32_t* __restrict__ word_map, const int64_t* __restrict__ yseq,
                                                          int64_t ld_y, int L, int step, const int32_t* __restrict__ step_dev,
                                                          const int64_t* __restrict__ cand, int C, float alpha, float add,
                                                          int accumulate, float* __restrict__ out, int64_t ldo, int V) {
  __shared__ int s_ctx[kMaxOrder];        // the context's words, oldest first
  __shared__ int s_node[kMaxOrder];       // [j - 1]: node of the suffix of length j, -1 when it is not listed
  __shared__ float s_bo[kMaxOrder];       // [j - 1]: its backoff (0 when it is not listed)
  const int n = blockIdx.x, tid = threadIdx.x;
  int i = step_dev ? *step_dev : step;    // the hypothesis is yseq[n][0 .. i]: <sos> and i tokens
  i = i < 0 ? 0 : (i > L - 1 ? L - 1 : i);
  const int m = min(i + 1, order - 1);
  if (tid < m) {
    const int p = i + 1 - m + tid;
    int w = bos_word;                     // position 0 is <s>, whatever token stands there
    if (p > 0) {
      const int64_t t = yseq[n * ld_y + p];
      w = (t >= 0 && t < V) ? word_map[t] : -1;
    }
    s_ctx[tid] = w;
  }
  __syncthreads();
  if (tid < m) {
    const int j = tid + 1;
    int node = s_ctx[m - j];
    if (node >= n_unigrams) node = -1;
    for (int k = 1; k < j && node >= 0; ++k) {
      const int w = s_ctx[m - j + k];
      node = w >= 0 ? find_child(word, child_begin, node, w) : -1;
    }
    s_node[tid] = node;
    s_bo[tid] = node >= 0 ? backoff[node] : 0.f;
  }
  __syncthreads();
  const int count = cand ? C : V;
  for (int c = tid; c < count; c += 256) {
    int v = c;
    if (cand) {
      const int64_t t = cand[(int64_t)n * C + c];
      if (t < 0 || t >= V) continue;
      v = (int)t;
    }
    const int w = word_map[v];
    float acc = 0.f, s = 0.f;
    bool hit = false;
    for (int j = m; j >= 1; --j) {
      const int node = s_node[j - 1];
      if (node < 0) continue;             // a suffix that is not listed: backoff 0
      const int h = w >= 0 ? find_child(word, child_begin, node, w) : -1;
      if (h >= 0) {
        s = logp[h] + acc;
        hit = true;
        break;
      }
      acc += s_bo[j - 1];
    }
    if (!hit) s = ((w >= 0 && w < n_unigrams) ? logp[w] : unk_logp) + acc;
    float* o = out + (int64_t)n * ldo + v;
    const float r = alpha * s + add;
    *o = accumulate ? *o + r : r;
  }
}

}  // namespace
}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_ngram_score(const int32_t* word, const float* logp, const float* backoff, const int32_t* child_begin,
                                 int32_t n_unigrams, int32_t order, int32_t bos_word, float unk_logp, const int32_t* word_map,
                                 const int64_t* yseq, int64_t ld_y, int32_t L, int32_t step, const int32_t* step_dev,
                                 const int64_t* cand, int32_t C, float alpha, float add, int32_t accumulate, float* out, int64_t ldo,
                                 int32_t N, int32_t V, tavsr_stream_t stream) {
  TAVSR_REQUIRE(word && logp && backoff && child_begin && word_map, TAVSR_EINVAL, "ngram_score: null table");
  TAVSR_REQUIRE(yseq && out, TAVSR_EINVAL, "ngram_score: null pointer");
  TAVSR_REQUIRE(order >= 1, TAVSR_EINVAL, "ngram_score: order %d", order);
  TAVSR_REQUIRE(order <= TAVSR_NGRAM_MAX_ORDER, TAVSR_EUNSUPPORTED, "ngram_score: order %d exceeds the kernel's limit of %d", order,
                TAVSR_NGRAM_MAX_ORDER);
  TAVSR_REQUIRE(n_unigrams >= 1 && bos_word < n_unigrams && L >= 1 && ld_y >= L && ldo >= V && (!cand || C >= 0), TAVSR_EINVAL,
                "ngram_score: bad sizes (n_unigrams %d, bos_word %d, L %d, ld_y %lld, ldo %lld, V %d)", n_unigrams, bos_word, L,
                (long long)ld_y, (long long)ldo, V);
  if (N <= 0 || V <= 0) return TAVSR_OK;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, word, logp, backoff, child_begin,
                     n_unigrams, order, bos_word, unk_logp, word_map, yseq, ld_y, L, step, step_dev, cand, C, alpha, add, accumulate,
                     out, ldo, V);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
