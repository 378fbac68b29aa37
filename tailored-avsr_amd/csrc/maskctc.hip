// Mask-CTC decoding (src/models/maskctc_model.py:285-349), the token bookkeeping of MaskCTCInference.forward as two kernels:
//   maskctc_init : greedy CTC ids + frame maxima of the posteriors (:289), collapse of repeats (:290), per-token maximum
//                  probability over its run of frames (:298-305), blanks dropped (:291), low-confidence tokens masked (:311-320),
//                  and the iteration plan (:326-327, :332)
//   maskctc_step : one pass of the fill loop (:331-334, last pass :340) on the decoder's logits
// One workgroup per utterance, per-utterance state in LDS, integer outputs: bit-exact contract.  No host value is read or
// written, so a whole decode loop is one stream of launches (capturable).
// Mask-CTC training (src/models/maskctc_model.py:216-241, espnet maskctc/add_mask_token.py:mask_uniform):
//   mask_uniform : the MLM input / target pair of a batch, drawn on the device from the dropout generator's counter stream
//   count_recip  : 1 / max(1, sum of the per-utterance target counts) - the length-normalised loss's denominator
#include <float.h>
#include <math.h>

#include "common.h"

namespace tavsr {

// torch.argmax / torch.max order: NaN is the maximum, the lowest index wins among equals
__device__ __forceinline__ bool mc_better(float x, int xi, float best, int bi) {
  if (xi == 0x7fffffff) return false;
  if (bi == 0x7fffffff) return true;
  return (x > best) || (x != x && best == best) || ((x == best || (x != x && best != best)) && xi < bi);
}

// row maximum and its index over V columns by one wave (all 64 lanes active); result uniform over the wave
__device__ __forceinline__ void mc_row_argmax(const float* __restrict__ row, int V, int lane, float& best, int& bi) {
  best = -INFINITY;
  bi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float x = row[v];
    if (mc_better(x, v, best, bi)) { best = x; bi = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (mc_better(ob, oi, best, bi)) { best = ob; bi = oi; }
  }
}

// inclusive scan of s_cnt[1..256] (s_cnt[0] = 0) by wave 0, four counts per lane (as embed_bwd_kernel)
__device__ __forceinline__ void mc_scan256(int* s_cnt, int t) {
  if (t < 64) {
    int a0 = s_cnt[4 * t + 1], a1 = a0 + s_cnt[4 * t + 2], a2 = a1 + s_cnt[4 * t + 3], a3 = a2 + s_cnt[4 * t + 4];
    int run = a3;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(run, o, 64);
      if (t >= o) run += up;
    }
    const int base = run - a3;
    s_cnt[4 * t + 1] = base + a0; s_cnt[4 * t + 2] = base + a1; s_cnt[4 * t + 3] = base + a2; s_cnt[4 * t + 4] = base + a3;
  }
}

// Dynamic LDS: T ints (frame ids) + T floats (frame maxima of the posterior).
// The run scan is flags + a block prefix sum for the output positions; the thread that owns the first frame of a run walks the run for
// its maximum (runs are a few frames long; an utterance that is one long run costs what the serial loop of ctc_greedy_kernel costs).
__global__ __launch_bounds__(256) void maskctc_init_kernel(const float* __restrict__ logits, int64_t ld_t, int64_t ld_b,
                                                           const int64_t* __restrict__ hlens, int blank, int mask_token,
                                                           double thr, int n_iter, int64_t* __restrict__ y_in,
                                                           int64_t* __restrict__ y_hat, float* __restrict__ tok_prob,
                                                           int64_t ld_y, int64_t* __restrict__ y_len,
                                                           int32_t* __restrict__ plan, int T, int V) {
  extern __shared__ int mc_sm[];
  int* s_id = mc_sm;
  float* s_p = reinterpret_cast<float*>(mc_sm + T);
  __shared__ int s_cnt[257];
  __shared__ int s_masks;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int Tb = hlens ? (int)max((int64_t)0, min((int64_t)T, hlens[b])) : T;
  const float* lg = logits + (int64_t)b * ld_b;
  if (tid == 0) s_masks = 0;
  for (int t = wv; t < Tb; t += 4) {
    const float* row = lg + (int64_t)t * ld_t;
    float best;
    int bi;
    mc_row_argmax(row, V, lane, best, bi);
    float se = 0.f;
    for (int v = lane; v < V; v += 64) se += expf(row[v] - best);
    se = wave_sum(se);
    if (lane == 0) { s_id[t] = bi; s_p[t] = 1.f / se; }
  }
  __syncthreads();
  // kept runs: a frame that differs from its predecessor and is not blank starts one
  const int per = (Tb + 255) / 256;
  const int t0 = min(Tb, tid * per), t1 = min(Tb, t0 + per);
  int cnt = 0;
  for (int t = t0; t < t1; ++t) cnt += (s_id[t] != blank) && (t == 0 || s_id[t] != s_id[t - 1]);
  s_cnt[tid + 1] = cnt;
  if (tid == 0) s_cnt[0] = 0;
  __syncthreads();
  mc_scan256(s_cnt, tid);
  __syncthreads();
  int pos = s_cnt[tid];
  const int n = s_cnt[256];
  int64_t* yi = y_in + (int64_t)b * ld_y;
  int64_t* yh = y_hat + (int64_t)b * ld_y;
  float* tp = tok_prob + (int64_t)b * ld_y;
  int masks = 0;
  for (int t = t0; t < t1; ++t) {
    const int c = s_id[t];
    if (c == blank || (t > 0 && c == s_id[t - 1])) continue;
    float m = -1.f;      // maskctc_model.py:301-304: starts at -1, replaced where strictly smaller
    for (int e = t; e < Tb && s_id[e] == c; ++e)
      if (m < s_p[e]) m = s_p[e];
    const bool masked = (double)m < thr;
    yh[pos] = c;
    tp[pos] = m;
    yi[pos] = masked ? mask_token : c;
    masks += masked;
    ++pos;
  }
  if (masks) atomicAdd(&s_masks, masks);
  for (int64_t l = n + tid; l < ld_y; l += 256) { yi[l] = 0; yh[l] = 0; tp[l] = 0.f; }
  __syncthreads();
  if (tid == 0) {
    const int mask_num = s_masks;
    const int num_iter = (mask_num >= n_iter && n_iter > 0) ? n_iter : mask_num;
    y_len[b] = n;
    plan[3 * b + 0] = mask_num;
    plan[3 * b + 1] = num_iter;
    plan[3 * b + 2] = num_iter > 0 ? mask_num / num_iter : 0;
  }
}

// topk order of the candidates: NaN is the largest, equal scores go to the lower position
__device__ __forceinline__ bool mc_before(float a, int ai, float b, int bi) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return an;
  if (!an && a != b) return a > b;
  return ai < bi;
}

// Dynamic LDS: L floats (row maxima of the masked positions) + L ints (their argmax, -1 where the position is not masked).
__global__ __launch_bounds__(256) void maskctc_step_kernel(const float* __restrict__ logits, int64_t ld_l, int64_t ld_b,
                                                           int64_t* __restrict__ y_in, int64_t ld_y,
                                                           const int64_t* __restrict__ y_len,
                                                           const int32_t* __restrict__ plan, int it, int mask_token, int L,
                                                           int V1) {
  extern __shared__ int mc_sm[];
  float* s_score = reinterpret_cast<float*>(mc_sm);
  int* s_arg = mc_sm + L;
  __shared__ int s_nm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int num_iter = plan[3 * b + 1];
  if (it >= num_iter) return;      // this utterance is finished (uniform over the workgroup)
  const int n = (int)max((int64_t)0, min((int64_t)L, y_len[b]));
  int64_t* yi = y_in + (int64_t)b * ld_y;
  const float* lg = logits + (int64_t)b * ld_b;
  if (tid == 0) s_nm = 0;
  __syncthreads();
  for (int l = wv; l < n; l += 4) {
    if (yi[l] != mask_token) {      // (uniform over the wave)
      if (lane == 0) s_arg[l] = -1;
      continue;
    }
    float best;
    int bi;
    mc_row_argmax(lg + (int64_t)l * ld_l, V1, lane, best, bi);
    if (lane == 0) { s_score[l] = best; s_arg[l] = bi; atomicAdd(&s_nm, 1); }
  }
  __syncthreads();
  if (it == num_iter - 1) {      // maskctc_model.py:339-340: everything still masked takes its argmax
    for (int l = tid; l < n; l += 256)
      if (s_arg[l] >= 0) yi[l] = s_arg[l];
    return;
  }
  const int k = min(plan[3 * b + 2], s_nm);
  for (int l = tid; l < n; l += 256) {
    if (s_arg[l] < 0) continue;
    const float sc = s_score[l];
    int rank = 0;
    for (int j = 0; j < n && rank < k; ++j)
      if (j != l && s_arg[j] >= 0 && mc_before(s_score[j], j, sc, l)) ++rank;
    if (rank < k) yi[l] = s_arg[l];
  }
}

// word (c & 3) of philox4x32_10(counter = c / 4, key = seed): the counter -> word mapping of dropout.hip
__device__ __forceinline__ uint32_t mc_word(uint64_t c, uint64_t seed) {
  const uint64_t ctr = c >> 2;
  uint32_t r[4];
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const int k = (int)(c & 3);      // (selects, not a dynamically indexed register array)
  return k == 0 ? r[0] : k == 1 ? r[1] : k == 2 ? r[2] : r[3];
}

// Dynamic LDS: Lmax ints (column of text the compacted token l came from) + Lmax ints (mask flags).
// The draws are WITH replacement: several j may hit one position, all of them store the same 1 (idempotent), and one pass
// afterwards writes both rows - every element of ys_in[b][0:Lmax] and ys_out[b][0:Lmax] exactly once, padding included.
__global__ __launch_bounds__(256) void mask_uniform_kernel(const int64_t* __restrict__ text, int64_t ld_text, int Lmax,
                                                           int mask_token, int eos, int ignore_id,
                                                           const uint64_t* __restrict__ seed, uint64_t offset, uint64_t S,
                                                           int64_t* __restrict__ ys_in, int64_t* __restrict__ ys_out,
                                                           int64_t ld_y, int32_t* __restrict__ n_target) {
  extern __shared__ int mc_sm[];
  int* s_src = mc_sm;
  int* s_flag = mc_sm + Lmax;
  __shared__ int s_cnt[257];
  __shared__ int s_masks;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = text + (int64_t)b * ld_text;
  const int per = (Lmax + 255) / 256;
  const int l0 = min(Lmax, tid * per), l1 = min(Lmax, l0 + per);
  int cnt = 0;
  for (int l = l0; l < l1; ++l) cnt += row[l] != (int64_t)ignore_id;
  s_cnt[tid + 1] = cnt;
  if (tid == 0) { s_cnt[0] = 0; s_masks = 0; }
  for (int l = tid; l < Lmax; l += 256) s_flag[l] = 0;
  __syncthreads();
  mc_scan256(s_cnt, tid);
  __syncthreads();
  int pos = s_cnt[tid];
  const int len = s_cnt[256];
  for (int l = l0; l < l1; ++l)
    if (row[l] != (int64_t)ignore_id) s_src[pos++] = l;
  if (len > 0) {
    const uint64_t sd = seed[0], base = offset + (uint64_t)b * S;
    const int n = 1 + (int)__umulhi(mc_word(base, sd), (uint32_t)len);      // randint(1, len + 1)
    for (int j = tid; j < n; j += 256) s_flag[__umulhi(mc_word(base + 1 + (uint64_t)j, sd), (uint32_t)len)] = 1;
  }
  __syncthreads();
  int64_t* yi = ys_in + (int64_t)b * ld_y;
  int64_t* yo = ys_out + (int64_t)b * ld_y;
  int masks = 0;
  for (int l = tid; l < Lmax; l += 256) {
    const bool real = l < len;
    const bool masked = real && s_flag[l];
    const int64_t tok = real ? row[s_src[l]] : (int64_t)eos;
    yi[l] = masked ? (int64_t)mask_token : tok;
    yo[l] = masked ? tok : (int64_t)ignore_id;
    masks += masked;
  }
  if (n_target) {
    if (masks) atomicAdd(&s_masks, masks);      // (integer, in LDS: the sum does not depend on the order)
    __syncthreads();
    if (tid == 0) n_target[b] = s_masks;
  }
}

// inv[0] = 1 / max(1, sum_b n[b]) by one wave: integer sum, one fp32 division
__global__ __launch_bounds__(64) void count_recip_kernel(const int32_t* __restrict__ n, int B, float* __restrict__ inv) {
  const int lane = threadIdx.x;
  int s = 0;
  for (int b = lane; b < B; b += 64) s += n[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) inv[0] = 1.f / (float)(s > 1 ? s : 1);
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_maskctc_init(const float* logits, int64_t ld_t, int64_t ld_b, const int64_t* hlens, int32_t blank,
                                  int32_t mask_token, double threshold, int32_t n_iterations, int64_t* y_in, int64_t* y_hat,
                                  float* tok_prob, int64_t ld_y, int64_t* y_len, int32_t* plan, int32_t B, int32_t T, int32_t V,
                                  tavsr_stream_t stream) {
  TAVSR_REQUIRE(logits && y_in && y_hat && tok_prob && y_len && plan, TAVSR_EINVAL, "maskctc_init: null pointer");
  TAVSR_REQUIRE(V >= 1 && T >= 0 && ld_y >= T && ld_y >= 1, TAVSR_EINVAL, "maskctc_init: V >= 1, ld_y >= max(T, 1) required");
  TAVSR_REQUIRE(mask_token >= 0, TAVSR_EINVAL, "maskctc_init: mask_token < 0");
  if (B <= 0) return TAVSR_OK;
  const size_t lds = (size_t)(T > 0 ? T : 1) * 8;
  TAVSR_REQUIRE(lds <= 60000, TAVSR_EUNSUPPORTED, "maskctc_init: T=%d exceeds the LDS budget of the frame table", T);
  hipLaunchKernelGGL(maskctc_init_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, logits, ld_t, ld_b, hlens, blank,
                     mask_token, threshold, n_iterations, y_in, y_hat, tok_prob, ld_y, y_len, plan, T, V);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_maskctc_step(const float* logits, int64_t ld_l, int64_t ld_b, int64_t* y_in, int64_t ld_y,
                                  const int64_t* y_len, const int32_t* plan, int32_t it, int32_t mask_token, int32_t B,
                                  int32_t L, int32_t V1, tavsr_stream_t stream) {
  TAVSR_REQUIRE(logits && y_in && y_len && plan, TAVSR_EINVAL, "maskctc_step: null pointer");
  TAVSR_REQUIRE(V1 >= 2, TAVSR_EINVAL, "maskctc_step: V + 1 >= 2 required (got %d)", V1);
  TAVSR_REQUIRE(it >= 0, TAVSR_EINVAL, "maskctc_step: it < 0");
  TAVSR_REQUIRE(L >= 0 && ld_y >= L && mask_token >= 0 && mask_token < V1, TAVSR_EINVAL,
                "maskctc_step: ld_y >= L >= 0 and 0 <= mask_token < V + 1 required");
  if (B <= 0 || L == 0) return TAVSR_OK;
  const size_t lds = (size_t)L * 8;
  TAVSR_REQUIRE(lds <= 60000, TAVSR_EUNSUPPORTED, "maskctc_step: L=%d exceeds the LDS budget of the candidate table", L);
  hipLaunchKernelGGL(maskctc_step_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, logits, ld_l, ld_b, y_in, ld_y, y_len,
                     plan, it, mask_token, L, V1);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_mask_uniform(const int64_t* text, int64_t ld_text, int32_t B, int32_t Lmax, int32_t mask_token,
                                  int32_t eos, int32_t ignore_id, const uint64_t* seed_dev, uint64_t offset, int64_t* ys_in,
                                  int64_t* ys_out, int64_t ld_y, int32_t* n_target, tavsr_stream_t stream) {
  TAVSR_REQUIRE(Lmax >= 0 && ld_text >= Lmax && ld_y >= Lmax, TAVSR_EINVAL, "mask_uniform: ld_text, ld_y >= Lmax >= 0 required");
  TAVSR_REQUIRE(Lmax <= TAVSR_MASK_UNIFORM_MAX_L, TAVSR_EUNSUPPORTED,
                "mask_uniform: Lmax=%d exceeds the kernel's limit of %d tokens per row", Lmax, TAVSR_MASK_UNIFORM_MAX_L);
  TAVSR_REQUIRE(B <= 0 || (seed_dev && (Lmax == 0 || (text && ys_in && ys_out))), TAVSR_EINVAL, "mask_uniform: null pointer");
  if (B <= 0) return TAVSR_OK;
  const uint64_t S = ((uint64_t)Lmax + 1 + 3) / 4 * 4;
  hipLaunchKernelGGL(mask_uniform_kernel, dim3(B), dim3(256), (size_t)(Lmax > 0 ? Lmax : 1) * 8, (hipStream_t)stream, text,
                     ld_text, Lmax, mask_token, eos, ignore_id, seed_dev, offset, S, ys_in, ys_out, ld_y, n_target);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_count_recip(const int32_t* n, int32_t B, float* inv, tavsr_stream_t stream) {
  TAVSR_REQUIRE(inv && (n || B <= 0), TAVSR_EINVAL, "count_recip: null pointer");
  hipLaunchKernelGGL(count_recip_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n, B > 0 ? B : 0, inv);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
