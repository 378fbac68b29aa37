// Validation error rates on the device: what ErrorCalculator (tavsr/models/espnet_model.py; espnet
// nets/e2e_asr_common.py ErrorCalculator) computes from the argmax ids and the transcripts of a batch, with no host read.
//   * edit_distance_rows: one workgroup per pair of padded int32 symbol rows, the lattice core of editdist.h.
//   * error_counts: one workgroup per (utterance, mode).  It expands the token ids of the hypothesis and of the reference
//     into symbol sequences held in LDS (code points through the calculator's token table, or word indices), runs the same
//     core and writes the edit count and the reference length.  Integers throughout; the n x m lattice exists nowhere.
// LDS of one workgroup (32-bit words; capH / capR = the most symbols a hypothesis / reference row can expand to):
//   16 header | 256 scan | capH + capR symbols | 3 (capR + 1) diagonals | words mode: 3 NW (word start, length, index)
#include "editdist.h"

namespace tavsr {

constexpr int kErrLdsBytes = 160 * 1024;
constexpr int kErrThreads = 256;
constexpr int kErrHeader = 16;
constexpr int kWordFlag = 1 << 30;      // words mode: the whitespace flag rides above the 21 bits of a code point

__global__ __launch_bounds__(kErrThreads) void edit_distance_rows_kernel(const int32_t* __restrict__ hyp, int64_t ldh,
                                                                         const int32_t* __restrict__ hyp_len, int max_hyp,
                                                                         const int32_t* __restrict__ ref, int64_t ldr,
                                                                         const int32_t* __restrict__ ref_len, int max_ref,
                                                                         int32_t* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  const int p = blockIdx.x;
  const int Lh = min(max(hyp_len[p], 0), max_hyp), Lr = min(max(ref_len[p], 0), max_ref);
  const int d = edit_distance_core(ref + p * ldr, Lr, hyp + p * ldh, Lh, lds, max_ref + 1);
  if (threadIdx.x == 0) dist[p] = d;
}

// exclusive prefix of one value per thread over the block (`tmp`: kErrThreads words); `total` = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int32_t* tmp, int& total) {
  const int tid = threadIdx.x;
  __syncthreads();      // tmp may still be read from the previous scan
  tmp[tid] = v;
  __syncthreads();
  for (int s = 1; s < kErrThreads; s <<= 1) {
    const int add = tid >= s ? tmp[tid - s] : 0;
    __syncthreads();
    tmp[tid] += add;
    __syncthreads();
  }
  total = tmp[kErrThreads - 1];
  return tmp[tid] - v;
}

struct ErrTables {
  const int32_t* span;        // [3][V + 1]: token v of text x owns cps[span[x][v] .. span[x][v + 1])
  const int32_t* cps;         // code points of the three texts
  const uint8_t* cp_space;    // per entry of cps: str.isspace()
  const uint8_t* drop;        // [V]: blank / space, dropped by the CTC character mode
  int V, tok_max;
};

enum { kTextRaw = 0, kTextHyp = 1, kTextRef = 2 };
enum { kModeCtcChars = 0, kModeAttChars = 1, kModeAttWords = 2 };

// ids[0 .. n) -> symbols out[0 .. returned count).  A kept position emits its token's code points of text `text`;
// collapse: a position equal to its left neighbour is skipped first; use_drop: tokens with drop[] set are skipped;
// no_blank_char: U+0020 is not emitted; flag_space: whitespace code points carry kWordFlag.  An id outside [0, V) emits
// nothing (-1 is the padding; the host route raises or wraps on any other).  Thread t owns `per` consecutive positions.
__device__ int expand_row(const int64_t* __restrict__ ids, int n, const ErrTables& tb, int text, bool collapse, bool use_drop,
                          bool no_blank_char, bool flag_space, int32_t* out, int cap, int32_t* scan_tmp) {
  const int per = (n + kErrThreads - 1) / kErrThreads;
  const int t0 = min((int)threadIdx.x * per, n), t1 = min(t0 + per, n);
  const int32_t* span = tb.span + (size_t)text * (tb.V + 1);
  int count = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int at = 0;
    if (pass == 1) {
      int total;
      at = block_excl_scan(count, scan_tmp, total);
      count = total;
    }
    for (int t = t0; t < t1; ++t) {
      const int64_t id = ids[t];
      if (id < 0 || id >= tb.V) continue;
      if (collapse && t > 0 && ids[t - 1] == id) continue;
      if (use_drop && tb.drop[id]) continue;
      const int s0 = span[id], s1 = min(span[id + 1], s0 + tb.tok_max);
      for (int s = s0; s < s1; ++s) {
        const int32_t cp = tb.cps[s];
        if (no_blank_char && cp == 0x20) continue;
        if (pass == 0) ++count;
        else if (at < cap) out[at++] = flag_space && tb.cp_space[s] ? (cp | kWordFlag) : cp;
      }
    }
  }
  return count;      // pass 1 left the block's total here, the same in every thread
}

// text[0 .. n) with whitespace flags -> (start, length) of its words, the maximal runs of unflagged code points, appended at
// word index w0; returns the number of words.  Thread t owns `per` consecutive characters.
__device__ int split_words(const int32_t* text, int n, int base, int32_t* wstart, int32_t* wlen, int w0, int32_t* scan_tmp) {
  const int per = (n + kErrThreads - 1) / kErrThreads;
  const int c0 = min((int)threadIdx.x * per, n), c1 = min(c0 + per, n);
  auto starts = [&](int c) { return !(text[c] & kWordFlag) && (c == 0 || (text[c - 1] & kWordFlag)); };
  int count = 0;
  for (int c = c0; c < c1; ++c) count += starts(c) ? 1 : 0;
  int total;
  int w = w0 + block_excl_scan(count, scan_tmp, total);
  for (int c = c0; c < c1; ++c)
    if (starts(c)) {
      int e = c + 1;
      while (e < n && !(text[e] & kWordFlag)) ++e;
      wstart[w] = base + c;
      wlen[w] = e - c;
      ++w;
    }
  return total;
}

__global__ __launch_bounds__(kErrThreads) void error_counts_kernel(const int64_t* __restrict__ ys_hat, int64_t ld_hat, int Th,
                                                                   const int64_t* __restrict__ ys_pad, int64_t ld_pad, int L,
                                                                   ErrTables tb, int modes, int capH_ctc, int capH_att, int capR,
                                                                   int32_t* __restrict__ errs, int32_t* __restrict__ ref_n, int B) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  const int b = blockIdx.x;
  int mode = 0;
  for (int seen = -1; mode < 3; ++mode)
    if ((modes >> mode) & 1)
      if (++seen == (int)blockIdx.y) break;
  const int capH = mode == kModeCtcChars ? capH_ctc : capH_att;
  int32_t* head = lds;
  int32_t* scan_tmp = head + kErrHeader;
  int32_t* symH = scan_tmp + kErrThreads;
  int32_t* symR = symH + capH;
  int32_t* diag = symR + capR;
  int32_t* wstart = diag + 3 * (capR + 1);
  const int NW = (capH + 1) / 2 + (capR + 1) / 2;
  int32_t* wlen = wstart + NW;
  int32_t* widx = wlen + NW;
  const int64_t* hat = ys_hat + b * ld_hat;
  const int64_t* pad = ys_pad + b * ld_pad;

  int Nh, Nr;
  if (mode == kModeCtcChars) {
    Nh = expand_row(hat, Th, tb, kTextRaw, true, true, false, false, symH, capH, scan_tmp);
    Nr = expand_row(pad, L, tb, kTextRaw, false, true, false, false, symR, capR, scan_tmp);
  } else {
    if (threadIdx.x == 0) head[0] = L;
    __syncthreads();
    for (int t = threadIdx.x; t < L; t += kErrThreads)
      if (pad[t] == -1) atomicMin(&head[0], t);
    __syncthreads();
    const int ymax = min(head[0], Th);      // the hypothesis is cut at the first -1 of the reference row
    const bool words = mode == kModeAttWords;
    Nh = expand_row(hat, ymax, tb, kTextHyp, false, false, !words, words, symH, capH, scan_tmp);
    Nr = expand_row(pad, L, tb, kTextRef, false, false, !words, words, symR, capR, scan_tmp);
    if (words) {
      __syncthreads();
      // symH and symR are one buffer: a word is (start, length) in it, hypothesis words first
      const int Wh = split_words(symH, min(Nh, capH), 0, wstart, wlen, 0, scan_tmp);
      const int Wr = split_words(symR, min(Nr, capR), capH, wstart, wlen, Wh, scan_tmp);
      __syncthreads();
      // a word's symbol is the index of the first identical word of the utterance: exact identity by direct comparison
      for (int w = threadIdx.x; w < Wh + Wr; w += kErrThreads) {
        const int n = wlen[w];
        const int32_t* me = symH + wstart[w];
        int first = w;
        for (int u = 0; u < w; ++u) {
          if (wlen[u] != n) continue;
          const int32_t* other = symH + wstart[u];
          int c = 0;
          while (c < n && other[c] == me[c]) ++c;
          if (c == n) { first = u; break; }
        }
        widx[w] = first;
      }
      __syncthreads();
      const int d = edit_distance_core(widx + Wh, Wr, widx, Wh, diag, capR + 1);
      if (threadIdx.x == 0) {
        errs[(size_t)blockIdx.y * B + b] = d;
        ref_n[(size_t)blockIdx.y * B + b] = Wr;
      }
      return;
    }
  }
  Nh = min(Nh, capH);
  Nr = min(Nr, capR);
  __syncthreads();
  int d = 0;
  if (!(mode == kModeCtcChars && Nr == 0))      // the CTC mode skips an utterance without reference characters: 0 / 0
    d = edit_distance_core(symR, Nr, symH, Nh, diag, capR + 1);
  if (threadIdx.x == 0) {
    errs[(size_t)blockIdx.y * B + b] = d;
    ref_n[(size_t)blockIdx.y * B + b] = Nr;
  }
}

// the launch plan of one error_counts call; ok == false: the shape is outside the bound stated in include/tavsr.h
struct ErrPlan {
  bool ok;
  int n_modes, capH_ctc, capH_att, capR;
  int64_t bytes;
};

static ErrPlan err_plan(int modes, int64_t B, int64_t Th, int64_t L, int64_t tok_max) {
  ErrPlan p{};
  if (modes <= 0 || modes > 7 || B < 0 || Th < 0 || L < 0 || tok_max < 1 || B > (1 << 24) || Th > (1 << 20) || L > (1 << 20) ||
      tok_max > (1 << 10))
    return p;
  const int64_t capR = L * tok_max, capH_ctc = Th * tok_max, capH_att = (Th < L ? Th : L) * tok_max;
  int64_t words = 0;
  for (int m = 0; m < 3; ++m) {
    if (!((modes >> m) & 1)) continue;
    ++p.n_modes;
    const int64_t capH = m == kModeCtcChars ? capH_ctc : capH_att;
    int64_t w = kErrHeader + kErrThreads + capH + capR + 3 * (capR + 1);
    if (m == kModeAttWords) w += 3 * ((capH + 1) / 2 + (capR + 1) / 2);
    words = w > words ? w : words;
  }
  p.bytes = words * 4;
  p.ok = p.bytes <= kErrLdsBytes;
  p.capH_ctc = (int)capH_ctc, p.capH_att = (int)capH_att, p.capR = (int)capR;
  return p;
}

}  // namespace tavsr

using namespace tavsr;

static int opt_in_lds(const void* fn, int64_t bytes, const char* what) {
  if (bytes > 48 * 1024) {      // the > 64 KB dynamic-LDS opt-in, as tavsr_ctc_align
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kErrLdsBytes);
    TAVSR_REQUIRE(e == hipSuccess, TAVSR_EUNSUPPORTED, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
  }
  return TAVSR_OK;
}

extern "C" int tavsr_edit_distance_rows(const int32_t* hyp, int64_t ldh, const int32_t* hyp_len, int32_t max_hyp, const int32_t* ref,
                                        int64_t ldr, const int32_t* ref_len, int32_t max_ref, int32_t* dist, int32_t B,
                                        tavsr_stream_t stream) {
  TAVSR_REQUIRE(B >= 0 && max_hyp >= 0 && max_ref >= 0 && ldh >= max_hyp && ldr >= max_ref, TAVSR_EINVAL,
                "edit_distance_rows: bad sizes (B=%d max_hyp=%d max_ref=%d ldh=%lld ldr=%lld)", B, max_hyp, max_ref, (long long)ldh,
                (long long)ldr);
  const int64_t bytes = 3 * ((int64_t)max_ref + 1) * 4;
  TAVSR_REQUIRE(bytes <= kErrLdsBytes, TAVSR_EUNSUPPORTED, "edit_distance_rows: reference rows of at most %d symbols (got %d)",
                kErrLdsBytes / 12 - 1, max_ref);
  if (B == 0) return TAVSR_OK;
  TAVSR_REQUIRE(hyp_len && ref_len && dist && (max_hyp == 0 || hyp) && (max_ref == 0 || ref), TAVSR_EINVAL,
                "edit_distance_rows: null pointer");
  const int rc = opt_in_lds(reinterpret_cast<const void*>(edit_distance_rows_kernel), bytes, "edit_distance_rows");
  if (rc != TAVSR_OK) return rc;
  hipLaunchKernelGGL(edit_distance_rows_kernel, dim3((unsigned)B), dim3(kErrThreads), (size_t)bytes, (hipStream_t)stream, hyp, ldh,
                     hyp_len, max_hyp, ref, ldr, ref_len, max_ref, dist);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_error_counts_ok(int32_t modes, int32_t B, int32_t Th, int32_t L, int32_t tok_max) {
  return err_plan(modes, B, Th, L, tok_max).ok ? 1 : 0;
}

extern "C" int tavsr_error_counts(const int64_t* ys_hat, int64_t ld_hat, int32_t Th, const int64_t* ys_pad, int64_t ld_pad, int32_t L,
                                  const int32_t* span, const int32_t* cps, const uint8_t* cp_space, const uint8_t* drop, int32_t V,
                                  int32_t tok_max, int32_t modes, int32_t* errs, int32_t* ref_n, int32_t B, tavsr_stream_t stream) {
  const ErrPlan p = err_plan(modes, B, Th, L, tok_max);
  TAVSR_REQUIRE(p.ok, TAVSR_EUNSUPPORTED,
                "error_counts: modes=%d B=%d Th=%d L=%d tok_max=%d is outside tavsr_error_counts_ok (LDS %lld of %d bytes)", modes, B, Th, L,
                tok_max, (long long)p.bytes, kErrLdsBytes);
  TAVSR_REQUIRE(V > 0 && ld_hat >= Th && ld_pad >= L, TAVSR_EINVAL, "error_counts: bad sizes (V=%d ld_hat=%lld ld_pad=%lld)", V,
                (long long)ld_hat, (long long)ld_pad);
  if (B == 0) return TAVSR_OK;
  TAVSR_REQUIRE(span && cps && cp_space && drop && errs && ref_n && (Th == 0 || ys_hat) && (L == 0 || ys_pad), TAVSR_EINVAL,
                "error_counts: null pointer");
  const int rc = opt_in_lds(reinterpret_cast<const void*>(error_counts_kernel), p.bytes, "error_counts");
  if (rc != TAVSR_OK) return rc;
  const ErrTables tb{span, cps, cp_space, drop, V, tok_max};
  hipLaunchKernelGGL(error_counts_kernel, dim3((unsigned)B, (unsigned)p.n_modes), dim3(kErrThreads), (size_t)p.bytes,
                     (hipStream_t)stream, ys_hat, ld_hat, Th, ys_pad, ld_pad, L, tb, modes, p.capH_ctc, p.capH_att, p.capR, errs, ref_n, B);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
