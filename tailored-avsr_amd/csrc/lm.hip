// Language-model training rows (espnet2 lm/espnet_model.py ESPnetLanguageModel.nll: x = pad(text, [1, 0], eos), t = pad(text, [0, 1],
// ignore_id), `for i, l in enumerate(text_lengths): t[i, l] = sos`, x_lengths = text_lengths + 1):
//   lm_shift    : the shifted input / target pair of a batch built on the device, rows delimited by `lengths` (never by a pad value)
//   lm_row_sums : per-sentence sums of the token nll rows (the numerator of a sentence's perplexity)
// Integer outputs, every output element written exactly once, no host value read: one launch each, capturable.
#include "common.h"

namespace tavsr {

// one workgroup per sentence; len is clamped to [0, min(W, Wout - 1)] so that no index leaves text[b][0:W] or the output rows
__global__ __launch_bounds__(256) void lm_shift_kernel(const int64_t* __restrict__ text, int64_t ld_text, int W,
                                                       const int64_t* __restrict__ lengths, int sos_eos,
                                                       int64_t* __restrict__ x, int64_t* __restrict__ t, int64_t ld_y, int Wout,
                                                       int64_t* __restrict__ x_lengths, int32_t* __restrict__ n) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cap = min(W, Wout - 1);
  const int64_t l64 = lengths[b];
  const int len = l64 < 0 ? 0 : l64 > (int64_t)cap ? cap : (int)l64;
  const int64_t* row = text + (int64_t)b * ld_text;
  int64_t* xr = x + (int64_t)b * ld_y;
  int64_t* tr = t + (int64_t)b * ld_y;
  for (int j = tid; j < Wout; j += 256) {
    xr[j] = j == 0 ? (int64_t)sos_eos : j <= len ? row[j - 1] : (int64_t)0;
    tr[j] = j < len ? row[j] : j == len ? (int64_t)sos_eos : (int64_t)-1;
  }
  if (tid == 0) {
    x_lengths[b] = (int64_t)len + 1;
    n[b] = len + 1;
  }
}

// out[r] = sum_c x[r][c]: one wave per row, lane-strided partial sums and a butterfly (a fixed order: same bits every run)
__global__ __launch_bounds__(256) void lm_row_sums_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                          int rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;      // (whole waves leave: the shuffles below run with all 64 lanes of the wave)
  const float* row = x + (int64_t)r * ldx;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += row[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) out[r] = s;
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_lm_shift(const int64_t* text, int64_t ld_text, const int64_t* lengths, int32_t B, int32_t W, int32_t sos_eos,
                              int64_t* x, int64_t* t, int64_t ld_y, int32_t Wout, int64_t* x_lengths, int32_t* n,
                              tavsr_stream_t stream) {
  TAVSR_REQUIRE(W >= 0 && Wout >= 1 && ld_text >= W && ld_y >= Wout, TAVSR_EINVAL,
                "lm_shift: ld_text >= W >= 0 and ld_y >= Wout >= 1 required");
  TAVSR_REQUIRE(sos_eos >= 0, TAVSR_EINVAL, "lm_shift: sos / eos id < 0");
  TAVSR_REQUIRE(B <= 0 || (lengths && x && t && x_lengths && n && (text || W == 0)), TAVSR_EINVAL, "lm_shift: null pointer");
  if (B <= 0) return TAVSR_OK;
  hipLaunchKernelGGL(lm_shift_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, text, ld_text, W, lengths, sos_eos, x, t, ld_y,
                     Wout, x_lengths, n);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_lm_row_sums(const float* x, int64_t ldx, float* out, int32_t rows, int32_t cols, tavsr_stream_t stream) {
  TAVSR_REQUIRE(cols >= 0 && ldx >= cols, TAVSR_EINVAL, "lm_row_sums: ldx >= cols >= 0 required");
  TAVSR_REQUIRE(rows <= 0 || (out && (x || cols == 0)), TAVSR_EINVAL, "lm_row_sums: null pointer");
  if (rows <= 0) return TAVSR_OK;
  hipLaunchKernelGGL(lm_row_sums_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, out, rows, cols);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
