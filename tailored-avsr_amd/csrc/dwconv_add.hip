// E-Branchformer's merge convolution (espnet2/asr/encoder/e_branchformer_encoder.py, EBranchformerEncoderLayer.forward:
// x_concat + depthwise_conv_fusion(x_concat)): a depthwise 1-D convolution over time on the 2D channels of the concatenated
// branch outputs, with its input added back.
//   u[b,t,c] = x[b,t,c] + bias[c] + sum_j w[c,j] x[b,t+j-pad,c],  pad = (K-1)/2, zero outside 0 <= t < T.
// HBM-bound by design: every element of x (and du) is read once per tile (+ (K-1)/64 for the halo) and every output written
// once.  Lanes are consecutive channels (coalesced 256-byte rows, LDS bank-conflict free), a workgroup stages a 64-step time
// tile with its halo and the taps of its 64 channels in LDS, and every thread produces four consecutive time steps from one
// sliding window (2 LDS reads per 4 FMAs).  The kernels know no lengths: T is dense, padded frames are data like any other.
// dw / dbias: every thread keeps the taps k = wave, wave + 4, ... of its channel in registers over the block's time chunk, the
// block writes one partial slab [C][K+1], and the slabs are summed in a fixed order (tavsr_sum_partials): no float atomics.
#include "common.h"

namespace tavsr {

constexpr int DA_CH = 64;                    // channels per block
constexpr int DA_TB = 64;                    // time steps per tile
constexpr int DA_KMAX = 31;                  // largest kernel size
constexpr int DA_ROWS = 96;                  // LDS rows of a tile: DA_TB + DA_KMAX - 1 = 94, + 2 that the weight-gradient window touches
constexpr int DA_CHUNK = 256;                // time steps per block in the backward kernel (one partial slab per chunk)
constexpr int DA_TAPS = (DA_KMAX + 3) / 4;   // taps per thread in the weight gradient

// rows [t0 - pad, t0 - pad + rows) of utterance b, channels c0 .. c0+63, into s[i][cx]; zero outside 0 <= t < T, for channels
// >= C and for the rows up to DA_ROWS that this K does not use (four loads per thread in flight)
__device__ __forceinline__ void da_load_tile(float* __restrict__ s, const float* __restrict__ x, int64_t ldx, int b, int T, int t0,
                                             int pad, int rows, int c, bool cok, int cx, int ty) {
  for (int ib = ty * 4; ib < DA_ROWS; ib += 16) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ib + q, t = t0 + i - pad;
      v[q] = (i < rows && t >= 0 && t < T && cok) ? x[((int64_t)b * T + t) * ldx + c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s[(ib + q) * DA_CH + cx] = v[q];      // DA_ROWS % 4 == 0: ib + q < DA_ROWS
  }
}

__global__ __launch_bounds__(256) void dwconv_add_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ u, int64_t ldu,
                                                             int T, int C, int K) {
  __shared__ float s_x[DA_ROWS * DA_CH];
  __shared__ float s_w[DA_KMAX * DA_CH];
  const int pad = (K - 1) / 2, rows = DA_TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * DA_CH + cx, t0 = blockIdx.y * DA_TB, b = blockIdx.z;
  const bool cok = c < C;
  da_load_tile(s_x, x, ldx, b, T, t0, pad, rows, c, cok, cx, ty);
  for (int k = ty; k < K; k += 4) s_w[k * DA_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  __syncthreads();
  if (!cok) return;
  const float bv = bias[c];
  const int nt = min(DA_TB, T - t0);
  for (int g = 0; g < 4; ++g) {
    const int tt = ty * 16 + g * 4;
    if (tt >= nt) break;
    const float* sx = s_x + tt * DA_CH + cx;
    float a0 = bv + sx[(pad + 0) * DA_CH], a1 = bv + sx[(pad + 1) * DA_CH], a2 = bv + sx[(pad + 2) * DA_CH],
          a3 = bv + sx[(pad + 3) * DA_CH];
    float x0 = sx[0], x1 = sx[DA_CH], x2 = sx[2 * DA_CH];
    for (int k = 0; k < K; ++k) {      // output tt + i reads LDS rows tt + i + k: rows <= tt + 3 + K - 1 < DA_TB + K - 1
      const float x3 = sx[(k + 3) * DA_CH], wv = s_w[k * DA_CH + cx];
      a0 = fmaf(wv, x0, a0); a1 = fmaf(wv, x1, a1); a2 = fmaf(wv, x2, a2); a3 = fmaf(wv, x3, a3);
      x0 = x1; x1 = x2; x2 = x3;
    }
    float* o = u + ((int64_t)b * T + t0 + tt) * ldu + c;
    o[0] = a0;
    if (tt + 1 < nt) o[ldu] = a1;
    if (tt + 2 < nt) o[2 * ldu] = a2;
    if (tt + 3 < nt) o[3 * ldu] = a3;
  }
}

// dx[t] = du[t] + sum_k w[k] du[t + pad - k];  partial sums of dw[c,k] = sum_t du[t] x[t+k-pad] and dbias[c] = sum_t du[t] over the
// block's chunk of DA_CHUNK time steps of one utterance -> part[(b * nchunk + chunk)][c][K+1] (tap K is the bias).
// Weight gradient: thread (channel, wave y) owns taps k = y + 4j.  Rows r, r+4, r+8, r+12 of a 16-row group need the x rows
// r + y + 4(s + j), s + j = 0..10: 11 + 4 LDS reads for 32 FMAs.  The accumulators of taps k >= K are NOT zero and mean nothing:
// for K < 31 they multiply du with live x rows of the tile (row r + k < 64 + K - 1), beyond those with the zero fill.  They are
// harmless only because the `ty + 4 * j < K` guard at the end never writes them: do not read them.
__global__ __launch_bounds__(256) void dwconv_add_bwd_kernel(const float* __restrict__ du, int64_t lddu, const float* __restrict__ x,
                                                             int64_t ldx, const float* __restrict__ w, float* __restrict__ dx,
                                                             int64_t lddx, float* __restrict__ part, int T, int C, int K) {
  __shared__ float s_d[DA_ROWS * DA_CH];
  __shared__ float s_x[DA_ROWS * DA_CH];
  __shared__ float s_w[DA_KMAX * DA_CH];
  const int pad = (K - 1) / 2, rows = DA_TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * DA_CH + cx, b = blockIdx.z;
  const bool cok = c < C;
  const int tbeg = blockIdx.y * DA_CHUNK, tend = min(T, tbeg + DA_CHUNK);
  for (int k = ty; k < K; k += 4) s_w[k * DA_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  float acc[DA_TAPS], accb = 0.f;
#pragma unroll
  for (int j = 0; j < DA_TAPS; ++j) acc[j] = 0.f;
  for (int t0 = tbeg; t0 < tend; t0 += DA_TB) {
    __syncthreads();      // the previous tile is consumed (and s_w is visible)
    da_load_tile(s_d, du, lddu, b, T, t0, pad, rows, c, cok, cx, ty);
    da_load_tile(s_x, x, ldx, b, T, t0, pad, rows, c, cok, cx, ty);
    __syncthreads();
    if (!cok) continue;
    const int nt = min(DA_TB, T - t0);
    for (int g = 0; g < 4; ++g) {
      const int tt = ty * 16 + g * 4;
      if (tt >= nt) break;
      const float* sd = s_d + tt * DA_CH + cx;
      float a0 = sd[(pad + 0) * DA_CH], a1 = sd[(pad + 1) * DA_CH], a2 = sd[(pad + 2) * DA_CH], a3 = sd[(pad + 3) * DA_CH];
      float d0 = sd[0], d1 = sd[DA_CH], d2 = sd[2 * DA_CH];
      for (int k = 0; k < K; ++k) {      // the forward's window with the taps flipped
        const float d3 = sd[(k + 3) * DA_CH], wv = s_w[(K - 1 - k) * DA_CH + cx];
        a0 = fmaf(wv, d0, a0); a1 = fmaf(wv, d1, a1); a2 = fmaf(wv, d2, a2); a3 = fmaf(wv, d3, a3);
        d0 = d1; d1 = d2; d2 = d3;
      }
      float* o = dx + ((int64_t)b * T + t0 + tt) * lddx + c;
      o[0] = a0;
      if (tt + 1 < nt) o[lddx] = a1;
      if (tt + 2 < nt) o[2 * lddx] = a2;
      if (tt + 3 < nt) o[3 * lddx] = a3;
    }
    for (int r0 = 0; r0 < nt; r0 += 16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float dv[4], xv[DA_TAPS + 3];
#pragma unroll
        for (int s = 0; s < 4; ++s) dv[s] = s_d[(r0 + r + 4 * s + pad) * DA_CH + cx];      // <= 63 + pad (rows >= nt hold zeros)
#pragma unroll
        for (int i = 0; i < DA_TAPS + 3; ++i) xv[i] = s_x[(r0 + r + ty + 4 * i) * DA_CH + cx];      // <= 48 + 3 + 3 + 40 < DA_ROWS
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < DA_TAPS; ++j) acc[j] = fmaf(dv[s], xv[s + j], acc[j]);
        if (ty == 0) accb += (dv[0] + dv[1]) + (dv[2] + dv[3]);
      }
    }
  }
  if (cok) {
    float* pw = part + (((int64_t)b * gridDim.y + blockIdx.y) * C + c) * (K + 1);
#pragma unroll
    for (int j = 0; j < DA_TAPS; ++j)
      if (ty + 4 * j < K) pw[ty + 4 * j] = acc[j];
    if (ty == 0) pw[K] = accb;
  }
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_dwconv_add_ok(int32_t B, int32_t T, int32_t C, int32_t K) {
  return K >= 1 && K <= DA_KMAX && (K & 1) && B >= 1 && B <= 65535 && T >= 1 && C >= 1 && (int64_t)B * T < (1ll << 31) &&
         cdiv(T, DA_TB) <= 65535 && (int64_t)C * (K + 1) < (1ll << 31);
}

extern "C" int tavsr_dwconv_add_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* u, int64_t ldu,
                                    int32_t B, int32_t T, int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_dwconv_add_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_add_fwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", DA_KMAX, B, T, C, K);
  TAVSR_REQUIRE(x && w && bias && u, TAVSR_EINVAL, "dwconv_add_fwd: null pointer");
  TAVSR_REQUIRE(ldx >= C && ldu >= C, TAVSR_EINVAL, "dwconv_add_fwd: row strides shorter than C");
  hipLaunchKernelGGL(dwconv_add_fwd_kernel, dim3(cdiv(C, DA_CH), cdiv(T, DA_TB), B), dim3(256), 0, (hipStream_t)stream, x, ldx, w,
                     bias, u, ldu, T, C, K);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int64_t tavsr_dwconv_add_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) {
  if (!tavsr_dwconv_add_ok(B, T, C, K)) return 0;
  return ((int64_t)B * cdiv(T, DA_CHUNK) + 1) * C * (K + 1);
}

extern "C" int tavsr_dwconv_add_bwd(const float* du, int64_t lddu, const float* x, int64_t ldx, const float* w, float* dx,
                                    int64_t lddx, float* dw, float* dbias, int32_t accumulate, float* ws, int32_t B, int32_t T,
                                    int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_dwconv_add_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_add_bwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", DA_KMAX, B, T, C, K);
  TAVSR_REQUIRE(du && x && w && dx && dw && dbias && ws, TAVSR_EINVAL, "dwconv_add_bwd: null pointer");
  TAVSR_REQUIRE(lddu >= C && ldx >= C && lddx >= C, TAVSR_EINVAL, "dwconv_add_bwd: row strides shorter than C");
  const int nchunk = cdiv(T, DA_CHUNK);
  const int64_t nslab = (int64_t)B * nchunk;
  TAVSR_REQUIRE(nslab < (1ll << 31), TAVSR_EUNSUPPORTED, "dwconv_add_bwd: too many partial slabs");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dwconv_add_bwd_kernel, dim3(cdiv(C, DA_CH), nchunk, B), dim3(256), 0, s, du, lddu, x, ldx, w, dx, lddx, ws, T, C, K);
  TAVSR_LAUNCH_CHECK();
  const int n = C * (K + 1);
  float* sum = ws + nslab * n;
  int rc = tavsr_sum_partials(ws, (int32_t)nslab, n, sum, n, 0, stream);
  if (rc) return rc;
  return dwconv_split(sum, dw, dbias, C, K, accumulate, s);      // [C][K+1] -> dw, dbias (cgmlp.hip's, shared)
}
