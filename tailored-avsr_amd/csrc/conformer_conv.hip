// Conformer's convolution module between its two pointwise convolutions (espnet/nets/pytorch_backend/conformer/convolution.py,
// ConvolutionModule.forward: glu(pointwise_conv1(x), dim=1) -> depthwise_conv): the GLU over the 2C channels of pointwise_conv1's
// output and the depthwise 1-D convolution over time, as one pass.
//   g[b,t,c] = h[b,t,c] * sigmoid(h[b,t,C+c])
//   z[b,t,c] = bias[c] + sum_j w[c,j] g[b,t+j-pad,c],  pad = (K-1)/2, g = 0 outside 0 <= t < T.
// The layout is dwconv_add.hip's: lanes are consecutive channels (coalesced 256-byte rows, LDS bank-conflict free), a workgroup
// stages a 64-step time tile with its halo and the taps of its 64 channels in LDS, every thread produces four consecutive time
// steps from one sliding window.  g is formed while the tile is staged (two loads, one v_exp + one v_rcp per element) and never
// reaches HBM, in either pass: the backward recomputes it from h, which it reads anyway for the GLU's derivative.  The halo stops
// at the utterance: rows t < 0 and t >= T are zeros, never the neighbouring utterance's rows of the [B*T, .] buffer.
// The kernels know no lengths: T is dense, padded frames are data like any other (espnet masks nothing here).
// dw / dbias: as in dwconv_add.hip - every thread keeps the taps k = wave, wave + 4, ... of its channel in registers over the
// block's time chunk, the block writes one partial slab [C][K+1], the slabs are summed in a fixed order: no float atomics.
// Static LDS: forward 24 KiB + 7.75 KiB; backward 2 x 24 KiB + 7.75 KiB = 55.75 of the 64 KiB a block may declare - which is
// why the backward does not also stage h's two halves for the GLU derivative: it re-reads the 4 rows it writes (cache hits:
// the tile load just read them).
#include "common.h"

namespace tavsr {

constexpr int GD_CH = 64;                    // channels per block
constexpr int GD_TB = 64;                    // time steps per tile
constexpr int GD_KMAX = 31;                  // largest kernel size
constexpr int GD_ROWS = 96;                  // LDS rows of a tile: GD_TB + GD_KMAX - 1 = 94, + 2 that the weight-gradient window touches
constexpr int GD_CHUNK = 256;                // time steps per block in the backward kernel (one partial slab per chunk)
constexpr int GD_TAPS = (GD_KMAX + 3) / 4;   // taps per thread in the weight gradient

// rows [t0 - pad, t0 - pad + rows) of utterance b, channels c0 .. c0+63, into s[i][cx]; zero outside 0 <= t < T, for channels
// >= C and for the rows up to GD_ROWS that this K does not use.  GLU: x is h [B*T][ldx] with 2C channels and the tile holds
// g = h[.., c] * sigmoid(h[.., C + c]) (zero where the row is outside the utterance: 0 * sigmoid(0)).
template <bool GLU>
__device__ __forceinline__ void gd_load_tile(float* __restrict__ s, const float* __restrict__ x, int64_t ldx, int b, int T, int t0,
                                             int pad, int rows, int C, int c, bool cok, int cx, int ty) {
  for (int ib = ty * 4; ib < GD_ROWS; ib += 16) {
    float v[4], gt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ib + q, t = t0 + i - pad;
      const bool ok = i < rows && t >= 0 && t < T && cok;
      const float* px = x + ((int64_t)b * T + t) * ldx + c;      // formed only, not read, where !ok
      v[q] = ok ? px[0] : 0.f;
      if (GLU) gt[q] = ok ? px[C] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s[(ib + q) * GD_CH + cx] = GLU ? v[q] * sigmoid_fast(gt[q]) : v[q];      // GD_ROWS % 4 == 0
  }
}

__global__ __launch_bounds__(256) void glu_dwconv_fwd_kernel(const float* __restrict__ h, int64_t ldh, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ z, int64_t ldz,
                                                             int T, int C, int K) {
  __shared__ float s_g[GD_ROWS * GD_CH];
  __shared__ float s_w[GD_KMAX * GD_CH];
  const int pad = (K - 1) / 2, rows = GD_TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * GD_CH + cx, t0 = blockIdx.y * GD_TB, b = blockIdx.z;
  const bool cok = c < C;
  gd_load_tile<true>(s_g, h, ldh, b, T, t0, pad, rows, C, c, cok, cx, ty);
  for (int k = ty; k < K; k += 4) s_w[k * GD_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  __syncthreads();
  if (!cok) return;
  const float bv = bias[c];
  const int nt = min(GD_TB, T - t0);
  for (int g = 0; g < 4; ++g) {
    const int tt = ty * 16 + g * 4;
    if (tt >= nt) break;
    const float* sg = s_g + tt * GD_CH + cx;
    float a0 = bv, a1 = bv, a2 = bv, a3 = bv;
    float x0 = sg[0], x1 = sg[GD_CH], x2 = sg[2 * GD_CH];
    for (int k = 0; k < K; ++k) {      // output tt + i reads LDS rows tt + i + k: rows <= tt + 3 + K - 1 < GD_TB + K - 1
      const float x3 = sg[(k + 3) * GD_CH], wv = s_w[k * GD_CH + cx];
      a0 = fmaf(wv, x0, a0); a1 = fmaf(wv, x1, a1); a2 = fmaf(wv, x2, a2); a3 = fmaf(wv, x3, a3);
      x0 = x1; x1 = x2; x2 = x3;
    }
    float* o = z + ((int64_t)b * T + t0 + tt) * ldz + c;
    o[0] = a0;
    if (tt + 1 < nt) o[ldz] = a1;
    if (tt + 2 < nt) o[2 * ldz] = a2;
    if (tt + 3 < nt) o[3 * ldz] = a3;
  }
}

// dg[t] = sum_k w[k] dz[t + pad - k];  dh[.., c] = dg * s,  dh[.., C + c] = dg * h[.., c] * s * (1 - s),  s = sigmoid(h[.., C + c]);
// partial sums of dw[c,k] = sum_t dz[t] g[t+k-pad] and dbias[c] = sum_t dz[t] over the block's chunk of GD_CHUNK time steps of one
// utterance -> part[(b * nchunk + chunk)][c][K+1] (tap K is the bias).
// Weight gradient: thread (channel, wave y) owns taps k = y + 4j, as dwconv_add_bwd_kernel.  The accumulators of taps k >= K are
// NOT zero and mean nothing (they multiply dz with live g rows of the tile); the `ty + 4 * j < K` guard at the end never writes
// them: do not read them.
__global__ __launch_bounds__(256) void glu_dwconv_bwd_kernel(const float* __restrict__ dz, int64_t lddz, const float* __restrict__ h,
                                                             int64_t ldh, const float* __restrict__ w, float* __restrict__ dh,
                                                             int64_t lddh, float* __restrict__ part, int T, int C, int K) {
  __shared__ float s_d[GD_ROWS * GD_CH];
  __shared__ float s_g[GD_ROWS * GD_CH];
  __shared__ float s_w[GD_KMAX * GD_CH];
  const int pad = (K - 1) / 2, rows = GD_TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * GD_CH + cx, b = blockIdx.z;
  const bool cok = c < C;
  const int tbeg = blockIdx.y * GD_CHUNK, tend = min(T, tbeg + GD_CHUNK);
  for (int k = ty; k < K; k += 4) s_w[k * GD_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  float acc[GD_TAPS], accb = 0.f;
#pragma unroll
  for (int j = 0; j < GD_TAPS; ++j) acc[j] = 0.f;
  for (int t0 = tbeg; t0 < tend; t0 += GD_TB) {
    __syncthreads();      // the previous tile is consumed (and s_w is visible)
    gd_load_tile<false>(s_d, dz, lddz, b, T, t0, pad, rows, C, c, cok, cx, ty);
    gd_load_tile<true>(s_g, h, ldh, b, T, t0, pad, rows, C, c, cok, cx, ty);
    __syncthreads();
    if (!cok) continue;
    const int nt = min(GD_TB, T - t0);
    for (int g = 0; g < 4; ++g) {
      const int tt = ty * 16 + g * 4;
      if (tt >= nt) break;
      // the rows of h this thread differentiates the GLU at (issued ahead of the tap loop; rows >= nt are not read)
      const float* ph = h + ((int64_t)b * T + t0 + tt) * ldh + c;
      float ha[4], hg[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = tt + i < nt;
        ha[i] = ok ? ph[i * ldh] : 0.f;
        hg[i] = ok ? ph[i * ldh + C] : 0.f;
      }
      const float* sd = s_d + tt * GD_CH + cx;
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      float d0 = sd[0], d1 = sd[GD_CH], d2 = sd[2 * GD_CH];
      for (int k = 0; k < K; ++k) {      // the forward's window with the taps flipped
        const float d3 = sd[(k + 3) * GD_CH], wv = s_w[(K - 1 - k) * GD_CH + cx];
        a[0] = fmaf(wv, d0, a[0]); a[1] = fmaf(wv, d1, a[1]); a[2] = fmaf(wv, d2, a[2]); a[3] = fmaf(wv, d3, a[3]);
        d0 = d1; d1 = d2; d2 = d3;
      }
      float* o = dh + ((int64_t)b * T + t0 + tt) * lddh + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (tt + i < nt) {
          const float s = sigmoid_fast(hg[i]);
          o[i * lddh] = a[i] * s;
          o[i * lddh + C] = a[i] * ha[i] * (s * (1.f - s));
        }
      }
    }
    for (int r0 = 0; r0 < nt; r0 += 16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float dv[4], xv[GD_TAPS + 3];
#pragma unroll
        for (int s = 0; s < 4; ++s) dv[s] = s_d[(r0 + r + 4 * s + pad) * GD_CH + cx];      // <= 63 + pad (rows >= nt hold zeros)
#pragma unroll
        for (int i = 0; i < GD_TAPS + 3; ++i) xv[i] = s_g[(r0 + r + ty + 4 * i) * GD_CH + cx];      // <= 48 + 3 + 3 + 40 < GD_ROWS
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < GD_TAPS; ++j) acc[j] = fmaf(dv[s], xv[s + j], acc[j]);
        if (ty == 0) accb += (dv[0] + dv[1]) + (dv[2] + dv[3]);
      }
    }
  }
  if (cok) {
    float* pw = part + (((int64_t)b * gridDim.y + blockIdx.y) * C + c) * (K + 1);
#pragma unroll
    for (int j = 0; j < GD_TAPS; ++j)
      if (ty + 4 * j < K) pw[ty + 4 * j] = acc[j];
    if (ty == 0) pw[K] = accb;
  }
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_glu_dwconv_ok(int32_t B, int32_t T, int32_t C, int32_t K) {
  return K >= 1 && K <= GD_KMAX && (K & 1) && B >= 1 && B <= 65535 && T >= 1 && C >= 1 && C < (1 << 30) &&
         (int64_t)B * T < (1ll << 31) && cdiv(T, GD_TB) <= 65535 && (int64_t)C * (K + 1) < (1ll << 31);
}

extern "C" int tavsr_glu_dwconv_fwd(const float* h, int64_t ldh, const float* w, const float* bias, float* z, int64_t ldz,
                                    int32_t B, int32_t T, int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_glu_dwconv_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "glu_dwconv_fwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", GD_KMAX, B, T, C, K);
  TAVSR_REQUIRE(h && w && bias && z, TAVSR_EINVAL, "glu_dwconv_fwd: null pointer");
  TAVSR_REQUIRE(ldh >= 2 * (int64_t)C && ldz >= C, TAVSR_EINVAL, "glu_dwconv_fwd: row strides shorter than 2C (h) / C (z)");
  hipLaunchKernelGGL(glu_dwconv_fwd_kernel, dim3(cdiv(C, GD_CH), cdiv(T, GD_TB), B), dim3(256), 0, (hipStream_t)stream, h, ldh, w,
                     bias, z, ldz, T, C, K);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int64_t tavsr_glu_dwconv_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) {
  if (!tavsr_glu_dwconv_ok(B, T, C, K)) return 0;
  return ((int64_t)B * cdiv(T, GD_CHUNK) + 1) * C * (K + 1);
}

extern "C" int tavsr_glu_dwconv_bwd(const float* dz, int64_t lddz, const float* h, int64_t ldh, const float* w, float* dh,
                                    int64_t lddh, float* dw, float* dbias, float* ws, int32_t B, int32_t T, int32_t C, int32_t K,
                                    tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_glu_dwconv_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "glu_dwconv_bwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", GD_KMAX, B, T, C, K);
  TAVSR_REQUIRE(dz && h && w && dh && dw && dbias && ws, TAVSR_EINVAL, "glu_dwconv_bwd: null pointer");
  TAVSR_REQUIRE(lddz >= C && ldh >= 2 * (int64_t)C && lddh >= 2 * (int64_t)C, TAVSR_EINVAL,
                "glu_dwconv_bwd: row strides shorter than C (dz) / 2C (h, dh)");
  const int nchunk = cdiv(T, GD_CHUNK);
  const int64_t nslab = (int64_t)B * nchunk;
  TAVSR_REQUIRE(nslab < (1ll << 31), TAVSR_EUNSUPPORTED, "glu_dwconv_bwd: too many partial slabs");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(glu_dwconv_bwd_kernel, dim3(cdiv(C, GD_CH), nchunk, B), dim3(256), 0, s, dz, lddz, h, ldh, w, dh, lddh, ws, T, C, K);
  TAVSR_LAUNCH_CHECK();
  const int n = C * (K + 1);
  float* sum = ws + nslab * n;
  int rc = tavsr_sum_partials(ws, (int32_t)nslab, n, sum, n, 0, stream);
  if (rc) return rc;
  return dwconv_split(sum, dw, dbias, C, K, 0, s);      // [C][K+1] -> dw, dbias (cgmlp.hip's, shared)
}
