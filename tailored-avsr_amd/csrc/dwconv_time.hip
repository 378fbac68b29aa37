// Depthwise 1-D convolutions over time, pad = (K-1)/2, zero outside 0 <= t < T of the block's own utterance, in three forms:
//   add:  E-Branchformer's merge convolution (espnet2/asr/encoder/e_branchformer_encoder.py, EBranchformerEncoderLayer.forward:
//         x_concat + depthwise_conv_fusion(x_concat)), its input added back:
//           u[b,t,c] = x[b,t,c] + bias[c] + sum_j w[c,j] x[b,t+j-pad,c]
//   GLU:  Conformer's convolution module between its two pointwise convolutions (espnet/nets/pytorch_backend/conformer/
//         convolution.py, ConvolutionModule.forward: glu(pointwise_conv1(x), dim=1) -> depthwise_conv), as one pass over the 2C
//         channels of pointwise_conv1's output h:
//           g[b,t,c] = h[b,t,c] * sigmoid(h[b,t,C+c]),   z[b,t,c] = bias[c] + sum_j w[c,j] g[b,t+j-pad,c]
//   gate: cgMLP's spatial gating unit after its LayerNorm (espnet2/asr/layers/cgmlp.py, ConvolutionalSpatialGatingUnit.forward:
//         x_r * conv(norm(x_g))) at every kernel size but the recipe's 31, which cgmlp.hip keeps in kernels of its own:
//           conv[b,t,c] = bias[c] + sum_j w[c,j] gn[b,t+j-pad,c],   out[b,t,c] = r[b,t,c] * conv[b,t,c]
// HBM-bound by design: every input element is read once per tile (+ (K-1)/64 for the halo) and every output written once.  Lanes
// are consecutive channels (coalesced 256-byte rows, LDS bank-conflict free), a workgroup stages a time tile with its halo (64
// steps; the gate form, which takes K up to 63, 32 steps in the same 96 LDS rows) and the taps of its 64 channels in LDS, and
// every thread produces four consecutive time steps from one sliding window (K + 3 LDS reads per 4 K FMAs).  The halo stops at
// the utterance: rows t < 0 and t >= T are zeros, never the neighbouring utterance's rows of the [B*T, .] buffer.  The kernels
// know no lengths: T is dense, padded frames are data like any other.
// g is formed while the tile is staged (two loads, one v_exp + one v_rcp per element) and never reaches HBM, in either pass: the
// backward recomputes it from h, which it reads anyway for the GLU's derivative.  The gate's backward forms dconv = du * r the
// same way.
// dw / dbias: every thread keeps the taps k = wave, wave + 4, ... of its channel in registers over the block's time chunk, the
// block writes one partial slab [C][K+1], and the slabs are summed in a fixed order (tavsr_sum_partials): no float atomics.
// Static LDS, add and GLU: forward 24 KiB + 7.75 KiB; backward 2 x 24 KiB + 7.75 KiB = 55.75 of the 64 KiB a block may declare -
// which is why the GLU backward does not also stage h's two halves for the GLU derivative: it re-reads the 4 rows it writes
// (cache hits: the tile load just read them), as the gate backward re-reads du and conv for dr.  Gate: 15.75 KiB of taps, 39.75
// KiB forward, 63.75 KiB backward.
// The forms differ only where the code names one: the tile geometry, how a tile element is formed, how the sums start (the add
// form adds its input back: x[t] forward, du[t] backward), and what becomes of the four sums.  No other combination (GLU with
// the add, plain without) has a caller or an instance.
#include "common.h"

namespace tavsr {

// the form F of a kernel.  As dt_load_tile's argument: how a tile element is formed - a plain load, the GLU of two columns, or the
// gate backward's product of two arrays
enum { DT_ADD, DT_GLU, DT_GATE };
constexpr int DT_CH = 64;                    // channels per block
constexpr int DT_ROWS = 96;                  // LDS rows of a tile: time steps + largest halo + 2 that the weight-gradient window touches
constexpr int DT_CHUNK = 256;                // time steps per block in the backward kernel (one partial slab per chunk)
constexpr int dt_kmax(int F) { return F == DT_GATE ? 63 : 31; }      // largest kernel size
constexpr int dt_tb(int F) { return F == DT_GATE ? 32 : 64; }        // time steps per tile: 64 + 30 + 2 = 32 + 62 + 2 = DT_ROWS
constexpr int dt_taps(int F) { return (dt_kmax(F) + 3) / 4; }        // taps per thread in the weight gradient: 8, 16
// the gate backward's two tiles and 63 x 64 taps are 65,280 bytes: 256 under the 64 KiB a block may declare
static_assert((2 * DT_ROWS + dt_kmax(DT_GATE)) * DT_CH * sizeof(float) <= 65536, "static LDS of the gate backward");
static_assert(dt_tb(DT_ADD) + dt_kmax(DT_ADD) + 1 == DT_ROWS && dt_tb(DT_GATE) + dt_kmax(DT_GATE) + 1 == DT_ROWS, "tile rows");

// rows [t0 - pad, t0 - pad + rows) of utterance b, channels c0 .. c0+63, into s[i][cx]; zero outside 0 <= t < T, for channels
// >= C and for the rows up to DT_ROWS that this K does not use (four loads per thread in flight).  GLU: x is h [B*T][ldx] with
// 2C channels and the tile holds g = h[.., c] * sigmoid(h[.., C + c]) (zero where the row is outside the utterance: 0 * sigmoid(0)).
// Gate: the tile holds the product x * y of two arrays, each with its own row stride.  y is not read otherwise.
template <int F>
__device__ __forceinline__ void dt_load_tile(float* __restrict__ s, const float* __restrict__ x, int64_t ldx, int b, int T, int t0,
                                             int pad, int rows, int C, int c, bool cok, int cx, int ty,
                                             const float* __restrict__ y = nullptr, int64_t ldy = 0) {
  for (int ib = ty * 4; ib < DT_ROWS; ib += 16) {
    float v[4], gt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ib + q, t = t0 + i - pad;
      const bool ok = i < rows && t >= 0 && t < T && cok;
      const float* px = x + ((int64_t)b * T + t) * ldx + c;      // formed only, not read, where !ok
      v[q] = ok ? px[0] : 0.f;
      if (F == DT_GLU) gt[q] = ok ? px[C] : 0.f;
      if (F == DT_GATE) gt[q] = ok ? y[((int64_t)b * T + t) * ldy + c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)      // DT_ROWS % 4 == 0
      s[(ib + q) * DT_CH + cx] = F == DT_GLU ? v[q] * sigmoid_fast(gt[q]) : F == DT_GATE ? v[q] * gt[q] : v[q];
  }
}

// add: u = x + bias + conv(x).  GLU: z = bias + conv(glu(x)), x = h with 2C channels.  Gate: u = r * (bias + conv(x)), x = gn, the
// convolution itself also stored to conv [B*T][C] unless that is null.  r and conv are the gate's alone.
template <int F>
__global__ __launch_bounds__(256) void dwconv_time_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ u, int64_t ldu,
                                                              int T, int C, int K, const float* __restrict__ r, int64_t ldr,
                                                              float* __restrict__ conv) {
  constexpr int TB = dt_tb(F);
  __shared__ float s_x[DT_ROWS * DT_CH];
  __shared__ float s_w[dt_kmax(F) * DT_CH];
  const int pad = (K - 1) / 2, rows = TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * DT_CH + cx, t0 = blockIdx.y * TB, b = blockIdx.z;
  const bool cok = c < C;
  dt_load_tile<F == DT_GLU ? DT_GLU : DT_ADD>(s_x, x, ldx, b, T, t0, pad, rows, C, c, cok, cx, ty);
  for (int k = ty; k < K; k += 4) s_w[k * DT_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  __syncthreads();
  if (!cok) return;
  const float bv = bias[c];
  const int nt = min(TB, T - t0);
  for (int g = 0; g < TB / 16; ++g) {      // a wave owns TB / 4 consecutive rows, four at a time
    const int tt = ty * (TB / 4) + g * 4;
    if (tt >= nt) break;
    float rv[4];
    if (F == DT_GATE) {      // issued ahead of the tap loop; rows >= nt are not read
#pragma unroll
      for (int i = 0; i < 4; ++i) rv[i] = tt + i < nt ? r[((int64_t)b * T + t0 + tt + i) * ldr + c] : 0.f;
    }
    const float* sx = s_x + tt * DT_CH + cx;
    float a0 = bv, a1 = bv, a2 = bv, a3 = bv;
    if (F == DT_ADD) {      // the input added back
      a0 += sx[(pad + 0) * DT_CH]; a1 += sx[(pad + 1) * DT_CH]; a2 += sx[(pad + 2) * DT_CH]; a3 += sx[(pad + 3) * DT_CH];
    }
    float x0 = sx[0], x1 = sx[DT_CH], x2 = sx[2 * DT_CH];
    for (int k = 0; k < K; ++k) {      // output tt + i reads LDS rows tt + i + k: rows <= tt + 3 + K - 1 < TB + K - 1
      const float x3 = sx[(k + 3) * DT_CH], wv = s_w[k * DT_CH + cx];
      a0 = fmaf(wv, x0, a0); a1 = fmaf(wv, x1, a1); a2 = fmaf(wv, x2, a2); a3 = fmaf(wv, x3, a3);
      x0 = x1; x1 = x2; x2 = x3;
    }
    if (F == DT_GATE) {
      if (conv) {
        float* pc = conv + ((int64_t)b * T + t0 + tt) * C + c;
        pc[0] = a0;
        if (tt + 1 < nt) pc[C] = a1;
        if (tt + 2 < nt) pc[2 * (int64_t)C] = a2;
        if (tt + 3 < nt) pc[3 * (int64_t)C] = a3;
      }
      a0 *= rv[0]; a1 *= rv[1]; a2 *= rv[2]; a3 *= rv[3];
    }
    float* o = u + ((int64_t)b * T + t0 + tt) * ldu + c;
    o[0] = a0;
    if (tt + 1 < nt) o[ldu] = a1;
    if (tt + 2 < nt) o[2 * ldu] = a2;
    if (tt + 3 < nt) o[3 * ldu] = a3;
  }
}

// add: dx[t] = d[t] + sum_k w[k] d[t + pad - k], d = du.
// GLU: dg[t] = sum_k w[k] d[t + pad - k], d = dz;  dx = dh with 2C channels: dh[.., c] = dg * s,  dh[.., C + c] = dg * h[.., c] * s *
//      (1 - s),  s = sigmoid(h[.., C + c]), x = h.
// gate: dgn[t] = sum_k w[k] d[t + pad - k], d = du * r formed as the tile is staged, x = gn, dx = dgn;  dr = du * conv beside it
//      (r, conv and dr are the gate's alone).
// Partial sums of dw[c,k] = sum_t d[t] xg[t+k-pad] (xg: the staged x or g) and dbias[c] = sum_t d[t] over the block's chunk of
// DT_CHUNK time steps of one utterance -> part[(b * nchunk + chunk)][c][K+1] (tap K is the bias).
// Weight gradient: thread (channel, wave y) owns taps k = y + 4j.  Rows r, r+4, r+8, r+12 of a 16-row group need the xg rows
// r + y + 4(s + j), s + j = 0..10 (gate: 0..18): 11 + 4 LDS reads for 32 FMAs (19 + 4 for 64).  The accumulators of taps k >= K
// are NOT zero and mean nothing: for K below the largest they multiply d with live xg rows of the tile (row r + k < TB + K - 1),
// beyond those with the zero fill.  They are harmless only because the `ty + 4 * j < K` guard at the end never writes them: do
// not read them.
template <int F>
__global__ __launch_bounds__(256) void dwconv_time_bwd_kernel(const float* __restrict__ d, int64_t ldd, const float* __restrict__ x,
                                                              int64_t ldx, const float* __restrict__ w, float* __restrict__ dx,
                                                              int64_t lddx, float* __restrict__ part, int T, int C, int K,
                                                              const float* __restrict__ r, int64_t ldr,
                                                              const float* __restrict__ conv, float* __restrict__ dr, int64_t lddr) {
  constexpr int TB = dt_tb(F), TAPS = dt_taps(F);
  __shared__ float s_d[DT_ROWS * DT_CH];
  __shared__ float s_x[DT_ROWS * DT_CH];
  __shared__ float s_w[dt_kmax(F) * DT_CH];
  const int pad = (K - 1) / 2, rows = TB + K - 1;
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * DT_CH + cx, b = blockIdx.z;
  const bool cok = c < C;
  const int tbeg = blockIdx.y * DT_CHUNK, tend = min(T, tbeg + DT_CHUNK);
  for (int k = ty; k < K; k += 4) s_w[k * DT_CH + cx] = cok ? w[(int64_t)c * K + k] : 0.f;
  float acc[TAPS], accb = 0.f;
#pragma unroll
  for (int j = 0; j < TAPS; ++j) acc[j] = 0.f;
  for (int t0 = tbeg; t0 < tend; t0 += TB) {
    __syncthreads();      // the previous tile is consumed (and s_w is visible)
    dt_load_tile<F == DT_GATE ? DT_GATE : DT_ADD>(s_d, d, ldd, b, T, t0, pad, rows, C, c, cok, cx, ty, r, ldr);
    dt_load_tile<F == DT_GLU ? DT_GLU : DT_ADD>(s_x, x, ldx, b, T, t0, pad, rows, C, c, cok, cx, ty);
    __syncthreads();
    if (!cok) continue;
    const int nt = min(TB, T - t0);
    for (int g = 0; g < TB / 16; ++g) {
      const int tt = ty * (TB / 4) + g * 4;
      if (tt >= nt) break;
      // GLU: the rows of h this thread differentiates the GLU at (issued ahead of the tap loop; rows >= nt are not read)
      float ha[4], hg[4];
      if (F == DT_GLU) {
        const float* ph = x + ((int64_t)b * T + t0 + tt) * ldx + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = tt + i < nt;
          ha[i] = ok ? ph[i * ldx] : 0.f;
          hg[i] = ok ? ph[i * ldx + C] : 0.f;
        }
      }
      if (F == DT_GATE) {      // likewise the rows of du and conv that dr is the product of
        const int64_t m = (int64_t)b * T + t0 + tt;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = tt + i < nt;
          ha[i] = ok ? d[(m + i) * ldd + c] : 0.f;
          hg[i] = ok ? conv[(m + i) * C + c] : 0.f;
        }
      }
      const float* sd = s_d + tt * DT_CH + cx;
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = F == DT_ADD ? sd[(pad + i) * DT_CH] : 0.f;
      float d0 = sd[0], d1 = sd[DT_CH], d2 = sd[2 * DT_CH];
      for (int k = 0; k < K; ++k) {      // the forward's window with the taps flipped
        const float d3 = sd[(k + 3) * DT_CH], wv = s_w[(K - 1 - k) * DT_CH + cx];
        a[0] = fmaf(wv, d0, a[0]); a[1] = fmaf(wv, d1, a[1]); a[2] = fmaf(wv, d2, a[2]); a[3] = fmaf(wv, d3, a[3]);
        d0 = d1; d1 = d2; d2 = d3;
      }
      float* o = dx + ((int64_t)b * T + t0 + tt) * lddx + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (tt + i < nt) {
          if (F == DT_GLU) {
            const float s = sigmoid_fast(hg[i]);
            o[i * lddx] = a[i] * s;
            o[i * lddx + C] = a[i] * ha[i] * (s * (1.f - s));
          } else {
            o[i * lddx] = a[i];
            if (F == DT_GATE) dr[((int64_t)b * T + t0 + tt + i) * lddr + c] = ha[i] * hg[i];
          }
        }
      }
    }
    for (int r0 = 0; r0 < nt; r0 += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float dv[4], xv[TAPS + 3];
#pragma unroll
        for (int s = 0; s < 4; ++s) dv[s] = s_d[(r0 + q + 4 * s + pad) * DT_CH + cx];      // <= TB - 1 + pad (rows >= nt hold zeros)
#pragma unroll
        for (int i = 0; i < TAPS + 3; ++i)      // <= 48 + 3 + 3 + 40 = 16 + 3 + 3 + 72 < DT_ROWS
          xv[i] = s_x[(r0 + q + ty + 4 * i) * DT_CH + cx];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < TAPS; ++j) acc[j] = fmaf(dv[s], xv[s + j], acc[j]);
        if (ty == 0) accb += (dv[0] + dv[1]) + (dv[2] + dv[3]);
      }
    }
  }
  if (cok) {
    float* pw = part + (((int64_t)b * gridDim.y + blockIdx.y) * C + c) * (K + 1);
#pragma unroll
    for (int j = 0; j < TAPS; ++j)
      if (ty + 4 * j < K) pw[ty + 4 * j] = acc[j];
    if (ty == 0) pw[K] = accb;
  }
}

// split [C][K+1] summed slab into dw[C][K] and dbias[C]
__global__ void dwconv_split_kernel(const float* __restrict__ sum, float* __restrict__ dw, float* __restrict__ db, int C,
                                    int K, int accumulate) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * (K + 1)) return;
  int c = i / (K + 1), k = i % (K + 1);
  float v = sum[i];
  if (k < K) dw[c * K + k] = accumulate ? dw[c * K + k] + v : v;
  else db[c] = accumulate ? db[c] + v : v;
}

int dwconv_split(const float* sum, float* dw, float* dbias, int C, int K, int accumulate, hipStream_t stream) {
  const int n = C * (K + 1);
  hipLaunchKernelGGL(dwconv_split_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, sum, dw, dbias, C, K, accumulate);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

// what every form refuses: the static LDS arrays (K), the grid (B, time tiles), 32-bit row and slab indices
static bool dt_ok(int F, int32_t B, int32_t T, int32_t C, int32_t K) {
  return K >= 1 && K <= dt_kmax(F) && (K & 1) && B >= 1 && B <= 65535 && T >= 1 && C >= 1 && (int64_t)B * T < (1ll << 31) &&
         cdiv(T, dt_tb(F)) <= 65535 && (int64_t)C * (K + 1) < (1ll << 31);
}

// floats of workspace: one slab [C][K+1] per (utterance, chunk) and one for their sum
int64_t dt_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) { return ((int64_t)B * cdiv(T, DT_CHUNK) + 1) * C * (K + 1); }

// one block per 64 channels x time tile x utterance; r, ldr and conv: the gate's
template <int F>
static int dt_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* u, int64_t ldu, int B, int T, int C, int K,
                  tavsr_stream_t stream, const float* r = nullptr, int64_t ldr = 0, float* conv = nullptr) {
  hipLaunchKernelGGL(dwconv_time_fwd_kernel<F>, dim3(cdiv(C, DT_CH), cdiv(T, dt_tb(F)), B), dim3(256), 0, (hipStream_t)stream, x, ldx,
                     w, bias, u, ldu, T, C, K, r, ldr, conv);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

// launch the backward kernel, sum its slabs in a fixed order, split the sum [C][K+1] into dw and dbias; r .. lddr: the gate's
template <int F>
static int dt_bwd(const char* name, const float* d, int64_t ldd, const float* x, int64_t ldx, const float* w, float* dx, int64_t lddx,
                  float* dw, float* dbias, int accumulate, float* ws, int B, int T, int C, int K, tavsr_stream_t stream,
                  const float* r = nullptr, int64_t ldr = 0, const float* conv = nullptr, float* dr = nullptr, int64_t lddr = 0) {
  const int nchunk = cdiv(T, DT_CHUNK);
  const int64_t nslab = (int64_t)B * nchunk;
  TAVSR_REQUIRE(nslab < (1ll << 31), TAVSR_EUNSUPPORTED, "%s: too many partial slabs", name);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dwconv_time_bwd_kernel<F>, dim3(cdiv(C, DT_CH), nchunk, B), dim3(256), 0, s, d, ldd, x, ldx, w, dx, lddx, ws,
                     T, C, K, r, ldr, conv, dr, lddr);
  TAVSR_LAUNCH_CHECK();
  const int n = C * (K + 1);
  float* sum = ws + nslab * n;
  int rc = tavsr_sum_partials(ws, (int32_t)nslab, n, sum, n, 0, stream);
  if (rc) return rc;
  return dwconv_split(sum, dw, dbias, C, K, accumulate, s);
}

// the gate form for tavsr_dwconv_gate_fwd / _bwd (cgmlp.hip), which have checked the pointers; gn, out, conv, du and dgn are dense
// [B*T][C].  An empty shape at a kernel size the form takes is nothing to do, not a refusal.
static bool dt_gate_empty(int B, int T, int C, int K) {
  return K >= 1 && K <= dt_kmax(DT_GATE) && (K & 1) && (B <= 0 || T <= 0 || C <= 0);
}

int dt_gate_fwd(const float* gn, const float* r, int64_t ldr, const float* w, const float* bias, float* out, float* conv, int B, int T,
                int C, int K, tavsr_stream_t stream) {
  if (dt_gate_empty(B, T, C, K)) return TAVSR_OK;
  TAVSR_REQUIRE(dt_ok(DT_GATE, B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_gate_fwd: odd kernel size <= %d and a shape within the index limits required (got B %d, T %d, C %d, K %d)",
                dt_kmax(DT_GATE), B, T, C, K);
  return dt_fwd<DT_GATE>(gn, C, w, bias, out, C, B, T, C, K, stream, r, ldr, conv);
}

int dt_gate_bwd(const float* du, const float* gn, const float* r, int64_t ldr, const float* conv, const float* w, float* dr,
                int64_t lddr, float* dgn, float* dw, float* dbias, int accumulate, float* ws, int B, int T, int C, int K,
                tavsr_stream_t stream) {
  if (dt_gate_empty(B, T, C, K)) return TAVSR_OK;
  TAVSR_REQUIRE(dt_ok(DT_GATE, B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_gate_bwd: odd kernel size <= %d and a shape within the index limits required (got B %d, T %d, C %d, K %d)",
                dt_kmax(DT_GATE), B, T, C, K);
  return dt_bwd<DT_GATE>("dwconv_gate_bwd", du, C, gn, C, w, dgn, C, dw, dbias, accumulate, ws, B, T, C, K, stream, r, ldr, conv, dr,
                         lddr);
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_dwconv_add_ok(int32_t B, int32_t T, int32_t C, int32_t K) { return dt_ok(DT_ADD, B, T, C, K); }

extern "C" int tavsr_dwconv_add_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* u, int64_t ldu,
                                    int32_t B, int32_t T, int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_dwconv_add_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_add_fwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", dt_kmax(DT_ADD), B, T, C, K);
  TAVSR_REQUIRE(x && w && bias && u, TAVSR_EINVAL, "dwconv_add_fwd: null pointer");
  TAVSR_REQUIRE(ldx >= C && ldu >= C, TAVSR_EINVAL, "dwconv_add_fwd: row strides shorter than C");
  return dt_fwd<DT_ADD>(x, ldx, w, bias, u, ldu, B, T, C, K, stream);
}

extern "C" int64_t tavsr_dwconv_add_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) {
  return tavsr_dwconv_add_ok(B, T, C, K) ? dt_bwd_ws(B, T, C, K) : 0;
}

extern "C" int tavsr_dwconv_add_bwd(const float* du, int64_t lddu, const float* x, int64_t ldx, const float* w, float* dx,
                                    int64_t lddx, float* dw, float* dbias, int32_t accumulate, float* ws, int32_t B, int32_t T,
                                    int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_dwconv_add_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "dwconv_add_bwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", dt_kmax(DT_ADD), B, T, C, K);
  TAVSR_REQUIRE(du && x && w && dx && dw && dbias && ws, TAVSR_EINVAL, "dwconv_add_bwd: null pointer");
  TAVSR_REQUIRE(lddu >= C && ldx >= C && lddx >= C, TAVSR_EINVAL, "dwconv_add_bwd: row strides shorter than C");
  return dt_bwd<DT_ADD>("dwconv_add_bwd", du, lddu, x, ldx, w, dx, lddx, dw, dbias, accumulate, ws, B, T, C, K, stream);
}

// the GLU form also indexes column C + c of a row: C < 2^30
extern "C" int tavsr_glu_dwconv_ok(int32_t B, int32_t T, int32_t C, int32_t K) { return dt_ok(DT_GLU, B, T, C, K) && C < (1 << 30); }

extern "C" int tavsr_glu_dwconv_fwd(const float* h, int64_t ldh, const float* w, const float* bias, float* z, int64_t ldz,
                                    int32_t B, int32_t T, int32_t C, int32_t K, tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_glu_dwconv_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "glu_dwconv_fwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", dt_kmax(DT_GLU), B, T, C, K);
  TAVSR_REQUIRE(h && w && bias && z, TAVSR_EINVAL, "glu_dwconv_fwd: null pointer");
  TAVSR_REQUIRE(ldh >= 2 * (int64_t)C && ldz >= C, TAVSR_EINVAL, "glu_dwconv_fwd: row strides shorter than 2C (h) / C (z)");
  return dt_fwd<DT_GLU>(h, ldh, w, bias, z, ldz, B, T, C, K, stream);
}

extern "C" int64_t tavsr_glu_dwconv_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) {
  return tavsr_glu_dwconv_ok(B, T, C, K) ? dt_bwd_ws(B, T, C, K) : 0;
}

extern "C" int tavsr_glu_dwconv_bwd(const float* dz, int64_t lddz, const float* h, int64_t ldh, const float* w, float* dh,
                                    int64_t lddh, float* dw, float* dbias, float* ws, int32_t B, int32_t T, int32_t C, int32_t K,
                                    tavsr_stream_t stream) {
  TAVSR_REQUIRE(tavsr_glu_dwconv_ok(B, T, C, K), TAVSR_EUNSUPPORTED,
                "glu_dwconv_bwd: odd kernel size <= %d and B, T, C >= 1 required (got B %d, T %d, C %d, K %d)", dt_kmax(DT_GLU), B, T, C, K);
  TAVSR_REQUIRE(dz && h && w && dh && dw && dbias && ws, TAVSR_EINVAL, "glu_dwconv_bwd: null pointer");
  TAVSR_REQUIRE(lddz >= C && ldh >= 2 * (int64_t)C && lddh >= 2 * (int64_t)C, TAVSR_EINVAL,
                "glu_dwconv_bwd: row strides shorter than C (dz) / 2C (h, dh)");
  return dt_bwd<DT_GLU>("glu_dwconv_bwd", dz, lddz, h, ldh, w, dh, lddh, dw, dbias, 0, ws, B, T, C, K, stream);
}
