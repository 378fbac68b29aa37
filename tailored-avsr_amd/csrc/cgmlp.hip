// cgMLP spatial gating unit at the recipe's kernel size, 31.
//   ConvolutionalSpatialGatingUnit (espnet2/asr/layers/cgmlp.py, called at
//   src/encoder/branchformer/encoder_layer.py:220): x_r * (depthwise_conv_k(LN(x_g)) + bias)
// The gate after a separate LayerNorm, out = r * (bias + dwconv_K(gn)), forward and backward with the taps in registers, and the
// whole unit fused with its LayerNorm (csgu_fwd_kernel).  Every other odd K up to 63 runs the gate form of the depthwise-
// convolution tile core (dwconv_time.hip), through the same entry points.
// HBM-bound, time-major tiles staged through LDS with the conv halo; parameter gradients go through
// per-block partial slabs + tavsr_sum_partials (deterministic, no atomics).
#include "common.h"

namespace tavsr {

constexpr int CG_CH = 64;    // channels per block (lanes -> consecutive channels: coalesced, LDS conflict free)
constexpr int CG_TT = 128;   // time steps per block
constexpr int CG_TB = 64;    // time steps per tile in the backward kernel

// out[b,t,c] = r[b,t,c] * (bias[c] + sum_k w[c,k] * gn[b,t+k-pad,c]) ; conv (pre-gate) optionally saved.
// The kernel size is a compile-time constant (the recipe's 31): the taps live in registers and four consecutive
// outputs share one sliding window of LDS reads (K + 3 reads for 4 outputs).
template <int K>
__global__ __launch_bounds__(256) void dwconv_gate_fwd_kfix_kernel(const float* __restrict__ gn, const float* __restrict__ r,
                                                                   int64_t ldr, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   float* __restrict__ conv, int B, int T, int C) {
  extern __shared__ float sm[];
  constexpr int pad = (K - 1) / 2, rows = CG_TT + K - 1;
  float* s_x = sm;                             // [rows][CG_CH]
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * CG_CH, t0 = blockIdx.y * CG_TT, b = blockIdx.z;
  const int c = c0 + cx;
  for (int ib = ty * 4; ib < rows; ib += 16) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ib + q, t = t0 + i - pad;
      v[q] = (i < rows && t >= 0 && t < T && c < C) ? gn[((int64_t)b * T + t) * C + c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (ib + q < rows) s_x[(ib + q) * CG_CH + cx] = v[q];
  }
  float wr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wr[k] = c < C ? w[(int64_t)c * K + k] : 0.f;
  __syncthreads();
  if (c >= C) return;
  const float bv = bias[c];
  constexpr int RPW = CG_TT / 4;               // rows per wave, contiguous
  for (int g = 0; g < RPW / 4; ++g) {
    const int tb = ty * RPW + g * 4;
    if (t0 + tb >= T) break;
    float rv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rv[q] = (t0 + tb + q < T) ? r[((int64_t)b * T + t0 + tb + q) * ldr + c] : 0.f;
    float o[4] = {bv, bv, bv, bv};
#pragma unroll
    for (int u = 0; u < K + 3; ++u) {
      const float v = s_x[(tb + u) * CG_CH + cx];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (u - q >= 0 && u - q < K) o[q] += wr[u - q] * v;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = t0 + tb + q;
      if (t < T) {
        const int64_t m = (int64_t)b * T + t;
        if (conv) conv[m * C + c] = o[q];
        out[m * C + c] = rv[q] * o[q];
      }
    }
  }
}

// The whole CSGU between the two channel projections in one launch (espnet ConvolutionalSpatialGatingUnit.forward: x_r, x_g =
// chunk(2); x_g = norm(x_g); x_g = depthwise conv over time; out = dropout(x_r * x_g)), given the LayerNorm statistics of the
// gate rows: block (64 channels, utterance) normalises its [T x 64] gate tile on the way into LDS (16-byte loads, all in flight
// together), convolves along time with the taps in registers and multiplies by x_r - the normalised gate never makes a round
// trip through HBM in eval, and is written once (with the convolution output) when the backward pass needs it.
template <int K>
__global__ __launch_bounds__(256, 2) void csgu_fwd_kernel(const float* __restrict__ g, int64_t ldg, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, float* __restrict__ conv, float* __restrict__ gn_out,
                                                       int B, int T, uint32_t thr, float inv_keep,
                                                       const uint64_t* __restrict__ seed, uint64_t offset4,
                                                       const float* __restrict__ rowstat, int stat_ld, float eps,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  // rowstat != null: the statistics come as per-row partial (sum, M2 about the tile's own mean) pairs of the 64-column tiles
  // of the GEMM that produced g ([rows][stat_ld][2]; the gate half is tiles C / 64 ..): the 16 lanes that load a row fetch one
  // pair each and merge them; block 0 writes mean / rstd out for the backward pass.
  constexpr int pad = (K - 1) / 2, rows = CG_TT + K - 1;
  __shared__ __attribute__((aligned(16))) float s_x[rows * CG_CH];
  __shared__ float s_w[CG_CH * K];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * CG_CH, b = blockIdx.y;
  for (int i = tid; i < CG_CH * K; i += 256) s_w[i] = w[(int64_t)c0 * K + i];      // the 64 x K tap block is contiguous
  // a thread = 4 consecutive channels (16-byte accesses everywhere) x, per pass, one of 16 rows
  const float4 gam = *reinterpret_cast<const float4*>(ln_w + c0 + 4 * (tid & 15));
  const float4 bet = *reinterpret_cast<const float4*>(ln_b + c0 + 4 * (tid & 15));
  const uint64_t sd = thr ? seed[0] : 0;
  // compute phase: a thread = 2 consecutive channels (taps in registers: 2 K of them) x CG_TT / 8 consecutive rows
  constexpr int RP = CG_TT / 8;
  const float2 bv = *reinterpret_cast<const float2*>(bias + c0 + 2 * (tid & 31));
  const int tid_ = tid;
  for (int t0 = 0; t0 < T; t0 += CG_TT) {
    if (t0) __syncthreads();                           // the previous tile has been read
    // lane coordinates the compiler cannot see through: otherwise every tile-invariant address of the body (~150 of them) is
    // hoisted out of this loop and spilled
    int tq_ = tid_;
    asm volatile("" : "+v"(tq_));
    const int l4 = tq_ & 15, rr = tq_ >> 4, cc = c0 + 4 * l4, l2 = tq_ & 31, rg = tq_ >> 5, c2 = c0 + 2 * l2;
    constexpr int NP = (rows + 15) / 16;
    float4 xv[NP];
    float mu[NP], rs[NP];
    // unconditional loads at clamped rows (straight-line code: all of them in flight together); uniform bases, 32-bit offsets
    const float* gb = g + (int64_t)b * T * ldg;
    const float* mb = mean + (int64_t)b * T;
    const float* sb = rstd + (int64_t)b * T;
    const int ldg32 = (int)ldg;
    float2 sp[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int tc = min(max(t0 + rr + 16 * q - pad, 0), T - 1);
      xv[q] = *reinterpret_cast<const float4*>(gb + (tc * ldg32 + C + cc));
      if (rowstat) {
        const int nt = C >> 6;                           // gate tiles (<= 16: one per lane of the row's 16)
        sp[q] = l4 < nt ? *reinterpret_cast<const float2*>(rowstat + ((int64_t)(b * T + tc) * stat_ld + nt + l4) * 2)
                        : make_float2(0.f, 0.f);
      } else {
        mu[q] = mb[tc];
        rs[q] = sb[tc];
      }
    }
    if (rowstat) {
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        // equal-count Chan merge of the nt tiles (every gate tile is a whole 64 columns): mean = avg of the tile means,
        // C var = sum M2_t + 64 sum (mean_t - mean)^2 - never from raw second moments (no cancellation)
        float s1 = sp[q].x;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s1 += __shfl_xor(s1, o, 64);
        const float m_ = s1 / (float)C;
        const float dm = l4 < (C >> 6) ? sp[q].x * (1.f / 64.f) - m_ : 0.f;
        float s2 = sp[q].y + 64.f * dm * dm;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
        mu[q] = m_;
        rs[q] = rsqrtf(s2 / (float)C + eps);
        const int i = rr + 16 * q, t = t0 + i - pad;
        if (mean_out && blockIdx.x == 0 && l4 == 0 && i >= pad && i < pad + CG_TT && t < T) {
          mean_out[(int64_t)b * T + t] = mu[q];
          rstd_out[(int64_t)b * T + t] = rs[q];
        }
      }
    }
    // x_r of the thread's output rows (rows tb .. tb + RP - 1 of the tile), fetched together with the gate tile
    const int tb = rg * RP;
    float2 rv[RP];
#pragma unroll
    for (int q = 0; q < RP; ++q) rv[q] = *reinterpret_cast<const float2*>(gb + (min(t0 + tb + q, T - 1) * ldg32 + c2));
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int i = rr + 16 * q, t = t0 + i - pad;
      if (i < rows) {
        const bool ok = t >= 0 && t < T;                // outside the utterance the convolution sees zeros, not beta
        const float4 v = ok ? make_float4((xv[q].x - mu[q]) * rs[q] * gam.x + bet.x, (xv[q].y - mu[q]) * rs[q] * gam.y + bet.y,
                                          (xv[q].z - mu[q]) * rs[q] * gam.z + bet.z, (xv[q].w - mu[q]) * rs[q] * gam.w + bet.w)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&s_x[i * CG_CH + 4 * l4]) = v;
        if (gn_out && ok && i >= pad && i < pad + CG_TT)
          *reinterpret_cast<float4*>(gn_out + ((int64_t)b * T + t) * C + cc) = v;
      }
    }
    __syncthreads();
    float2 wv[K];                                       // (per tile: not live across the load phase)
#pragma unroll
    for (int k = 0; k < K; ++k) wv[k] = make_float2(s_w[(2 * l2) * K + k], s_w[(2 * l2 + 1) * K + k]);
#pragma unroll
    for (int gi = 0; gi < RP / 4; ++gi) {               // 4 outputs share one sliding window of K + 3 LDS rows
      const int tq = tb + 4 * gi;
      if (t0 + tq >= T) break;
      float2 o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = bv;
#pragma unroll
      for (int u = 0; u < K + 3; ++u) {
        const float2 v = *reinterpret_cast<const float2*>(&s_x[(tq + u) * CG_CH + 2 * l2]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (u - q >= 0 && u - q < K) { o[q].x += wv[u - q].x * v.x; o[q].y += wv[u - q].y * v.y; }
        if ((u & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // a few window rows in flight at a time, not all of them
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + tq + q;
        if (t < T) {
          const int64_t e = ((int64_t)b * T + t) * C + c2;
          if (conv) *reinterpret_cast<float2*>(conv + e) = o[q];
          float2 y = make_float2(rv[4 * gi + q].x * o[q].x, rv[4 * gi + q].y * o[q].y);
          if (thr) {                                    // tavsr_dropout's mapping: element e = word e & 3 of counter offset4 + e / 4
            const uint64_t ctr = offset4 + ((uint64_t)e >> 2);
            uint32_t r4[4];
            philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), r4);
            const uint32_t ra = (e & 2) ? r4[2] : r4[0], rb = (e & 2) ? r4[3] : r4[1];
            y.x = ra >= thr ? y.x * inv_keep : 0.f;
            y.y = rb >= thr ? y.y * inv_keep : 0.f;
          }
          *reinterpret_cast<float2*>(out + e) = y;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// du -> dr = du*conv ; dconv = du*r ; dgn[t] = sum_k w[c,k]*dconv[t-k+pad] ;
// dw[c,k] = sum_{b,t} dconv[t]*gn[t+k-pad], dbias[c] = sum_{b,t} dconv[t].
// One block per (64 channels, utterance): it walks the utterance in time tiles of CG_TB steps (dconv and gn tiles
// with their conv halo in LDS, lanes = consecutive channels: coalesced and bank-conflict free) and keeps the
// weight-gradient sums in registers - thread (channel c, wave y) owns taps k = y, y+4, ... (tap K is the bias) - so
// there is no cross-thread reduction and one partial slab [C][K+1] per utterance, summed by sum_partials_kernel.
// Taps in registers, four consecutive data gradients per sliding window, and the weight gradient in groups of four
// rows 4 apart (rows r, r+4, r+8, r+12 need gn rows r+ty+4s, s = 0..10: the taps this thread owns, k = ty + 4j, line
// up across them).
template <int K>
__global__ __launch_bounds__(256) void dwconv_gate_bwd_kfix_kernel(const float* __restrict__ du, const float* __restrict__ gn,
                                                                   const float* __restrict__ r, int64_t ldr,
                                                                   const float* __restrict__ conv,
                                                                   const float* __restrict__ w, float* __restrict__ dr,
                                                                   int64_t lddr, float* __restrict__ dgn,
                                                                   float* __restrict__ part, int B, int T, int C,
                                                                   const float* __restrict__ zr, int64_t ldz, int act) {
  // zr != null: r = act(zr) is the left half of cgMLP's activated projection; dr is written as the gradient w.r.t. zr
  // (dr * act'(zr)): no activation-backward pass over that half afterwards
  extern __shared__ float sm[];
  constexpr int pad = (K - 1) / 2, rows = CG_TB + K - 1;
  constexpr int NTAP = (K + 1 + 3) / 4;        // taps per thread (tap K is the bias)
  static_assert(CG_TB == 64 && NTAP == 8, "row grouping below assumes 64-step tiles and 8 taps per thread");
  float* s_d = sm;                         // dconv with halo [rows][CG_CH]
  float* s_g = s_d + rows * CG_CH;         // gn with halo    [rows][CG_CH]
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * CG_CH, b = blockIdx.y;
  const int c = c0 + cx;
  const bool cok = c < C;
  float wr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wr[k] = cok ? w[(int64_t)c * K + k] : 0.f;
  float acc[NTAP];
#pragma unroll
  for (int j = 0; j < NTAP; ++j) acc[j] = 0.f;
  for (int t0 = 0; t0 < T; t0 += CG_TB) {
    __syncthreads();
    for (int ib = ty * 4; ib < rows; ib += 16) {
      float duv[4], rv[4], gv[4], cv[4], zv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ib + q, t = t0 + i - pad;
        duv[q] = rv[q] = gv[q] = cv[q] = zv[q] = 0.f;
        if (i < rows && t >= 0 && t < T && cok) {
          const int64_t m = (int64_t)b * T + t;
          duv[q] = du[m * C + c];
          rv[q] = r[m * ldr + c];
          gv[q] = gn[m * C + c];
          if (i >= pad && i < pad + CG_TB) {
            cv[q] = conv[m * C + c];
            if (zr) zv[q] = zr[m * ldz + c];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ib + q, t = t0 + i - pad;
        if (i < rows) {
          s_d[i * CG_CH + cx] = duv[q] * rv[q];
          s_g[i * CG_CH + cx] = gv[q];
          if (i >= pad && i < pad + CG_TB && t < T && cok) {
            float v = duv[q] * cv[q];
            if (zr) v *= act_bwd(act, zv[q]);
            dr[((int64_t)b * T + t) * lddr + c] = v;
          }
        }
      }
    }
    __syncthreads();
    const int nt = min(CG_TB, T - t0);
    if (cok) {
      // data gradients: wave ty owns rows [16 ty, 16 ty + 16), four at a time; dgn[tt] = sum_k w[k] * s_d[tt + 2 pad - k]
      for (int g = 0; g < 4; ++g) {
        const int tb = ty * 16 + g * 4;
        if (tb >= nt) break;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = -3; u < K; ++u) {          // LDS row tb + 2 pad - u feeds output q with tap u + q
          const float v = s_d[(tb + 2 * pad - u) * CG_CH + cx];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (u + q >= 0 && u + q < K) o[q] += wr[u + q] * v;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (tb + q < nt) dgn[((int64_t)b * T + t0 + tb + q) * C + c] = o[q];
      }
      // weight gradient: acc[j] += dconv[tt] * gn row (tt + ty + 4 j); the bias tap (k == K: ty == 3, j == 7) adds dconv
      for (int m4 = 0; m4 < 4; ++m4) {
#pragma unroll
        for (int r0 = 0; r0 < 4; ++r0) {
          const int rb = m4 * 16 + r0;          // rows rb, rb + 4, rb + 8, rb + 12
          if (rb >= nt) continue;
          float dv[4], G[11];
#pragma unroll
          for (int a = 0; a < 4; ++a) dv[a] = (rb + 4 * a < nt) ? s_d[(rb + 4 * a + pad) * CG_CH + cx] : 0.f;
#pragma unroll
          for (int sidx = 0; sidx < 11; ++sidx) {
            const int row = rb + ty + 4 * sidx;
            G[sidx] = row < rows ? s_g[row * CG_CH + cx] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < NTAP; ++j) {
            const bool is_bias = (ty + 4 * j == K);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[j] += dv[a] * (is_bias ? 1.f : G[a + j]);
          }
        }
      }
    }
  }
  if (cok) {
    float* pw = part + ((int64_t)b * C + c) * (K + 1);
#pragma unroll
    for (int j = 0; j < NTAP; ++j)
      if (ty + 4 * j <= K) pw[ty + 4 * j] = acc[j];
  }
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_dwconv_gate_fwd(const float* gn, const float* r, int64_t ldr, const float* w, const float* bias,
                                     float* out, float* conv, int32_t B, int32_t T, int32_t C, int32_t K,
                                     tavsr_stream_t stream) {
  TAVSR_REQUIRE(gn && r && w && bias && out, TAVSR_EINVAL, "dwconv_gate_fwd: null pointer");
  if (K != 31) return dt_gate_fwd(gn, r, ldr, w, bias, out, conv, B, T, C, K, stream);
  if (B <= 0 || T <= 0 || C <= 0) return TAVSR_OK;
  hipLaunchKernelGGL(dwconv_gate_fwd_kfix_kernel<31>, dim3(cdiv(C, CG_CH), cdiv(T, CG_TT), B), dim3(256),
                     (CG_TT + 30) * CG_CH * sizeof(float), (hipStream_t)stream, gn, r, ldr, w, bias, out, conv, B, T, C);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_csgu_fwd(const float* g, int64_t ldg, const float* ln_w, const float* ln_b, float eps, const float* conv_w,
                              const float* conv_b, float* out, float* gn, float* conv, float* mean, float* rstd, float p_drop,
                              const uint64_t* seed_dev, uint64_t offset, int32_t B, int32_t T, int32_t C, int32_t K,
                              const float* rowstat, tavsr_stream_t stream) {
  TAVSR_REQUIRE(g && ln_w && ln_b && conv_w && conv_b && out && mean && rstd, TAVSR_EINVAL, "csgu_fwd: null pointer");
  TAVSR_REQUIRE(K == 31 && C > 0 && C % CG_CH == 0, TAVSR_EUNSUPPORTED, "csgu_fwd: kernel size 31 and C %% 64 == 0 (got %d, %d)", K, C);
  TAVSR_REQUIRE(ldg % 4 == 0 && ldg >= 2 * (int64_t)C && ((uintptr_t)g % 16 == 0) && ((uintptr_t)ln_w % 16 == 0) &&
                    ((uintptr_t)ln_b % 16 == 0) && (!gn || (uintptr_t)gn % 16 == 0), TAVSR_EALIGN, "csgu_fwd: rows must be 16-byte aligned");
  TAVSR_REQUIRE(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed_dev) && offset % 4 == 0, TAVSR_EINVAL,
                "csgu_fwd: dropout needs p in [0, 1), a device seed and an offset %% 4 == 0");
  if (B <= 0 || T <= 0) return TAVSR_OK;
  // statistics of the gate rows (columns C .. 2C-1 of g) - a launch of their own, or the producing GEMM's row statistics -
  // then the fused pass
  if (rowstat) {
    TAVSR_REQUIRE(C <= 1024 && ldg % 64 == 0 && ((uintptr_t)rowstat % 8 == 0), TAVSR_EUNSUPPORTED,
                  "csgu_fwd: GEMM row statistics need C <= 1024 and a row stride %% 64 == 0");
  } else {
    int rc = tavsr_layernorm_fwd(g + C, ldg, nullptr, nullptr, eps, nullptr, 0, mean, rstd, B * T, C, stream);
    if (rc) return rc;
  }
  const uint32_t thr = p_drop > 0.f ? (uint32_t)((double)p_drop * 4294967296.0) : 0u;
  hipLaunchKernelGGL(csgu_fwd_kernel<31>, dim3(C / CG_CH, B), dim3(256), 0, (hipStream_t)stream, g, ldg, C, mean, rstd, ln_w, ln_b,
                     conv_w, conv_b, out, conv, gn, B, T, thr, p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f, seed_dev, offset / 4,
                     rowstat, (int)(ldg / 64), eps, mean, rstd);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

// K = 31: one slab [C][K+1] per utterance and one for their sum; the core's slabs otherwise
extern "C" int64_t tavsr_dwconv_gate_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K) {
  return K == 31 ? ((int64_t)B + 1) * C * (K + 1) : dt_bwd_ws(B, T, C, K);
}

static int dwconv_gate_bwd_impl(const float* du, const float* gn, const float* r, int64_t ldr, const float* conv, const float* w,
                               float* dr, int64_t lddr, float* dgn, float* dw, float* dbias, int32_t accumulate, float* ws, int32_t B,
                               int32_t T, int32_t C, int32_t K, const float* zr, int64_t ldz, int32_t act, tavsr_stream_t stream) {
  TAVSR_REQUIRE(du && gn && r && conv && w && dr && dgn && dw && dbias && ws, TAVSR_EINVAL,
                "dwconv_gate_bwd: null pointer");
  if (K != 31) return dt_gate_bwd(du, gn, r, ldr, conv, w, dr, lddr, dgn, dw, dbias, accumulate, ws, B, T, C, K, stream);
  if (B <= 0 || T <= 0 || C <= 0) return TAVSR_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dwconv_gate_bwd_kfix_kernel<31>, dim3(cdiv(C, CG_CH), B), dim3(256),
                     2 * (CG_TB + 30) * CG_CH * sizeof(float), s, du, gn, r, ldr, conv, w, dr, lddr, dgn, ws, B, T, C, zr, ldz, (int)act);
  TAVSR_LAUNCH_CHECK();
  const int nblk = B, n = C * (K + 1);
  float* sum = ws + (int64_t)nblk * n;
  int rc = tavsr_sum_partials(ws, nblk, n, sum, n, 0, stream);
  if (rc) return rc;
  return dwconv_split(sum, dw, dbias, C, K, accumulate, s);
}

extern "C" int tavsr_dwconv_gate_bwd(const float* du, const float* gn, const float* r, int64_t ldr, const float* conv,
                                     const float* w, float* dr, int64_t lddr, float* dgn, float* dw, float* dbias,
                                     int32_t accumulate, float* ws, int32_t B, int32_t T, int32_t C, int32_t K,
                                     tavsr_stream_t stream) {
  return dwconv_gate_bwd_impl(du, gn, r, ldr, conv, w, dr, lddr, dgn, dw, dbias, accumulate, ws, B, T, C, K, nullptr, 0, 0, stream);
}

// ... with r = act(zr): dr comes back as the gradient w.r.t. the pre-activation zr (kernel size 31 only)
extern "C" int tavsr_dwconv_gate_bwd_act(const float* du, const float* gn, const float* r, int64_t ldr, const float* conv,
                                         const float* w, float* dr, int64_t lddr, float* dgn, float* dw, float* dbias,
                                         int32_t accumulate, float* ws, int32_t B, int32_t T, int32_t C, int32_t K,
                                         const float* zr, int64_t ldz, int32_t act, tavsr_stream_t stream) {
  TAVSR_REQUIRE(zr && K == 31, TAVSR_EUNSUPPORTED, "dwconv_gate_bwd_act: needs zr and kernel size 31 (K=%d)", K);
  return dwconv_gate_bwd_impl(du, gn, r, ldr, conv, w, dr, lddr, dgn, dw, dbias, accumulate, ws, B, T, C, K, zr, ldz, act, stream);
}
