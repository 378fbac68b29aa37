// Fastformer additive attention (espnet2 asr/layers/fastformer.py FastSelfAttention; the `fast_selfattn` option of
// src/encoder/branchformer/encoder.py:106-120,223-259) between the q | k projection GEMM and the `transform` GEMM, forward and
// backward, and the absolute positional encodings' add (PositionalEncoding / ScaledPositionalEncoding).
//
//   s[b,h,t]  = (<W[h,:], x[b,t,:] * cs[b,:]> + bias[h]) / sqrt(dh)        the dot spans ALL D columns, cs = 1 for the query
//   w[b,h,:]  = softmax over the t < len[b] of s[b,h,:], exactly 0 at the padded frames
//   pool[b,c] = sum_{t < len[b]} w[b,head(c),t] * x[b,t,c] * cs[b,c]
// once on the query rows (alpha, pq) and once on the key rows scaled by pq (beta, pk); then wv = pk * q on every row.
//
// Launches.  The score dots read whole rows, the pooling reads one head's columns: they are two launches.  The score pass is
// row-parallel (one wave per frame, a block per 64 frames of one utterance: B * ceil(T / 64) blocks, 256 at B = 32, T = 499), the
// pooling pass has one block per (utterance, head) and reads T scores and a T x dh slice.  Folding the scores into the (b, h)
// blocks would make each of the 32 - 96 blocks a batch gives read all D columns of its utterance: H times the traffic on a
// third of the 256 CUs.  Rows stream from HBM / L2 at any T: nothing of size T is kept in LDS.
//
// Backward.  dq and dk come from two more row-parallel launches (the mirror of the two score passes); each block leaves its
// share of d query_att / d key_att (weight | bias) and of d pq as one partial slab, and the slabs are summed in a fixed order
// (tavsr_sum_partials): no atomics, the same bits every run.  The bias gradients are computed (sums of softmax gradients, zero
// up to rounding), not assumed.
//
// Padded frames (t >= len[b]) are never read by the pooling or by any parameter gradient: they are skipped by control flow,
// never multiplied by a zero weight, so NaN there stays there.  The one reduction the reference takes over ALL T rows is
// d pk = sum_t dwv * q (the output rows transform(pk * q) + q exist at padded frames too); a padded row takes part in it only
// where its upstream gradient is not exactly zero.
//
// Range: 1 <= H <= 8, D <= 512, D % H == 0 and dh = D / H a multiple of 4 (a lane's 16-byte vector never straddles two heads);
// row strides multiples of 4 floats and 16-byte aligned row starts.  tavsr_fastattn_ok tells; the entries refuse the rest.
#include "common.h"

namespace tavsr {

constexpr int kFaRows = 64;      // frames of one utterance per block of the row-parallel launches
constexpr int kFaMaxH = 8;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 fma4(const float s, const float4 a, const float4 c) {
  return make_float4(fmaf(s, a.x, c.x), fmaf(s, a.y, c.y), fmaf(s, a.z, c.z), fmaf(s, a.w, c.w));
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ int clamp_len(const int64_t* lens, int b, int T) {
  const int64_t n = lens ? lens[b] : (int64_t)T;
  return n < 0 ? 0 : (n > T ? T : (int)n);
}

// score[b,h,t] for the frames of one block; padded frames get 0 (never read).  NV: 16-byte vectors per lane (D <= 256 * NV)
template <int NV>
__global__ __launch_bounds__(256) void fa_score_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ cs,
                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                       const int64_t* __restrict__ lens, float* __restrict__ score, int T, int D,
                                                       int H, float scale) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = clamp_len(lens, b, T);
  const int t0 = blockIdx.x * kFaRows;
  float4 w[kFaMaxH][NV];
  bool ok[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c0 = (i * 64 + lane) * 4;
    ok[i] = c0 < D;
    const float4 s = ok[i] ? (cs ? ld4(cs + (int64_t)b * D + c0) : make_float4(1.f, 1.f, 1.f, 1.f)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int h = 0; h < kFaMaxH; ++h)
      w[h][i] = (h < H && ok[i]) ? mul4(ld4(W + (int64_t)h * D + c0), s) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float my_bias = lane < H ? bias[lane] : 0.f;
  for (int t = t0 + wave; t < t0 + kFaRows && t < T; t += 4) {      // (wave-uniform)
    float mine = 0.f;
    if (t < len) {
      const float* row = x + ((int64_t)b * T + t) * ldx;
      float4 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = ok[i] ? ld4(row + (i * 64 + lane) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int h = 0; h < kFaMaxH; ++h) {
        if (h < H) {
          float part = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) part += dot4(v[i], w[h][i]);
          const float s = wave_sum(part);
          if (lane == h) mine = scale * (s + my_bias);
        }
      }
    }
    if (lane < H) score[((int64_t)b * H + lane) * T + t] = mine;
  }
}

__device__ __forceinline__ float block_max4(float v, float* red) {      // 256 threads; red: 4 floats of LDS
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum4(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// one block per (head, utterance): the masked softmax of the head's scores over time (two passes: max, then sum, in fp32 on
// v_exp_f32), the weights written for every t < T (0 at the padded frames), then the weighted sum of the head's dh columns
__global__ __launch_bounds__(256) void fa_pool_kernel(const float* __restrict__ score, const float* __restrict__ x, int64_t ldx,
                                                      const float* __restrict__ cs, const int64_t* __restrict__ lens,
                                                      float* __restrict__ wout, float* __restrict__ pooled, int T, int D, int H) {
  __shared__ float red[4];
  __shared__ float acc_lds[256];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int dh = D / H;
  const int len = clamp_len(lens, b, T);
  const float* s = score + ((int64_t)b * H + h) * T;
  float* wo = wout + ((int64_t)b * H + h) * T;
  float m = -INFINITY;
  for (int t = tid; t < len; t += 256) m = fmaxf(m, s[t]);
  m = block_max4(m, red);
  float sum = 0.f;
  for (int t = tid; t < len; t += 256) sum += __builtin_amdgcn_exp2f((s[t] - m) * kLog2e);
  sum = block_sum4(sum, red);
  const float inv = len > 0 ? 1.f / sum : 0.f;
  for (int t = tid; t < T; t += 256) wo[t] = t < len ? __builtin_amdgcn_exp2f((s[t] - m) * kLog2e) * inv : 0.f;
  __syncthreads();      // the weights are read back below by other threads of this block
  const int CW = dh < 256 ? dh : 256, lanes = 256 / CW;
  const int r = tid / CW, cc = tid - r * CW;
  for (int cb = 0; cb < dh; cb += CW) {      // (one round unless dh > 256)
    const int c = cb + cc;
    float acc = 0.f;
    if (r < lanes && c < dh) {
      const int col = h * dh + c;
      const float k = cs ? cs[(int64_t)b * D + col] : 1.f;
      for (int t = r; t < len; t += lanes) acc = fmaf(wo[t], x[((int64_t)b * T + t) * ldx + col] * k, acc);
    }
    __syncthreads();
    acc_lds[tid] = acc;
    __syncthreads();
    if (r == 0 && c < dh) {
      float tot = 0.f;
      for (int j = 0; j < lanes; ++j) tot += acc_lds[j * CW + cc];      // fixed order
      pooled[(int64_t)b * D + h * dh + c] = tot;
    }
  }
}

// wv[b,t,:] = pk[b,:] * q[b,t,:] on every row (the padded ones too: the reference computes them)
__global__ __launch_bounds__(256) void fa_scale_rows_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ pk,
                                                            float* __restrict__ wv, int64_t M, int T, int D) {
  const int D4 = D >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * D4) return;
  const int64_t row = i / D4;
  const int c0 = (int)(i - row * D4) * 4;
  const int64_t b = row / T;
  st4(wv + row * D + c0, mul4(ld4(q + row * ldq + c0), ld4(pk + b * D + c0)));
}

// dpk[b,c] = sum_t dwv[b,t,c] * q[b,t,c]; a padded frame takes part only where its upstream gradient is not exactly zero
__global__ __launch_bounds__(256) void fa_bwd_pool_kernel(const float* __restrict__ dwv, int64_t ldd, const float* __restrict__ q,
                                                          int64_t ldq, const int64_t* __restrict__ lens, float* __restrict__ dpk,
                                                          int T, int D) {
  __shared__ float acc_lds[256];
  const int b = blockIdx.y, cc = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cc;
  const int len = clamp_len(lens, b, T);
  float acc = 0.f;
  if (c < D)
    for (int t = r; t < T; t += 4) {
      const int64_t row = (int64_t)b * T + t;
      const float g = dwv[row * ldd + c];
      if (t < len || g != 0.f) acc = fmaf(g, q[row * ldq + c], acc);
    }
  acc_lds[threadIdx.x] = acc;
  __syncthreads();
  if (r == 0 && c < D) dpk[(int64_t)b * D + c] = (acc_lds[cc] + acc_lds[64 + cc]) + (acc_lds[128 + cc] + acc_lds[192 + cc]);
}

// The mirror of a score + pooling pass on the frames of one block.  For the valid frames, with xs = x * cs:
//   da[h] = <dpool, xs>_head h,  ds[h] = w[h,t] * (da[h] - <dpool, pool>_head h),
//   g[c]  = w[head(c),t] * dpool[c] + scale * sum_h ds[h] * W[h,c]                      (the gradient of xs)
// IS_K: dx = g * cs (0 at the padded frames) and the block's share of d cs = sum_t g * x;  query: dx = dres + dwv * pk + g on
// every row (dres + dwv * pk at the padded ones).  The block's shares of dW[h,c] = scale * sum_t ds[h] * xs[c] and
// db[h] = scale * sum_t ds[h] go to its slab part[blk] = dW [H*D] | db [H] | d cs [D] (IS_K).
template <int NV, bool IS_K>
__global__ __launch_bounds__(256) void fa_bwd_rows_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ cs,
                                                          const float* __restrict__ wpool, const float* __restrict__ dpool,
                                                          const float* __restrict__ pool, const float* __restrict__ W,
                                                          const int64_t* __restrict__ lens, const float* __restrict__ dres,
                                                          int64_t lddres, const float* __restrict__ dwv, int64_t lddwv,
                                                          const float* __restrict__ pk, float* __restrict__ dx, int64_t lddx,
                                                          float* __restrict__ part, int64_t part_stride, int T, int D, int H,
                                                          float scale) {
  __shared__ __attribute__((aligned(16))) float lds[4][512];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dh = D / H;
  const int len = clamp_len(lens, b, T);
  const int t0 = blockIdx.x * kFaRows;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 w[kFaMaxH][NV], accw[kFaMaxH][NV], dpl[NV], csv[NV], pkv[NV], accq[NV];
  float accb[kFaMaxH], dotp[kFaMaxH];
  int hc[NV];
  bool ok[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c0 = (i * 64 + lane) * 4;
    ok[i] = c0 < D;
    hc[i] = ok[i] ? c0 / dh : -1;
    dpl[i] = ok[i] ? ld4(dpool + (int64_t)b * D + c0) : zero;
    csv[i] = (IS_K && ok[i]) ? ld4(cs + (int64_t)b * D + c0) : zero;
    pkv[i] = (!IS_K && ok[i]) ? ld4(pk + (int64_t)b * D + c0) : zero;
    accq[i] = zero;
#pragma unroll
    for (int h = 0; h < kFaMaxH; ++h) {
      w[h][i] = (h < H && ok[i]) ? ld4(W + (int64_t)h * D + c0) : zero;
      accw[h][i] = zero;
    }
  }
#pragma unroll
  for (int h = 0; h < kFaMaxH; ++h) {
    accb[h] = 0.f;
    dotp[h] = 0.f;
    if (h < H) {
      float part_ = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (hc[i] == h) part_ += dot4(dpl[i], ld4(pool + (int64_t)b * D + (i * 64 + lane) * 4));
      dotp[h] = wave_sum(part_);
    }
  }
  for (int t = t0 + wave; t < t0 + kFaRows && t < T; t += 4) {      // (wave-uniform)
    const int64_t row = (int64_t)b * T + t;
    if (t >= len) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (ok[i]) {
          const int c0 = (i * 64 + lane) * 4;
          if (IS_K) st4(dx + row * lddx + c0, zero);
          else {
            const float4 r = ld4(dres + row * lddres + c0), g = ld4(dwv + row * lddwv + c0);
            st4(dx + row * lddx + c0, make_float4(fmaf(g.x, pkv[i].x, r.x), fmaf(g.y, pkv[i].y, r.y), fmaf(g.z, pkv[i].z, r.z),
                                                  fmaf(g.w, pkv[i].w, r.w)));
          }
        }
      continue;
    }
    float4 xv[NV], xs[NV], g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      xv[i] = ok[i] ? ld4(x + row * ldx + (i * 64 + lane) * 4) : zero;
      xs[i] = IS_K ? mul4(xv[i], csv[i]) : xv[i];
      g[i] = zero;
    }
    float wsel[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) wsel[i] = 0.f;
#pragma unroll
    for (int h = 0; h < kFaMaxH; ++h) {
      if (h < H) {
        float part_ = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (hc[i] == h) part_ += dot4(dpl[i], xs[i]);
        const float da = wave_sum(part_);
        const float wt = wpool[((int64_t)b * H + h) * T + t];
        const float ds = scale * (wt * (da - dotp[h]));
        accb[h] += ds;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          if (hc[i] == h) wsel[i] = wt;
          g[i] = fma4(ds, w[h][i], g[i]);
          accw[h][i] = fma4(ds, xs[i], accw[h][i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!ok[i]) continue;
      const int c0 = (i * 64 + lane) * 4;
      g[i] = fma4(wsel[i], dpl[i], g[i]);
      if (IS_K) {
        st4(dx + row * lddx + c0, mul4(g[i], csv[i]));
        accq[i] = make_float4(fmaf(g[i].x, xv[i].x, accq[i].x), fmaf(g[i].y, xv[i].y, accq[i].y), fmaf(g[i].z, xv[i].z, accq[i].z),
                              fmaf(g[i].w, xv[i].w, accq[i].w));
      } else {
        const float4 r = ld4(dres + row * lddres + c0), u = ld4(dwv + row * lddwv + c0);
        st4(dx + row * lddx + c0, make_float4(r.x + fmaf(u.x, pkv[i].x, g[i].x), r.y + fmaf(u.y, pkv[i].y, g[i].y),
                                              r.z + fmaf(u.z, pkv[i].z, g[i].z), r.w + fmaf(u.w, pkv[i].w, g[i].w)));
      }
    }
  }
  // the four waves' shares, added in a fixed order, into the block's slab
  float* slab = part + ((int64_t)b * gridDim.x + blockIdx.x) * part_stride;
  const int rounds = H + (IS_K ? 1 : 0);
  for (int rd = 0; rd < rounds; ++rd) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!ok[i]) continue;
      float4 v = accq[i];      // (the round behind the H weight rows: the key rows' share of d cs)
#pragma unroll
      for (int h = 0; h < kFaMaxH; ++h)
        if (h == rd && rd < H) v = accw[h][i];
      st4(&lds[wave][(i * 64 + lane) * 4], v);
    }
    __syncthreads();
    float* dst = slab + (rd < H ? (int64_t)rd * D : (int64_t)H * D + H);
    for (int c = threadIdx.x; c < D; c += 256) dst[c] = (lds[0][c] + lds[1][c]) + (lds[2][c] + lds[3][c]);
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < kFaMaxH; ++h) lds[wave][h] = accb[h];
  }
  __syncthreads();
  if (threadIdx.x < H) {
    const int h = threadIdx.x;
    slab[(int64_t)H * D + h] = (lds[0][h] + lds[1][h]) + (lds[2][h] + lds[3][h]);
  }
}

// dcs[b,c] = sum over the utterance's blocks, in block order, of their shares
__global__ __launch_bounds__(256) void fa_sum_dcs_kernel(const float* __restrict__ part, int64_t part_stride, int nchunk, int64_t off,
                                                         float* __restrict__ dcs, int D) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  float acc = 0.f;
  for (int j = 0; j < nchunk; ++j) acc += part[((int64_t)b * nchunk + j) * part_stride + off + c];
  dcs[(int64_t)b * D + c] = acc;
}

// y[b,t,:] = xscale * x[b,t,:] + a * pe[t,:], a = *alpha (device scalar) or 1
__global__ __launch_bounds__(256) void add_pe_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                                     const float* __restrict__ alpha, float xscale, float* __restrict__ y, int64_t n,
                                                     int64_t TD) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = alpha ? alpha[0] : 1.f;
  y[i] = fmaf(xscale, x[i], a * pe[i % TD]);
}

constexpr int kPeBlocks = 128;
// part[blk] = this block's share of sum dy * pe (elements blk*256 + tid, stride 128 * 256): a fixed assignment, a fixed order
__global__ __launch_bounds__(256) void add_pe_dalpha_kernel(const float* __restrict__ dy, const float* __restrict__ pe, int64_t n,
                                                            int64_t TD, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kPeBlocks * 256) acc = fmaf(dy[i], pe[i % TD], acc);
  acc = block_sum4(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// (the same range: fastattn_ok of tavsr/ops/fastattn.py, which constructors ask without the library, and the words of
// ops.FASTATTN_LIMIT - the three change together)
static bool fa_shape_ok(int D, int H) { return H >= 1 && H <= kFaMaxH && D >= 4 && D <= 512 && D % H == 0 && (D / H) % 4 == 0; }
static bool fa_rows_ok(const float* p, int64_t ld) { return (ld % 4) == 0 && ((uintptr_t)p & 15) == 0; }
static int fa_chunks(int T) { return (T + kFaRows - 1) / kFaRows; }
static int64_t fa_part_stride(int D, int H) { return ((int64_t)H * D + H + D + 63) / 64 * 64; }

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_fastattn_ok(int32_t D, int32_t H) { return fa_shape_ok(D, H) ? 1 : 0; }

#define FA_SHAPE_REQUIRE(what)                                                                                                  \
  TAVSR_REQUIRE(fa_shape_ok(D, H), TAVSR_EUNSUPPORTED, what ": 1 <= H <= 8, D <= 512, D %% H == 0 and D / H a multiple of 4 (got D %d, H %d)", \
                D, H);                                                                                                          \
  TAVSR_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && (int64_t)B * T < (1ll << 31), TAVSR_EUNSUPPORTED, what ": 1 <= B <= 65535, T >= 1, B * T < 2^31")

extern "C" int tavsr_fastattn_pool(const float* x, int64_t ldx, const float* cs, const float* W, const float* bias, const int64_t* lens,
                                   float* score_ws, float* w_out, float* pooled, int32_t B, int32_t T, int32_t D, int32_t H,
                                   tavsr_stream_t stream) {
  TAVSR_REQUIRE(x && W && bias && score_ws && w_out && pooled, TAVSR_EINVAL, "fastattn_pool: null pointer");
  FA_SHAPE_REQUIRE("fastattn_pool");
  TAVSR_REQUIRE(fa_rows_ok(x, ldx) && fa_rows_ok(W, D) && (!cs || fa_rows_ok(cs, D)), TAVSR_EALIGN,
                "fastattn_pool: rows must start 16-byte aligned (strides multiples of 4)");
  const float scale = 1.f / sqrtf((float)(D / H));
  const dim3 grid(fa_chunks(T), B);
  if (D <= 256)
    hipLaunchKernelGGL(fa_score_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, cs, W, bias, lens, score_ws, T, D, H, scale);
  else
    hipLaunchKernelGGL(fa_score_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, cs, W, bias, lens, score_ws, T, D, H, scale);
  TAVSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fa_pool_kernel, dim3(H, B), dim3(256), 0, (hipStream_t)stream, score_ws, x, ldx, cs, lens, w_out, pooled, T, D, H);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_fastattn_scale_rows(const float* q, int64_t ldq, const float* pk, float* wv, int32_t B, int32_t T, int32_t D,
                                         tavsr_stream_t stream) {
  TAVSR_REQUIRE(q && pk && wv, TAVSR_EINVAL, "fastattn_scale_rows: null pointer");
  TAVSR_REQUIRE(B >= 1 && T >= 1 && D >= 4 && D % 4 == 0 && (int64_t)B * T < (1ll << 31), TAVSR_EUNSUPPORTED,
                "fastattn_scale_rows: D must be a multiple of 4, B * T < 2^31");
  TAVSR_REQUIRE(fa_rows_ok(q, ldq) && fa_rows_ok(pk, D) && fa_rows_ok(wv, D), TAVSR_EALIGN, "fastattn_scale_rows: 16-byte aligned rows");
  const int64_t M = (int64_t)B * T, n4 = M * (D / 4);
  hipLaunchKernelGGL(fa_scale_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, ldq, pk, wv, M, T, D);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_fastattn_bwd_pool(const float* dwv, int64_t lddwv, const float* q, int64_t ldq, const int64_t* lens, float* dpk,
                                       int32_t B, int32_t T, int32_t D, tavsr_stream_t stream) {
  TAVSR_REQUIRE(dwv && q && dpk, TAVSR_EINVAL, "fastattn_bwd_pool: null pointer");
  TAVSR_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && D >= 1 && (int64_t)B * T < (1ll << 31), TAVSR_EUNSUPPORTED,
                "fastattn_bwd_pool: 1 <= B <= 65535, B * T < 2^31");
  hipLaunchKernelGGL(fa_bwd_pool_kernel, dim3((D + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, dwv, lddwv, q, ldq, lens, dpk, T, D);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int64_t tavsr_fastattn_bwd_ws(int32_t B, int32_t T, int32_t D, int32_t H) {
  if (!fa_shape_ok(D, H) || B < 1 || T < 1) return 0;
  return (int64_t)B * fa_chunks(T) * fa_part_stride(D, H);
}

extern "C" int tavsr_fastattn_bwd_rows(int32_t is_k, const float* x, int64_t ldx, const float* cs, const float* w_pool, const float* dpool,
                                       const float* pool, const float* W, const int64_t* lens, const float* dres, int64_t lddres,
                                       const float* dwv, int64_t lddwv, const float* pk, float* dx, int64_t lddx, float* dWb,
                                       float* dcs, float* ws, int32_t B, int32_t T, int32_t D, int32_t H, tavsr_stream_t stream) {
  TAVSR_REQUIRE(x && w_pool && dpool && pool && W && dx && dWb && ws, TAVSR_EINVAL, "fastattn_bwd_rows: null pointer");
  TAVSR_REQUIRE(is_k ? (cs && dcs) : (dres && dwv && pk), TAVSR_EINVAL, "fastattn_bwd_rows: null pointer");
  FA_SHAPE_REQUIRE("fastattn_bwd_rows");
  TAVSR_REQUIRE(fa_rows_ok(x, ldx) && fa_rows_ok(dx, lddx) && fa_rows_ok(W, D) && fa_rows_ok(dpool, D) && fa_rows_ok(pool, D) &&
                    (is_k ? fa_rows_ok(cs, D) : (fa_rows_ok(dres, lddres) && fa_rows_ok(dwv, lddwv) && fa_rows_ok(pk, D))),
                TAVSR_EALIGN, "fastattn_bwd_rows: rows must start 16-byte aligned (strides multiples of 4)");
  const float scale = 1.f / sqrtf((float)(D / H));
  const int nchunk = fa_chunks(T);
  const int64_t ps = fa_part_stride(D, H);
  const dim3 grid(nchunk, B);
  hipStream_t s = (hipStream_t)stream;
#define FA_LAUNCH(NV, K)                                                                                                          \
  hipLaunchKernelGGL((fa_bwd_rows_kernel<NV, K>), grid, dim3(256), 0, s, x, ldx, cs, w_pool, dpool, pool, W, lens, dres, lddres, dwv, \
                     lddwv, pk, dx, lddx, ws, ps, T, D, H, scale)
  if (is_k) {
    if (D <= 256) FA_LAUNCH(1, true); else FA_LAUNCH(2, true);
  } else {
    if (D <= 256) FA_LAUNCH(1, false); else FA_LAUNCH(2, false);
  }
#undef FA_LAUNCH
  TAVSR_LAUNCH_CHECK();
  int rc = tavsr_sum_partials(ws, B * nchunk, ps, dWb, H * D + H, 0, stream);      // dW [H*D] | db [H]
  if (rc != TAVSR_OK) return rc;
  if (is_k) {
    hipLaunchKernelGGL(fa_sum_dcs_kernel, dim3((D + 255) / 256, B), dim3(256), 0, s, ws, ps, nchunk, (int64_t)H * D + H, dcs, D);
    TAVSR_LAUNCH_CHECK();
  }
  return TAVSR_OK;
}

extern "C" int tavsr_add_pe(const float* x, const float* pe, const float* alpha_dev, float xscale, float* y, int32_t B, int32_t T,
                            int32_t D, tavsr_stream_t stream) {
  TAVSR_REQUIRE(x && pe && y, TAVSR_EINVAL, "add_pe: null pointer");
  TAVSR_REQUIRE(B >= 1 && T >= 1 && D >= 1, TAVSR_EINVAL, "add_pe: empty shape");
  const int64_t TD = (int64_t)T * D, n = TD * B;
  hipLaunchKernelGGL(add_pe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, pe, alpha_dev, xscale, y, n, TD);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int64_t tavsr_add_pe_dalpha_ws(void) { return kPeBlocks; }

extern "C" int tavsr_add_pe_dalpha(const float* dy, const float* pe, float* dalpha, float* ws, int32_t B, int32_t T, int32_t D,
                                   tavsr_stream_t stream) {
  TAVSR_REQUIRE(dy && pe && dalpha && ws, TAVSR_EINVAL, "add_pe_dalpha: null pointer");
  TAVSR_REQUIRE(B >= 1 && T >= 1 && D >= 1, TAVSR_EINVAL, "add_pe_dalpha: empty shape");
  const int64_t TD = (int64_t)T * D;
  hipLaunchKernelGGL(add_pe_dalpha_kernel, dim3(kPeBlocks), dim3(256), 0, (hipStream_t)stream, dy, pe, TD * B, TD, ws);
  TAVSR_LAUNCH_CHECK();
  return tavsr_sum_partials(ws, kPeBlocks, 1, dalpha, 1, 0, stream);
}
