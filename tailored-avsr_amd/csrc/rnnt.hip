// Transducer (RNN-T) kernels: the LSTM recurrence of the prediction network (forward, backward, one-step form), the joint
// network's lattice rows reduced to three floats each, the alpha / beta lattice along anti-diagonals, the joint gradient, and
// the per-frame pick of the greedy search.  Contracts: include/tavsr.h.  The matrix products around them (x W_ih^T, lin_enc,
// lin_dec, z W_out^T and their gradients) are tavsr_gemm calls; nothing here reads a value on the host.
#include <float.h>
#include <math.h>

#include "seq.h"

namespace tavsr {

// ---------------------------------------------------------------------------------------------- LSTM
// Partition: a workgroup owns kLstmRows batch rows and all 4H gate columns for all steps; rows are independent, so workgroups
// never wait for each other.  Inside the workgroup (1024 threads) the reduction over k is cut into KS = lstm_slices(H) slices:
// thread (ks, j) accumulates slice ks of hidden unit j's four gate columns for all rows, the partial sums meet in LDS and the
// threads of slice 0 add them in slice order and do the gate arithmetic - the c / h update needs no further exchange.  h of the
// previous step is read from LDS as a broadcast.  W_hh is read transposed ([H][4H], built once per call by lstm_wt_kernel) so
// that a wave's loads are contiguous; every load feeds kLstmRows multiply-adds, which divides the weight stream by kLstmRows.
constexpr int kLstmRows = 4;
constexpr int kLstmMaxH = 1024;
constexpr int kLstmThreads = 1024;
constexpr int kLstmMaxSlices = 8;
constexpr int kLstmLdsBytes = 160 * 1024;

__host__ __device__ inline int lstm_slices(int H) {
  const int ks = kLstmThreads / H;
  return ks < 1 ? 1 : (ks > kLstmMaxSlices ? kLstmMaxSlices : ks);
}

__global__ void lstm_wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int H) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // wt[k][j] = w[j][k], j < 4H, k < H
  if (i >= (int64_t)4 * H * H) return;
  const int k = (int)(i / (4 * H)), j = (int)(i % (4 * H));
  wt[i] = w[(int64_t)j * H + k];
}

// xg [B][L][4H] (row stride ld_xg) = x W_ih^T.  Outputs (all nullable but hN / cN): y [B][L][H] (0 at padded steps), hprev
// [B][L][H] (the state a step started from), c_all [B][L][H], gates [B][L][4H] (activated i, f, g, o; 0 at padded steps).
__global__ __launch_bounds__(kLstmThreads) void lstm_fwd_kernel(const float* __restrict__ xg, int64_t ld_xg,
                                                                const float* __restrict__ wt, const float* __restrict__ b_ih,
                                                                const float* __restrict__ b_hh, const float* __restrict__ h0,
                                                                const float* __restrict__ c0, const int64_t* __restrict__ lens,
                                                                const uint8_t* __restrict__ mask, float* __restrict__ y,
                                                                float* __restrict__ hprev, float* __restrict__ c_all,
                                                                float* __restrict__ gates, float* __restrict__ hN,
                                                                float* __restrict__ cN, int B, int L, int H) {
  constexpr int R = kLstmRows;
  extern __shared__ float sm[];
  float* s_h = sm;                  // [2][R][H]
  float* s_c = sm + 2 * R * H;      // [R][H]
  float* s_p = sm + 3 * R * H;      // [KS][R * 4][H] partial sums of the k slices
  const int tid = threadIdx.x, b0 = blockIdx.x * R, nr = min(R, B - b0);
  const int KS = lstm_slices(H);
  const int j = tid % H, ks = tid / H;
  const bool slice = ks < KS, owner = tid < H;      // owner: slice 0's thread of unit j does the unit's gate arithmetic
  const int k0 = (int)((int64_t)ks * H / KS), k1 = (int)((int64_t)(ks + 1) * H / KS);
  for (int i = tid; i < R * H; i += kLstmThreads) {
    const int r = i / H, c = i - r * H;
    const bool in = r < nr;
    s_h[i] = (in && h0) ? h0[(int64_t)(b0 + r) * H + c] : 0.f;
    s_h[R * H + i] = 0.f;      // (rows past the batch stay 0 in both buffers)
    s_c[i] = (in && c0) ? c0[(int64_t)(b0 + r) * H + c] : 0.f;
  }
  int64_t len[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    len[r] = 0;
    if (r < nr) {
      len[r] = lens ? lens[b0 + r] : (int64_t)L;
      if (mask && !mask[b0 + r]) len[r] = 0;
    }
  }
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (owner) {
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = (b_ih ? b_ih[g * H + j] : 0.f) + (b_hh ? b_hh[g * H + j] : 0.f);
  }
  __syncthreads();
  const int H4 = 4 * H;
  for (int t = 0; t < L; ++t) {
    const float* hc = s_h + (t & 1) * R * H;
    float* hn = s_h + ((t + 1) & 1) * R * H;
    float base[R][4];      // the input product and the biases: loaded ahead of the k loop, used behind it
    if (owner) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) base[r][g] = r < nr ? xg[((int64_t)(b0 + r) * L + t) * ld_xg + g * H + j] + bias[g] : 0.f;
    }
    if (slice) {
      float a[R][4];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r][0] = a[r][1] = a[r][2] = a[r][3] = 0.f;
#pragma unroll 4
      for (int k = k0; k < k1; ++k) {
        const float* wr = wt + (int64_t)k * H4 + j;
        const float w0 = wr[0], w1 = wr[H], w2 = wr[2 * H], w3 = wr[3 * H];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float hv = hc[r * H + k];
          a[r][0] = fmaf(hv, w0, a[r][0]);
          a[r][1] = fmaf(hv, w1, a[r][1]);
          a[r][2] = fmaf(hv, w2, a[r][2]);
          a[r][3] = fmaf(hv, w3, a[r][3]);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) s_p[((ks * R + r) * 4 + g) * H + j] = a[r][g];
    }
    __syncthreads();
    if (owner) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= nr) continue;
        float a[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          a[g] = base[r][g];
          for (int q = 0; q < KS; ++q) a[g] += s_p[((q * R + r) * 4 + g) * H + j];      // slice order: a fixed sum
        }
        const int64_t o = ((int64_t)(b0 + r) * L + t) * H + j;
        const float hp = hc[r * H + j], cp = s_c[r * H + j];
        if (hprev) hprev[o] = hp;
        if (t < len[r]) {
          const float ig = sigmoid_fast(a[0]), fg = sigmoid_fast(a[1]), gg = tanh_fast(a[2]), og = sigmoid_fast(a[3]);
          const float c = fmaf(fg, cp, ig * gg);
          const float h = og * tanh_fast(c);
          s_c[r * H + j] = c;
          hn[r * H + j] = h;
          if (y) y[o] = h;
          if (c_all) c_all[o] = c;
          if (gates) {
            float* gp = gates + ((int64_t)(b0 + r) * L + t) * H4 + j;
            gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
          }
        } else {
          hn[r * H + j] = hp;
          if (y) y[o] = 0.f;
          if (c_all) c_all[o] = cp;
          if (gates) {
            float* gp = gates + ((int64_t)(b0 + r) * L + t) * H4 + j;
            gp[0] = 0.f; gp[H] = 0.f; gp[2 * H] = 0.f; gp[3 * H] = 0.f;
          }
        }
      }
    }
    __syncthreads();
  }
  const float* hl = s_h + (L & 1) * R * H;
  for (int i = tid; i < nr * H; i += kLstmThreads) {
    const int r = i / H, c = i - r * H;
    hN[(int64_t)(b0 + r) * H + c] = hl[i];
    cN[(int64_t)(b0 + r) * H + c] = s_c[i];
  }
}

// the same partition walked backwards.  dgates [B][L][4H] (pre-activation gradients, 0 at padded steps) is the operand of the
// three GEMMs dx = dgates W_ih, dW_ih = dgates^T x, dW_hh = dgates^T hprev and of the bias column sums.  dh0 / dc0 [B][H].
// Per step: the threads of slice 0 form the gate gradients of their unit, then thread (js, k) sums slice js of the 4H gate
// columns of dgates W_hh for hidden unit k (W_hh in torch's layout: contiguous over k), and slice 0 adds the partial sums.
__global__ __launch_bounds__(kLstmThreads) void lstm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dhN,
                                                                const float* __restrict__ dcN, const float* __restrict__ w_hh,
                                                                const float* __restrict__ c0, const int64_t* __restrict__ lens,
                                                                const float* __restrict__ c_all, const float* __restrict__ gates,
                                                                float* __restrict__ dgates, float* __restrict__ dh0,
                                                                float* __restrict__ dc0, int B, int L, int H) {
  constexpr int R = kLstmRows;
  extern __shared__ float sm[];
  float* s_dg = sm;                   // [R][4H]
  float* s_dh = sm + R * 4 * H;       // [R][H]   gradient reaching h_t through the recurrence
  float* s_dc = s_dh + R * H;         // [R][H]
  float* s_p = s_dc + R * H;          // [KS][R][H]
  const int tid = threadIdx.x, b0 = blockIdx.x * R, nr = min(R, B - b0);
  const int H4 = 4 * H;
  const int KS = lstm_slices(H);
  const int j = tid % H, js = tid / H;
  const bool slice = js < KS, owner = tid < H;
  const int q0 = (int)((int64_t)js * H4 / KS), q1 = (int)((int64_t)(js + 1) * H4 / KS);
  for (int i = tid; i < R * H; i += kLstmThreads) {
    const int r = i / H, c = i - r * H;
    const bool in = r < nr;
    s_dh[i] = (in && dhN) ? dhN[(int64_t)(b0 + r) * H + c] : 0.f;
    s_dc[i] = (in && dcN) ? dcN[(int64_t)(b0 + r) * H + c] : 0.f;
  }
  int64_t len[R];
#pragma unroll
  for (int r = 0; r < R; ++r) len[r] = r < nr ? (lens ? lens[b0 + r] : (int64_t)L) : 0;
  __syncthreads();
  for (int t = L - 1; t >= 0; --t) {
    if (owner) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float di = 0.f, df = 0.f, dg = 0.f, dov = 0.f;
        if (r < nr && t < len[r]) {
          const int64_t o = ((int64_t)(b0 + r) * L + t) * H + j;
          const float* gp = gates + ((int64_t)(b0 + r) * L + t) * H4 + j;
          const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
          const float c = c_all[o];
          const float cp = t > 0 ? c_all[o - H] : (c0 ? c0[(int64_t)(b0 + r) * H + j] : 0.f);
          const float dh = (dy ? dy[o] : 0.f) + s_dh[r * H + j];
          const float tc = tanh_fast(c);
          const float dc = fmaf(dh * og, fmaf(-tc, tc, 1.f), s_dc[r * H + j]);
          dov = dh * tc * og * (1.f - og);
          di = dc * gg * ig * (1.f - ig);
          df = dc * cp * fg * (1.f - fg);
          dg = dc * ig * fmaf(-gg, gg, 1.f);
          s_dc[r * H + j] = dc * fg;
        }
        s_dg[r * H4 + j] = di; s_dg[r * H4 + H + j] = df; s_dg[r * H4 + 2 * H + j] = dg; s_dg[r * H4 + 3 * H + j] = dov;
        if (r < nr) {
          float* dp = dgates + ((int64_t)(b0 + r) * L + t) * H4 + j;
          dp[0] = di; dp[H] = df; dp[2 * H] = dg; dp[3 * H] = dov;
        }
      }
    }
    __syncthreads();
    if (slice) {
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 8
      for (int q = q0; q < q1; ++q) {
        const float w = w_hh[(int64_t)q * H + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(s_dg[r * H4 + q], w, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) s_p[(js * R + r) * H + j] = acc[r];
    }
    __syncthreads();
    if (owner) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < nr && t < len[r]) {
          float acc = 0.f;
          for (int q = 0; q < KS; ++q) acc += s_p[(q * R + r) * H + j];      // slice order: a fixed sum
          s_dh[r * H + j] = acc;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nr * H; i += kLstmThreads) {
    const int r = i / H, c = i - r * H;
    if (dh0) dh0[(int64_t)(b0 + r) * H + c] = s_dh[i];
    if (dc0) dc0[(int64_t)(b0 + r) * H + c] = s_dc[i];
  }
}

// ---------------------------------------------------------------------------------------------- joint rows
// Lattice row n = (b * T + t) * U1 + u.  A row is live when t < tlens[b] and u <= ulens[b].
__device__ __forceinline__ bool rnnt_row(int64_t n, int T, int U1, const int64_t* tlens, const int64_t* ulens, int& b, int& t,
                                         int& u) {
  u = (int)(n % U1);
  const int64_t bt = n / U1;
  t = (int)(bt % T);
  b = (int)(bt / T);
  return t < tlens[b] && u <= ulens[b] && u < U1;
}

// out[r][:] = r < lens[b] + extra ? x[r][:] : 0      (the joint never multiplies a padded row: its content may be anything)
__global__ void rnnt_mask_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens, int extra,
                                      float* __restrict__ out, int64_t total, int Tn, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / D;
  const int b = (int)(row / Tn), t = (int)(row % Tn);
  out[i] = t < lens[b] + extra ? x[i] : 0.f;
}

// z[i][:] = tanh(e[b][t][:] + d[b][u][:]) for the rows n0 + i of a chunk; dead rows are 0
__global__ void rnnt_z_kernel(const float* __restrict__ e, const float* __restrict__ d, const int64_t* __restrict__ tlens,
                              const int64_t* __restrict__ ulens, float* __restrict__ z, int64_t n0, int nrows, int T, int U1,
                              int J) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nrows * J) return;
  const int row = (int)(i / J), c = (int)(i % J);
  int b, t, u;
  float v = 0.f;
  if (rnnt_row(n0 + row, T, U1, tlens, ulens, b, t, u))
    v = tanh_fast(e[((int64_t)b * T + t) * J + c] + d[((int64_t)b * U1 + u) * J + c]);
  z[i] = v;
}

// one wave per row of a chunk's logits: logsumexp, lp_blank, lp_label (label y[b][u], absent at u == ulens[b]: 0 is stored)
__global__ __launch_bounds__(256) void rnnt_rows_kernel(const float* __restrict__ logits, int64_t ldv,
                                                        const int32_t* __restrict__ y, int64_t ld_y,
                                                        const int64_t* __restrict__ tlens, const int64_t* __restrict__ ulens,
                                                        int blank, float* __restrict__ lse, float* __restrict__ lp_blank,
                                                        float* __restrict__ lp_label, int64_t n0, int nrows, int T, int U1, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int64_t n = n0 + row;
  int b, t, u;
  if (!rnnt_row(n, T, U1, tlens, ulens, b, t, u)) {
    if (lane == 0) { lse[n] = 0.f; lp_blank[n] = 0.f; lp_label[n] = 0.f; }
    return;
  }
  const float* x = logits + (int64_t)row * ldv;
  float mx = -FLT_MAX;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(x[v] - mx);
  se = wave_sum(se);
  if (lane == 0) {
    const float lz = mx + logf(se);
    lse[n] = lz;
    lp_blank[n] = x[blank] - lz;
    float ll = 0.f;
    if (u < ulens[b] && u < U1 - 1) {
      const int lab = y[(int64_t)b * ld_y + u];
      if (lab >= 0 && lab < V) ll = x[lab] - lz;
    }
    lp_label[n] = ll;
  }
}

// G[row][v] = scale * (occ * softmax - [v == blank] p_blank - [v == label] p_label), in place over the chunk's logits;
// scale = gscale[0] * inv_b (the upstream gradient is device data)
__global__ __launch_bounds__(256) void rnnt_g_kernel(float* __restrict__ logits, int64_t ldv, const int32_t* __restrict__ y,
                                                     int64_t ld_y, const int64_t* __restrict__ tlens,
                                                     const int64_t* __restrict__ ulens, int blank, const float* __restrict__ lse,
                                                     const float* __restrict__ occ, const float* __restrict__ p_blank,
                                                     const float* __restrict__ p_label, const float* __restrict__ gscale,
                                                     float inv_b, int64_t n0, int nrows, int T, int U1, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int64_t n = n0 + row;
  float* x = logits + (int64_t)row * ldv;
  int b, t, u;
  if (!rnnt_row(n, T, U1, tlens, ulens, b, t, u)) {
    for (int v = lane; v < ldv; v += 64) x[v] = 0.f;
    return;
  }
  const float scale = (gscale ? gscale[0] : 1.f) * inv_b;
  const float lz = lse[n], oc = occ[n], pb = p_blank[n], pl = p_label[n];
  int lab = -1;
  if (u < ulens[b] && u < U1 - 1) lab = y[(int64_t)b * ld_y + u];
  for (int v = lane; v < V; v += 64) {
    float g = oc * expf(x[v] - lz);
    if (v == blank) g -= pb;
    if (v == lab) g -= pl;
    x[v] = scale * g;
  }
  for (int v = V + lane; v < ldv; v += 64) x[v] = 0.f;
}

// dz *= 1 - z^2 for a chunk, in place
__global__ void rnnt_dtanh_kernel(float* __restrict__ dz, const float* __restrict__ z, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float zz = z[i];
  dz[i] *= fmaf(-zz, zz, 1.f);
}

// de[b][t][:] += sum over the chunk's rows of that (b, t) in u order: one workgroup per (b, t) the chunk touches.  Every
// element has one owner per launch and the launches of the chunks are ordered: no atomics, a fixed order.
__global__ void rnnt_de_kernel(const float* __restrict__ dz, float* __restrict__ de, int64_t n0, int nrows, int U1, int J) {
  const int64_t bt = n0 / U1 + blockIdx.x;
  const int64_t lo = max(n0, bt * U1), hi = min(n0 + nrows, (bt + 1) * U1);
  for (int c = threadIdx.x; c < J; c += blockDim.x) {
    float acc = 0.f;
    for (int64_t n = lo; n < hi; ++n) acc += dz[(n - n0) * J + c];
    de[bt * J + c] += acc;
  }
}

// dd[b][u][:] += sum over the chunk's rows of that (b, u) in t order: one workgroup per (b, u)
__global__ void rnnt_dd_kernel(const float* __restrict__ dz, float* __restrict__ dd, int64_t n0, int nrows, int T, int U1, int J) {
  const int b = blockIdx.x / U1, u = blockIdx.x % U1;
  const int64_t first = ((int64_t)b * T) * U1 + u;                       // row of t = 0
  int64_t t_lo = n0 <= first ? 0 : (n0 - first + U1 - 1) / U1;
  int64_t t_hi = n0 + nrows <= first ? 0 : (n0 + nrows - first + U1 - 1) / U1;      // exclusive
  if (t_hi > T) t_hi = T;
  if (t_lo >= t_hi) return;
  for (int c = threadIdx.x; c < J; c += blockDim.x) {
    float acc = 0.f;
    for (int64_t t = t_lo; t < t_hi; ++t) acc += dz[(first + t * U1 - n0) * J + c];
    dd[((int64_t)b * U1 + u) * J + c] += acc;
  }
}

__global__ void rnnt_acc_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// ---------------------------------------------------------------------------------------------- lattice
// alpha and beta are sums of up to T + U log-probabilities: at U = 129 they reach ~400, where one fp32 rounding is 3e-5 and a
// hundred of them miss the 1e-4 bar of the coefficients exp(alpha + beta - ll).  The sums are kept in fp64 (adds only); the
// bounded correction term log1p(exp(-|a - b|)) <= log 2 and the final exponentials run in fp32 on differences formed in fp64.
__device__ __forceinline__ double rnnt_log_add(double a, double b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const double m = a > b ? a : b;
  return m + (double)log1pf(expf(-(float)fabs(a - b)));
}

constexpr int kLatticeLdsBytes = 160 * 1024;

// alpha / beta [T][U1] of utterance b, in LDS or in the caller's workspace: one body, the same arithmetic either way.
// alpha[t][u] = logadd(alpha[t-1][u] + lpb[t-1][u], alpha[t][u-1] + lpl[t][u-1]), beta mirrored; the alpha step of
// anti-diagonal d and the beta step of the mirrored one share a barrier.
__device__ __forceinline__ void rnnt_lattice_body(const float* __restrict__ lpb, const float* __restrict__ lpl, int Tb, int Ub,
                                                  int U1, double* alpha, double* beta, float* __restrict__ nll,
                                                  float* __restrict__ occ, float* __restrict__ p_blank,
                                                  float* __restrict__ p_label, int T) {
  const int tid = threadIdx.x;
  if (Tb <= 0) {
    if (tid == 0) *nll = 0.f;
    for (int i = tid; i < T * U1; i += 256) { occ[i] = 0.f; p_blank[i] = 0.f; p_label[i] = 0.f; }
    return;
  }
  const double ninf = -INFINITY;
  const int nd = Tb + Ub;      // anti-diagonals 0 .. nd - 1
  for (int dg = 0; dg < nd; ++dg) {
    for (int u = tid; u <= Ub; u += 256) {
      const int t = dg - u;
      if (t >= 0 && t < Tb) {
        double a;
        if (t == 0 && u == 0) {
          a = 0.0;
        } else {
          const double up = t > 0 ? alpha[(t - 1) * U1 + u] + (double)lpb[(t - 1) * U1 + u] : ninf;
          const double left = u > 0 ? alpha[t * U1 + u - 1] + (double)lpl[t * U1 + u - 1] : ninf;
          a = rnnt_log_add(up, left);
        }
        alpha[t * U1 + u] = a;
      }
      const int tb = (nd - 1 - dg) - u;      // the mirrored diagonal
      if (tb >= 0 && tb < Tb) {
        double bt;
        if (tb == Tb - 1 && u == Ub) {
          bt = (double)lpb[tb * U1 + u];
        } else {
          const double down = tb + 1 < Tb ? beta[(tb + 1) * U1 + u] + (double)lpb[tb * U1 + u] : ninf;
          const double right = u < Ub ? beta[tb * U1 + u + 1] + (double)lpl[tb * U1 + u] : ninf;
          bt = rnnt_log_add(down, right);
        }
        beta[tb * U1 + u] = bt;
      }
    }
    __syncthreads();
  }
  const double ll = alpha[(Tb - 1) * U1 + Ub] + (double)lpb[(Tb - 1) * U1 + Ub];
  if (tid == 0) *nll = (float)-ll;
  for (int i = tid; i < T * U1; i += 256) {
    const int t = i / U1, u = i - t * U1;
    float oc = 0.f, pb = 0.f, pl = 0.f;
    if (t < Tb && u <= Ub) {
      const double a = alpha[i];
      oc = expf((float)(a + beta[i] - ll));
      if (t + 1 < Tb) pb = expf((float)(a + (double)lpb[i] + beta[i + U1] - ll));
      else if (u == Ub) pb = expf((float)(a + (double)lpb[i] - ll));
      if (u < Ub) pl = expf((float)(a + (double)lpl[i] + beta[i + 1] - ll));
    }
    occ[i] = oc; p_blank[i] = pb; p_label[i] = pl;
  }
}

__device__ __forceinline__ void rnnt_lattice_lens(const int64_t* tlens, const int64_t* ulens, int b, int T, int U1, int& Tb, int& Ub) {
  const int64_t tl = tlens[b], ul = ulens[b];
  Tb = (int)(tl < 0 ? 0 : (tl < T ? tl : T));
  Ub = (int)(ul < 0 ? 0 : (ul < U1 - 1 ? ul : U1 - 1));
}

__global__ __launch_bounds__(256) void rnnt_lattice_lds_kernel(const float* __restrict__ lp_blank, const float* __restrict__ lp_label,
                                                               const int64_t* __restrict__ tlens, const int64_t* __restrict__ ulens,
                                                               float* __restrict__ nll, float* __restrict__ occ,
                                                               float* __restrict__ p_blank, float* __restrict__ p_label, int T, int U1) {
  extern __shared__ double smd[];
  const int b = blockIdx.x;
  const int64_t o = (int64_t)b * T * U1;
  int Tb, Ub;
  rnnt_lattice_lens(tlens, ulens, b, T, U1, Tb, Ub);
  rnnt_lattice_body(lp_blank + o, lp_label + o, Tb, Ub, U1, smd, smd + (int64_t)T * U1, nll + b, occ + o, p_blank + o, p_label + o, T);
}

__global__ __launch_bounds__(256) void rnnt_lattice_ws_kernel(const float* __restrict__ lp_blank, const float* __restrict__ lp_label,
                                                              const int64_t* __restrict__ tlens, const int64_t* __restrict__ ulens,
                                                              float* __restrict__ nll, float* __restrict__ occ,
                                                              float* __restrict__ p_blank, float* __restrict__ p_label, double* ws,
                                                              int T, int U1) {
  const int b = blockIdx.x;
  const int64_t o = (int64_t)b * T * U1;
  int Tb, Ub;
  rnnt_lattice_lens(tlens, ulens, b, T, U1, Tb, Ub);
  rnnt_lattice_body(lp_blank + o, lp_label + o, Tb, Ub, U1, ws + 2 * o, ws + 2 * o + (int64_t)T * U1, nll + b, occ + o, p_blank + o,
                    p_label + o, T);
}

// ---------------------------------------------------------------------------------------------- greedy search
// z[b][:] = tanh(e[b][min(frame, T - 1)][:] + d[b][:]) for the frame in device memory
__global__ void rnnt_frame_z_kernel(const float* __restrict__ e, const float* __restrict__ d, const int32_t* __restrict__ frame,
                                    float* __restrict__ z, int B, int T, int J) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * J) return;
  const int b = i / J, c = i - b * J;
  const int t = min(max(*frame, 0), T - 1);
  z[i] = tanh_fast(e[((int64_t)b * T + t) * J + c] + d[i]);
}

// One workgroup, a wave per utterance in turn: log-softmax and argmax (lowest index on ties) of its logits row at the current
// frame.  Where the frame is inside the utterance and the argmax is not blank: append it, add its log-probability, commit = 1
// and tok = argmax; else commit = 0.  The last thing the launch does is frame += 1.
__global__ __launch_bounds__(256) void rnnt_greedy_pick_kernel(const float* __restrict__ logits, int64_t ldv,
                                                               const int64_t* __restrict__ tlens, int blank, int32_t* frame,
                                                               int64_t* __restrict__ tok, uint8_t* __restrict__ commit,
                                                               int64_t* __restrict__ hyp, int64_t ld_hyp, int32_t* __restrict__ hyp_len,
                                                               float* __restrict__ score, int B, int V) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t = *frame;
  for (int b = wv; b < B; b += 4) {
    const float* x = logits + (int64_t)b * ldv;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float xv = x[v];
      if (bi == 0x7fffffff || xv > best) { best = xv; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    float se = 0.f;
    for (int v = lane; v < V; v += 64) se += expf(x[v] - best);
    se = wave_sum(se);
    if (lane == 0) {
      const bool take = t < tlens[b] && bi != blank && hyp_len[b] < ld_hyp;
      commit[b] = take ? 1 : 0;
      if (take) {
        hyp[(int64_t)b * ld_hyp + hyp_len[b]] = bi;
        hyp_len[b] += 1;
        score[b] += -logf(se);
        tok[b] = bi;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *frame = t + 1;
}

static bool lstm_sizes_ok(int64_t B, int64_t L, int64_t H) { return B >= 0 && L >= 0 && H > 0 && H % 4 == 0 && H <= kLstmMaxH; }

static int lstm_lds_optin(const void* fn, size_t bytes, const char* what) {
  TAVSR_REQUIRE(bytes <= (size_t)kLstmLdsBytes, TAVSR_EUNSUPPORTED, "%s: %zu bytes of LDS exceed a workgroup's %d", what, bytes, kLstmLdsBytes);
  if (bytes > 48 * 1024) {      // the > 64 KB dynamic-LDS opt-in, as tavsr_ctc_align
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLstmLdsBytes);
    TAVSR_REQUIRE(e == hipSuccess, TAVSR_EUNSUPPORTED, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
  }
  return TAVSR_OK;
}

static int lstm_launch_fwd(const float* xg, int64_t ld_xg, const float* w_hh_t, const float* b_ih, const float* b_hh, const float* h0,
                           const float* c0, const int64_t* lens, const uint8_t* mask, float* y, float* hprev, float* c_all,
                           float* gates, float* hN, float* cN, int B, int L, int H, hipStream_t s) {
  const size_t lds = ((size_t)3 * kLstmRows * H + (size_t)lstm_slices(H) * kLstmRows * 4 * H) * sizeof(float);
  const int rc = lstm_lds_optin(reinterpret_cast<const void*>(lstm_fwd_kernel), lds, "lstm_fwd");
  if (rc != TAVSR_OK) return rc;
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(cdiv(B, kLstmRows)), dim3(kLstmThreads), lds, s, xg, ld_xg, w_hh_t, b_ih, b_hh, h0, c0, lens, mask,
                     y, hprev, c_all, gates, hN, cN, B, L, H);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_lstm_rows_per_wg(void) { return kLstmRows; }

extern "C" int tavsr_lstm_wt(const float* w_hh, float* w_hh_t, int32_t H, tavsr_stream_t stream) {
  TAVSR_REQUIRE(w_hh && w_hh_t, TAVSR_EINVAL, "lstm_wt: null pointer");
  TAVSR_REQUIRE(lstm_sizes_ok(0, 0, H), TAVSR_EUNSUPPORTED, "lstm: H=%d must be a multiple of 4 and <= %d", H, kLstmMaxH);
  hipLaunchKernelGGL(lstm_wt_kernel, dim3(cdiv((int64_t)4 * H * H, 256)), dim3(256), 0, (hipStream_t)stream, w_hh, w_hh_t, H);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_lstm_fwd(const float* xg, int64_t ld_xg, const float* w_hh_t, const float* b_ih, const float* b_hh,
                              const float* h0, const float* c0, const int64_t* lens, float* y, float* hprev, float* c_all,
                              float* gates, float* hN, float* cN, int32_t B, int32_t L, int32_t H, tavsr_stream_t stream) {
  TAVSR_REQUIRE(lstm_sizes_ok(B, L, H), TAVSR_EUNSUPPORTED, "lstm_fwd: H=%d must be a multiple of 4 and <= %d (B=%d L=%d)", H, kLstmMaxH, B, L);
  if (B == 0) return TAVSR_OK;
  TAVSR_REQUIRE(w_hh_t && hN && cN && (L == 0 || xg), TAVSR_EINVAL, "lstm_fwd: null pointer");
  TAVSR_REQUIRE(ld_xg >= 4 * (int64_t)H, TAVSR_EINVAL, "lstm_fwd: ld_xg=%lld < 4H", (long long)ld_xg);
  return lstm_launch_fwd(xg, ld_xg, w_hh_t, b_ih, b_hh, h0, c0, lens, nullptr, y, hprev, c_all, gates, hN, cN, B, L, H, (hipStream_t)stream);
}

extern "C" int tavsr_lstm_step(const float* xg, int64_t ld_xg, const float* w_hh_t, const float* b_ih, const float* b_hh,
                               const float* h_in, const float* c_in, const uint8_t* commit, float* h_out, float* c_out, int32_t N,
                               int32_t H, tavsr_stream_t stream) {
  TAVSR_REQUIRE(lstm_sizes_ok(N, 1, H), TAVSR_EUNSUPPORTED, "lstm_step: H=%d must be a multiple of 4 and <= %d (N=%d)", H, kLstmMaxH, N);
  if (N == 0) return TAVSR_OK;
  TAVSR_REQUIRE(xg && w_hh_t && h_out && c_out, TAVSR_EINVAL, "lstm_step: null pointer");
  TAVSR_REQUIRE(ld_xg >= 4 * (int64_t)H, TAVSR_EINVAL, "lstm_step: ld_xg=%lld < 4H", (long long)ld_xg);
  return lstm_launch_fwd(xg, ld_xg, w_hh_t, b_ih, b_hh, h_in, c_in, nullptr, commit, nullptr, nullptr, nullptr, nullptr, h_out, c_out,
                         N, 1, H, (hipStream_t)stream);
}

extern "C" int tavsr_lstm_bwd(const float* dy, const float* dhN, const float* dcN, const float* w_hh, const float* c0,
                              const int64_t* lens, const float* c_all, const float* gates, float* dgates, float* dh0, float* dc0,
                              int32_t B, int32_t L, int32_t H, tavsr_stream_t stream) {
  TAVSR_REQUIRE(lstm_sizes_ok(B, L, H), TAVSR_EUNSUPPORTED, "lstm_bwd: H=%d must be a multiple of 4 and <= %d (B=%d L=%d)", H, kLstmMaxH, B, L);
  if (B == 0) return TAVSR_OK;
  TAVSR_REQUIRE(w_hh && (L == 0 || (c_all && gates && dgates)), TAVSR_EINVAL, "lstm_bwd: null pointer");
  const size_t lds = ((size_t)6 * kLstmRows * H + (size_t)lstm_slices(H) * kLstmRows * H) * sizeof(float);
  const int rc = lstm_lds_optin(reinterpret_cast<const void*>(lstm_bwd_kernel), lds, "lstm_bwd");
  if (rc != TAVSR_OK) return rc;
  hipLaunchKernelGGL(lstm_bwd_kernel, dim3(cdiv(B, kLstmRows)), dim3(kLstmThreads), lds, (hipStream_t)stream, dy, dhN, dcN, w_hh, c0, lens, c_all,
                     gates, dgates, dh0, dc0, B, L, H);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_mask_rows(const float* x, const int64_t* lens, int32_t extra, float* out, int32_t B, int32_t Tn, int32_t D,
                                    tavsr_stream_t stream) {
  const int64_t total = (int64_t)B * Tn * D;
  if (total <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(x && lens && out, TAVSR_EINVAL, "rnnt_mask_rows: null pointer");
  hipLaunchKernelGGL(rnnt_mask_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, lens, extra, out, total, Tn, D);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

static int64_t pad4(int64_t v) { return (v + 3) / 4 * 4; }
static bool rnnt_sizes_ok(int64_t B, int64_t T, int64_t U1, int64_t J, int64_t V, int64_t chunk) {
  return B > 0 && T > 0 && U1 > 0 && J > 0 && V > 0 && chunk > 0 && B * T * U1 < ((int64_t)1 << 31) && chunk * pad4(V) < ((int64_t)1 << 31) &&
         chunk * J < ((int64_t)1 << 31);
}

// floats: z [chunk][J] | logits / G [chunk][pad4(V)] | dz [chunk][J] | dW_out part [V][J] | db_out part [V] (each rounded to 64)
struct RnntWs { int64_t z, lg, dz, dw, db, words; };
static RnntWs rnnt_ws_layout(int64_t J, int64_t V, int64_t chunk, bool grad) {
  auto r64 = [](int64_t n) { return (n + 63) / 64 * 64; };
  RnntWs o;
  o.z = 0;
  o.lg = o.z + r64(chunk * J);
  o.dz = o.lg + r64(chunk * pad4(V));
  o.dw = o.dz + (grad ? r64(chunk * J) : 0);
  o.db = o.dw + (grad ? r64(V * J) : 0);
  o.words = o.db + (grad ? r64(V) : 0);
  return o;
}

extern "C" int64_t tavsr_rnnt_ws(int32_t B, int32_t T, int32_t U1, int32_t J, int32_t V, int32_t chunk, int32_t grad) {
  if (!rnnt_sizes_ok(B, T, U1, J, V, chunk)) return 0;
  const int64_t rows = (int64_t)B * T * U1;
  return rnnt_ws_layout(J, V, chunk < rows ? chunk : rows, grad != 0).words;
}

static int rnnt_chunk_logits(const float* e, const float* d, const float* w_out, const float* b_out, const int64_t* tlens,
                             const int64_t* ulens, float* z, float* lg, int64_t n0, int nrows, int T, int U1, int J, int V,
                             hipStream_t s) {
  hipLaunchKernelGGL(rnnt_z_kernel, dim3(cdiv((int64_t)nrows * J, 256)), dim3(256), 0, s, e, d, tlens, ulens, z, n0, nrows, T, U1, J);
  TAVSR_LAUNCH_CHECK();
  tavsr_gemm_desc g = seq::lin(nrows, V, J, z, J, w_out, b_out, lg, pad4(V));
  return tavsr_gemm(&g, (tavsr_stream_t)s);
}

extern "C" int tavsr_rnnt_joint_rows(const float* e, const float* d, const float* w_out, const float* b_out, const int32_t* y,
                                     int64_t ld_y, const int64_t* tlens, const int64_t* ulens, int32_t blank, float* lse,
                                     float* lp_blank, float* lp_label, float* ws, int32_t B, int32_t T, int32_t U1, int32_t J,
                                     int32_t V, int32_t chunk, tavsr_stream_t stream) {
  if (B <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(e && d && w_out && tlens && ulens && lse && lp_blank && lp_label && ws && (U1 == 1 || y), TAVSR_EINVAL,
                "rnnt_joint_rows: null pointer");
  TAVSR_REQUIRE(rnnt_sizes_ok(B, T, U1, J, V, chunk) && blank >= 0 && blank < V && ld_y >= U1 - 1, TAVSR_EINVAL,
                "rnnt_joint_rows: bad sizes (B=%d T=%d U1=%d J=%d V=%d chunk=%d blank=%d)", B, T, U1, J, V, chunk, blank);
  const int64_t rows = (int64_t)B * T * U1;
  const int64_t ch = chunk < rows ? chunk : rows;
  const RnntWs o = rnnt_ws_layout(J, V, ch, false);
  for (int64_t n0 = 0; n0 < rows; n0 += ch) {
    const int nr = (int)(rows - n0 < ch ? rows - n0 : ch);
    const int rc = rnnt_chunk_logits(e, d, w_out, b_out, tlens, ulens, ws + o.z, ws + o.lg, n0, nr, T, U1, J, V, (hipStream_t)stream);
    if (rc != TAVSR_OK) return rc;
    hipLaunchKernelGGL(rnnt_rows_kernel, dim3(cdiv(nr, 4)), dim3(256), 0, (hipStream_t)stream, ws + o.lg, pad4(V), y, ld_y, tlens, ulens,
                       blank, lse, lp_blank, lp_label, n0, nr, T, U1, V);
    TAVSR_LAUNCH_CHECK();
  }
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_lattice_lds_ok(int32_t T, int32_t U1) {
  return T > 0 && U1 > 0 && (int64_t)2 * T * U1 * 8 <= kLatticeLdsBytes;
}

extern "C" int64_t tavsr_rnnt_lattice_ws(int32_t B, int32_t T, int32_t U1) {
  if (B <= 0 || T <= 0 || U1 <= 0) return 0;
  return (int64_t)4 * B * T * U1;      // two fp64 arrays, counted in floats
}

extern "C" int tavsr_rnnt_lattice(const float* lp_blank, const float* lp_label, const int64_t* tlens, const int64_t* ulens, float* nll,
                                  float* occ, float* p_blank, float* p_label, float* ws, int32_t B, int32_t T, int32_t U1,
                                  tavsr_stream_t stream) {
  if (B <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(lp_blank && lp_label && tlens && ulens && nll && occ && p_blank && p_label, TAVSR_EINVAL, "rnnt_lattice: null pointer");
  TAVSR_REQUIRE(T > 0 && U1 > 0 && (int64_t)B * T * U1 < ((int64_t)1 << 30), TAVSR_EINVAL, "rnnt_lattice: bad sizes (B=%d T=%d U1=%d)", B, T, U1);
  if (ws) {
    TAVSR_REQUIRE(((uintptr_t)ws & 7) == 0, TAVSR_EINVAL, "rnnt_lattice: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(rnnt_lattice_ws_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lp_blank, lp_label, tlens, ulens, nll, occ,
                       p_blank, p_label, reinterpret_cast<double*>(ws), T, U1);
  } else {
    TAVSR_REQUIRE(tavsr_rnnt_lattice_lds_ok(T, U1), TAVSR_EUNSUPPORTED,
                  "rnnt_lattice: alpha and beta of T=%d, U+1=%d do not fit a workgroup's LDS (tavsr_rnnt_lattice_lds_ok): pass a "
                  "workspace of tavsr_rnnt_lattice_ws floats", T, U1);
    const size_t lds = (size_t)2 * T * U1 * sizeof(double);
    const int rc = lstm_lds_optin(reinterpret_cast<const void*>(rnnt_lattice_lds_kernel), lds, "rnnt_lattice");
    if (rc != TAVSR_OK) return rc;
    hipLaunchKernelGGL(rnnt_lattice_lds_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, lp_blank, lp_label, tlens, ulens, nll, occ,
                       p_blank, p_label, T, U1);
  }
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_joint_grad(const float* e, const float* d, const float* w_out, const float* b_out, const int32_t* y,
                                     int64_t ld_y, const int64_t* tlens, const int64_t* ulens, int32_t blank, const float* lse,
                                     const float* occ, const float* p_blank, const float* p_label, const float* gscale, float inv_b,
                                     float* de, float* dd, float* dw_out, float* db_out, float* ws, int32_t B, int32_t T, int32_t U1,
                                     int32_t J, int32_t V, int32_t chunk, tavsr_stream_t stream) {
  if (B <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(e && d && w_out && tlens && ulens && lse && occ && p_blank && p_label && de && dd && dw_out && ws && (U1 == 1 || y),
                TAVSR_EINVAL, "rnnt_joint_grad: null pointer");
  TAVSR_REQUIRE(rnnt_sizes_ok(B, T, U1, J, V, chunk) && blank >= 0 && blank < V && ld_y >= U1 - 1, TAVSR_EINVAL,
                "rnnt_joint_grad: bad sizes (B=%d T=%d U1=%d J=%d V=%d chunk=%d blank=%d)", B, T, U1, J, V, chunk, blank);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * T * U1;
  const int64_t ch = chunk < rows ? chunk : rows;
  const RnntWs o = rnnt_ws_layout(J, V, ch, true);
  TAVSR_HIP_CHECK(hipMemsetAsync(de, 0, (size_t)B * T * J * sizeof(float), s));
  TAVSR_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)B * U1 * J * sizeof(float), s));
  TAVSR_HIP_CHECK(hipMemsetAsync(dw_out, 0, (size_t)V * J * sizeof(float), s));
  if (db_out) TAVSR_HIP_CHECK(hipMemsetAsync(db_out, 0, (size_t)V * sizeof(float), s));
  float *z = ws + o.z, *lg = ws + o.lg, *dz = ws + o.dz, *dwp = ws + o.dw, *dbp = ws + o.db;
  const int64_t ldv = pad4(V);
  for (int64_t n0 = 0; n0 < rows; n0 += ch) {
    const int nr = (int)(rows - n0 < ch ? rows - n0 : ch);
    int rc = rnnt_chunk_logits(e, d, w_out, b_out, tlens, ulens, z, lg, n0, nr, T, U1, J, V, s);
    if (rc != TAVSR_OK) return rc;
    hipLaunchKernelGGL(rnnt_g_kernel, dim3(cdiv(nr, 4)), dim3(256), 0, s, lg, ldv, y, ld_y, tlens, ulens, blank, lse, occ, p_blank,
                       p_label, gscale, inv_b, n0, nr, T, U1, V);
    TAVSR_LAUNCH_CHECK();
    // dz = G W_out  ([nr][V] x [V][J])
    tavsr_gemm_desc g;
    memset(&g, 0, sizeof g);
    g.M = nr; g.N = J; g.K = V; g.A = lg; g.lda = ldv; g.B = w_out; g.ldb = J; g.b_kmajor = 1; g.C = dz; g.ldc = J;
    g.nb1 = g.nb2 = 1; g.alpha = 1.f;
    rc = tavsr_gemm(&g, stream);
    if (rc != TAVSR_OK) return rc;
    // dW_out part = G^T z  ([V][nr] x [nr][J]), db_out part = column sums of G (the A operand's row sums)
    memset(&g, 0, sizeof g);
    g.M = V; g.N = J; g.K = nr; g.A = lg; g.lda = ldv; g.a_kmajor = 1; g.B = z; g.ldb = J; g.b_kmajor = 1; g.C = dwp; g.ldc = J;
    g.nb1 = g.nb2 = 1; g.alpha = 1.f;
    g.a_rowsum = db_out ? dbp : nullptr;
    rc = tavsr_gemm(&g, stream);
    if (rc != TAVSR_OK) return rc;
    hipLaunchKernelGGL(rnnt_acc_kernel, dim3(cdiv((int64_t)V * J, 256)), dim3(256), 0, s, dw_out, dwp, (int64_t)V * J);
    TAVSR_LAUNCH_CHECK();
    if (db_out) {
      hipLaunchKernelGGL(rnnt_acc_kernel, dim3(cdiv(V, 256)), dim3(256), 0, s, db_out, dbp, (int64_t)V);
      TAVSR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rnnt_dtanh_kernel, dim3(cdiv((int64_t)nr * J, 256)), dim3(256), 0, s, dz, z, (int64_t)nr * J);
    TAVSR_LAUNCH_CHECK();
    const int nbt = (int)((n0 + nr - 1) / U1 - n0 / U1 + 1);
    hipLaunchKernelGGL(rnnt_de_kernel, dim3(nbt), dim3(J < 256 ? 64 : 256), 0, s, dz, de, n0, nr, U1, J);
    TAVSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rnnt_dd_kernel, dim3(B * U1), dim3(J < 256 ? 64 : 256), 0, s, dz, dd, n0, nr, T, U1, J);
    TAVSR_LAUNCH_CHECK();
  }
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_frame_z(const float* e, const float* d, const int32_t* frame, float* z, int32_t B, int32_t T, int32_t J,
                                  tavsr_stream_t stream) {
  if (B <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(e && d && frame && z && T > 0 && J > 0, TAVSR_EINVAL, "rnnt_frame_z: null pointer or bad sizes");
  hipLaunchKernelGGL(rnnt_frame_z_kernel, dim3(cdiv((int64_t)B * J, 256)), dim3(256), 0, (hipStream_t)stream, e, d, frame, z, B, T, J);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_greedy_pick(const float* logits, int64_t ldv, const int64_t* tlens, int32_t blank, int32_t* frame,
                                      int64_t* tok, uint8_t* commit, int64_t* hyp, int64_t ld_hyp, int32_t* hyp_len, float* score,
                                      int32_t B, int32_t V, tavsr_stream_t stream) {
  if (B <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(logits && tlens && frame && tok && commit && hyp && hyp_len && score, TAVSR_EINVAL, "rnnt_greedy_pick: null pointer");
  TAVSR_REQUIRE(V > 0 && ldv >= V && blank >= 0 && blank < V && ld_hyp > 0, TAVSR_EINVAL, "rnnt_greedy_pick: bad sizes");
  hipLaunchKernelGGL(rnnt_greedy_pick_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, ldv, tlens, blank, frame, tok, commit,
                     hyp, ld_hyp, hyp_len, score, B, V);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
