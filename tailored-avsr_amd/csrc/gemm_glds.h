// Device code shared by the two GEMM translation units (gemm.hip: plain / tail / grouped products and the host entry points;
// gemm_conv.hip: implicit convolutions and the Conv3d stem): the launch arguments, the register-staged loader, both epilogues,
// the LDS-DMA loader, the operand-source interface with the plain source, and the LDS-DMA kernel's ring (glds_tile).
// The library is built without relocatable device code: everything here is a template, inline or static, and a __device__
// variable stays in the unit that uses it.
#pragma once
#include <type_traits>

#include "common.h"

namespace tavsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kBK = 32;      // K-step of the LDS-DMA kernels

struct GemmArgs {
  tavsr_gemm_desc d;
  int kchunk;     // K elements per split (multiple of BK)
  int nsplit;
  int tiles_m, tiles_n;
  int vec_epi;    // LDS-DMA kernels: epilogue through LDS with 16-byte row accesses (finish_tile_vec)
  int zmap;       // split-K convolution weight gradients: all tiles of a K slice on one XCD (see gemm_glds_kernel)
  int n_big, kunit;   // position-major weight gradient, two slice lengths (plan_conv): slices z < n_big hold kchunk + kunit
};

template <int ROWS, int BK, bool KMAJOR>
struct Tile {
  static constexpr int LD = KMAJOR ? (ROWS + 4) : (BK + 4);
  static constexpr int SIZE = KMAJOR ? BK * LD : ROWS * LD;
};

// Global -> register -> LDS staging of one ROWS x BK operand tile (NV float4 per thread).
template <int ROWS, int BK, bool KMAJOR, bool VEC, int NT>
struct Loader {
  static constexpr int NV = ROWS * BK / 4 / NT;
  static_assert(ROWS * BK % (4 * NT) == 0, "tile must divide over the block");
  static constexpr int VPL = KMAJOR ? ROWS / 4 : BK / 4;   // float4 per contiguous line
  using T = Tile<ROWS, BK, KMAJOR>;

  // vector v covers 4 consecutive elements along the contiguous direction
  __device__ static __forceinline__ void coords(int v, int& row, int& k) {
    if (KMAJOR) {
      k = v / VPL;
      row = (v % VPL) * 4;
    } else {
      row = v / VPL;
      k = (v % VPL) * 4;
    }
  }
  // element offsets of this thread's vectors relative to (row0, k = 0); rows are clamped for the
  // k-contiguous layout (the epilogue never stores rows >= nrows, so what they hold is irrelevant)
  __device__ static __forceinline__ void offsets(int64_t ld, int row0, int nrows, int tid, int64_t (&off)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int row, k;
      coords(tid + i * NT, row, k);
      if (KMAJOR)
        off[i] = (int64_t)k * ld + row0 + row;
      else
        off[i] = (int64_t)min(row0 + row, nrows - 1) * ld + k;
    }
  }
  __device__ static __forceinline__ void load_fast(const float* __restrict__ g, const int64_t (&off)[NV],
                                                   float4 (&r)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) r[i] = *reinterpret_cast<const float4*>(g + off[i]);
  }
  // fully predicated (edge tiles, K tails, unaligned operands): zero fill outside [nrows) x [K)
  __device__ static __forceinline__ void load_safe(const float* __restrict__ g, int64_t ld, int row0, int k0,
                                                   int nrows, int K, int tid, float4 (&r)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int row, k;
      coords(tid + i * NT, row, k);
      int gr = row0 + row, gk = k0 + k;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (KMAJOR) {
        if (gk < K) {
          const float* p = g + (int64_t)gk * ld + gr;
          if (VEC && gr + 3 < nrows) {
            val = *reinterpret_cast<const float4*>(p);
          } else {
            if (gr + 0 < nrows) val.x = p[0];
            if (gr + 1 < nrows) val.y = p[1];
            if (gr + 2 < nrows) val.z = p[2];
            if (gr + 3 < nrows) val.w = p[3];
          }
        }
      } else {
        if (gr < nrows) {
          const float* p = g + (int64_t)gr * ld + gk;
          if (VEC && gk + 3 < K) {
            val = *reinterpret_cast<const float4*>(p);
          } else {
            if (gk + 0 < K) val.x = p[0];
            if (gk + 1 < K) val.y = p[1];
            if (gk + 2 < K) val.z = p[2];
            if (gk + 3 < K) val.w = p[3];
          }
        }
      }
      r[i] = val;
    }
  }
  __device__ static __forceinline__ void store(float* __restrict__ s, int tid, const float4 (&r)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int row, k;
      coords(tid + i * NT, row, k);
      *reinterpret_cast<float4*>(s + (KMAJOR ? k * T::LD + row : row * T::LD + k)) = r[i];
    }
  }
};

// Fragments of one 32-row sub-tile for k-group g (8 k values): f[j] is the operand of MFMA j, k = 8g+4h+j.
template <int ROWS, int BK, bool KMAJOR>
__device__ __forceinline__ void read_frag(const float* __restrict__ s, int row, int g, int lk, float (&f)[4]) {
  using T = Tile<ROWS, BK, KMAJOR>;
  if (KMAJOR) {
    const float* p = s + (g * 8 + 4 * lk) * T::LD + row;
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = p[j * T::LD];
  } else {
    const float4 v = *reinterpret_cast<const float4*>(s + row * T::LD + g * 8 + 4 * lk);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
}

// Position-major virtual rows of an implicit 3x3 / pad 1 convolution (tavsr_gemm_desc.conv_posmajor): virtual row
// r = v * n + image, where v counts the H x W pixel positions of the OUTPUT map interior first (at stride 1: 9 taps inside the
// image), then the edges (6), then the corners (4).  A tile whose rows share one position (uni) maps its rows without a division.
// Stride st = 2: output position (y, x) is centred on input pixel (2 y, 2 x) of the HI x WI input map, so the first row / column
// always loses its upper / left taps and the last one its lower / right taps only where the input size is odd (11 -> 6: both
// borders, 6 -> 3: one); the classes above are then no tap classes, and the launch's order comes from struct TileOrder alone.
struct PosMajor {
  int n, H, W;          // images, (output) map
  int st, HI, WI;       // stride, input map (stride 1: H, W)
  int uni, base, rp;    // the tile lies on ONE position: its virtual rows start at base = v * n, rp = y * W + x
  __host__ __device__ __forceinline__ void pos(int v, int& y, int& x) const {
    const int Hi = H > 2 ? H - 2 : 0, Wi = W > 2 ? W - 2 : 0, Hb = H - Hi, Wb = W - Wi;       // interior / border coordinates
    int u = v;
    if (u < Hi * Wi) { y = u / Wi + 1; x = u % Wi + 1; return; }
    u -= Hi * Wi;
    if (u < Hi * Wb) { y = u / Wb + 1; x = (u % Wb) ? W - 1 : 0; return; }
    u -= Hi * Wb;
    if (u < Hb * Wi) { y = (u / Wi) ? H - 1 : 0; x = u % Wi + 1; return; }
    u -= Hb * Wi;
    y = (u / Wb) ? H - 1 : 0;
    x = (u % Wb) ? W - 1 : 0;
  }
  __host__ __device__ __forceinline__ uint32_t taps(int y, int x) const {      // bit tap: the tap's neighbour of (y, x) is inside the image
    uint32_t mk = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      mk |= (uint32_t)((unsigned)(st * y + tap / 3 - 1) < (unsigned)HI && (unsigned)(st * x + tap % 3 - 1) < (unsigned)WI) << tap;
    return mk;
  }
  __device__ __forceinline__ int row(int r) const {                   // the real row (image * H * W + y * W + x) of virtual row r
    if (uni) return (r - base) * (H * W) + rp;
    const int v = r / n;
    int y, x;
    pos(v, y, x);
    return (r - v * n) * (H * W) + y * W + x;
  }
};

// Common tail of both kernels: lane pairs complete the row sums, then either the split-K slab store or the fused
// epilogue.  Accumulator layout: lane owns column (lane&31), rows (r&3) + 8*(r>>2) + 4*(lane>>5).
template <int TM, int TN, bool PM = false>
__device__ __forceinline__ void finish_tile(const tavsr_gemm_desc& d, int nsplit, f32x16 (&acc)[TM][TN],
                                            float (&asum)[TM], bool want_rowsum, int m0, int n0, int wm, int wn, int lr,
                                            int lk, int z1, int z2, int64_t coff, int zidx, const float* bias_pre = nullptr,
                                            const PosMajor* pm = nullptr) {
  if (want_rowsum) {
#pragma unroll
    for (int i = 0; i < TM; ++i) asum[i] += __shfl_xor(asum[i], 32, 64);
  }

  // ---- split-K: every slice stores its raw accumulators (and row sums) to its slab; splitk_epilogue_kernel
  //      sums the slabs in slice order (deterministic) and applies the epilogue
  if (nsplit > 1) {
    const int64_t mn = (int64_t)d.M * d.N;
    const int nbatch = gridDim.y;
    float* slab = d.ws + ((int64_t)zidx * nbatch + blockIdx.y) * mn;
    float* rsum0 = d.ws + (int64_t)nsplit * nbatch * mn;       // [nsplit][M] (only when nbatch == 1)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * TN * 32 + j * 32 + lr;
      if (n >= d.N) continue;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int mb = m0 + wm * TM * 32 + i * 32 + 4 * lk;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mb + (r & 3) + 8 * (r >> 2);
          if (m < d.M) slab[(int64_t)(PM ? pm->row(m) : m) * d.N + n] = acc[i][j][r];
        }
      }
    }
    if (want_rowsum && lk == 0) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * TM * 32 + i * 32 + lr;
        if (m < d.M) rsum0[(int64_t)zidx * d.M + m] = asum[i];
      }
    }
    return;
  }

  // ---- epilogue: lane owns column (lane&31), rows (r&3) + 8*(r>>2) + 4*(lane>>5)
  if (want_rowsum && lk == 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * TM * 32 + i * 32 + lr;
      if (m < d.M) d.a_rowsum[m] = d.alpha * asum[i];
    }
  }
  float* C = d.C + coff;
  float* Z = d.Z ? d.Z + coff : nullptr;
  const float* R = d.R ? d.R + z1 * d.sR1 + z2 * d.sR2 : nullptr;
  const float* DZ = d.DZ ? d.DZ + coff : nullptr;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * TN * 32 + j * 32 + lr;
    if (n >= d.N) continue;
    const float bv = bias_pre ? bias_pre[j] : (d.bias ? d.bias[n] : 0.f);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mb = m0 + wm * TM * 32 + i * 32 + 4 * lk;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mv = mb + (r & 3) + 8 * (r >> 2);
        if (mv >= d.M) continue;
        const int m = PM ? pm->row(mv) : mv;
        float v = acc[i][j][r] + bv;
        const int64_t o = (int64_t)m * d.ldc + n;
        if (Z) Z[o] = v;
        v = act_fwd(d.act, v);
        if (DZ) v *= act_bwd(d.dact, DZ[o]);
        v *= d.alpha;
        if (R) v += R[(int64_t)m * d.ldr + n];
        C[o] = v;
      }
    }
  }
}

// Epilogue through LDS (the staging ring is free once the K loop is over): the accumulators (lane = column, registers =
// rows) are written to a [BM][BN] image and read back row-wise, so that bias / pre-activation store / activation /
// act' / alpha / residual and the C (or split-K slab) store all move 16 bytes per lane along rows - a wave instruction
// covers whole 256-byte row segments instead of 2 x 128 bytes, and a 64x64 tile with a pre-activation output issues 8
// store instructions per lane instead of 32.  At K = 256 the old per-register epilogue was a third of a block's life
// (profiles/r01_gemm_trace.txt).  Needs N % 4 == 0 and 16-byte aligned rows of every output / epilogue operand.
template <int BM, int BN, int NT, int TM, int TN, bool PM = false>
__device__ __forceinline__ void finish_tile_vec(const tavsr_gemm_desc& d, int nsplit, f32x16 (&acc)[TM][TN], float* __restrict__ img,
                                                int m0, int n0, int wm, int wn, int lr, int lk, int z1, int z2, int64_t coff,
                                                int tid, int zidx, const PosMajor* pm = nullptr) {
  __syncthreads();                                   // every wave has finished reading the staging ring
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        img[(wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk) * BN + wn * TN * 32 + j * 32 + lr] = acc[i][j][r];
  __syncthreads();
  constexpr int V4R = BN / 4, PER = BM * BN / 4 / NT;
  static_assert(BM * BN % (4 * NT) == 0, "tile must divide over the block");
  const bool split = nsplit > 1;
  float* base;
  int64_t ld;
  if (split) {
    base = d.ws + ((int64_t)zidx * gridDim.y + blockIdx.y) * ((int64_t)d.M * d.N);
    ld = d.N;
  } else {
    base = d.C + coff;
    ld = d.ldc;
  }
  const float* R = (!split && d.R) ? d.R + z1 * d.sR1 + z2 * d.sR2 : nullptr;
  float* Z = (!split && d.Z) ? d.Z + coff : nullptr;
  const float* DZ = (!split && d.DZ) ? d.DZ + coff : nullptr;
  const bool rowstat = BN == 64 && !split && d.rowstat != nullptr;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int idx = q * NT + tid, row = idx / V4R, c4 = idx % V4R;
    const int mv = m0 + row, n = n0 + 4 * c4;
    const bool ok = mv < d.M && n < d.N;
    const int m = PM && ok ? pm->row(mv) : mv;       // conv_posmajor: every row-addressed access below takes the real row
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
    v = *reinterpret_cast<const float4*>(img + row * BN + 4 * c4);
    const int64_t o = (int64_t)m * ld + n;
    if (!split) {
      if (d.bias) {
        const float4 b = *reinterpret_cast<const float4*>(d.bias + n);
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
      }
      if (Z) *reinterpret_cast<float4*>(Z + o) = v;
      v.x = act_fwd(d.act, v.x); v.y = act_fwd(d.act, v.y); v.z = act_fwd(d.act, v.z); v.w = act_fwd(d.act, v.w);
      if (DZ) {
        const float4 z = *reinterpret_cast<const float4*>(DZ + o);
        v.x *= act_bwd(d.dact, z.x); v.y *= act_bwd(d.dact, z.y); v.z *= act_bwd(d.dact, z.z); v.w *= act_bwd(d.dact, z.w);
      }
      if (d.drop_p > 0.f) {              // one Philox call per 16-byte group (the mask tavsr_dropout draws for [M][N])
        const uint64_t sd = d.drop_seed[0], ctr = (d.drop_offset >> 2) + (uint64_t)(((int64_t)m * d.N + n) >> 2);
        const uint32_t thr = (uint32_t)((double)d.drop_p * 4294967296.0);
        const float ik = 1.f / (1.f - d.drop_p);
        uint32_t w[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), w);
        v.x = w[0] >= thr ? v.x * ik : 0.f; v.y = w[1] >= thr ? v.y * ik : 0.f;
        v.z = w[2] >= thr ? v.z * ik : 0.f; v.w = w[3] >= thr ? v.w * ik : 0.f;
      }
      v.x *= d.alpha; v.y *= d.alpha; v.z *= d.alpha; v.w *= d.alpha;
      if (R) {
        const float4 rr = *reinterpret_cast<const float4*>(R + (int64_t)m * d.ldr + n);
        v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
      }
    }
    *reinterpret_cast<float4*>(base + o) = v;
    }
    if (rowstat) {       // the 16 lanes that share a row of a 64-wide tile: sum of what was stored and M2 about the tile's own mean ...
      float s1 = ok ? (v.x + v.y) + (v.z + v.w) : 0.f, s2 = 0.f;
      if (d.rowdot_a) {  // ... or its two weighted sums (tavsr_gemm_desc.rowdot_a / _b: the merge's pooling and branch-weight projections)
        const float4 wa = ok ? *reinterpret_cast<const float4*>(d.rowdot_a + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 wb = ok ? *reinterpret_cast<const float4*>(d.rowdot_b + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        s1 = (v.x * wa.x + v.y * wa.y) + (v.z * wa.z + v.w * wa.w);
        s2 = (v.x * wb.x + v.y * wb.y) + (v.z * wb.z + v.w * wb.w);
      }
#pragma unroll
      for (int o2 = 8; o2 > 0; o2 >>= 1) s1 += __shfl_xor(s1, o2, 64);
      if (!d.rowdot_a && ok) {   // deviations from the tile mean (of its min(64, N - n0) valid columns), never raw squares: no cancellation
        const float tm = s1 / (float)min(64, d.N - n0);
        const float e0 = v.x - tm, e1 = v.y - tm, e2 = v.z - tm, e3 = v.w - tm;
        s2 = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
      }
#pragma unroll
      for (int o2 = 8; o2 > 0; o2 >>= 1) s2 += __shfl_xor(s2, o2, 64);
      if (c4 == 0 && mv < d.M)
        *reinterpret_cast<float2*>(d.rowstat + ((int64_t)m * ((d.N + 63) / 64) + n0 / 64) * 2) = make_float2(s1, s2);
    }
  }
}

// host-side test of the vectorised epilogue's requirements
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool vec_epi_ok(const tavsr_gemm_desc& d) {
  return d.N % 4 == 0 && d.ldc % 4 == 0 && d.sC1 % 4 == 0 && d.sC2 % 4 == 0 && aligned16(d.C) && (!d.bias || aligned16(d.bias)) &&
         (!d.Z || aligned16(d.Z)) && (!d.DZ || aligned16(d.DZ)) &&
         (!d.R || (aligned16(d.R) && d.ldr % 4 == 0 && d.sR1 % 4 == 0 && d.sR2 % 4 == 0)) && (!d.ws || aligned16(d.ws));
}

// ---------------------------------------------------------------------------------------------- LDS-DMA kernel
// Fast path for tiles whose operands can be fetched with unpredicated 16-byte loads (aligned, K a multiple of 32,
// row-contiguous operands with rows % 4 == 0).  Operand tiles go global -> LDS directly (global_load_lds_dwordx4:
// no staging registers, so the compiler cannot turn the prefetch into a synchronous load by copying its result
// registers - which is what it did to the register ring of gemm_kernel, profiles/r01_gemm_notes.md) through a ring
// of S LDS stages; a counted s_waitcnt vmcnt leaves S-2 tiles in flight across the ONE barrier per K-step.
// LDS images (a wave-instruction writes 1 KB linearly: no padding possible, conflicts are avoided by swizzling):
//   k-contiguous operand  : [row][32 floats]; 16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 7)
//                           (the SOURCE address is permuted, the LDS write stays linear; ds_read_b128 applies the
//                           same XOR: the 16 lanes of a b128 group hit 16 distinct 16-byte slots)
//   row-contiguous operand: [k][ROWS floats], read by ds_read_b32 over 32 consecutive rows
//   B as three bf16 planes : [plane][row][4 chunks of 8 bf16], chunk c of row r at c ^ ((r >> 2) & 3) ("split operands" below)
typedef __attribute__((address_space(3))) float lds_float;
typedef const __attribute__((address_space(1))) float glb_float;

template <int ROWS, bool KMAJOR, int NT>
struct GLoader {
  static constexpr int NR = ROWS * 8 / NT;   // LDS-DMA instructions per thread per tile
  static_assert(ROWS * 8 % NT == 0, "tile must divide over the block");
  __device__ static __forceinline__ void offsets(int64_t ld, int row0, int nrows, int tid, int64_t (&off)[NR]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int q = i * NT + tid;
      if (KMAJOR) {
        const int k = q / (ROWS / 4);
        int r = row0 + (q % (ROWS / 4)) * 4;
        if (r + 3 >= nrows) r = row0;            // rows past the edge are never stored: any valid address will do
        off[i] = (int64_t)k * ld + r;
      } else {
        const int row = q >> 3, cp = q & 7;
        const int cl = cp ^ ((row >> 1) & 7);
        off[i] = (int64_t)min(row0 + row, nrows - 1) * ld + cl * 4;
      }
    }
  }
  __device__ static __forceinline__ void issue(const float* __restrict__ g, const int64_t (&off)[NR],
                                               float* __restrict__ stage, int wave) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
      __builtin_amdgcn_global_load_lds((glb_float*)(g + off[i]), (lds_float*)(stage + (i * NT + wave * 64) * 4), 16, 0, 0);
  }
};

__device__ __forceinline__ void dma16(const float* src, float* dst) {      // one 16-byte (per lane) LDS-DMA; dst: the wave's 1 KB
  __builtin_amdgcn_global_load_lds((glb_float*)src, (lds_float*)dst, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const float* src, float* dst) {       // 4-byte gather; dst: the wave's 256 bytes
  __builtin_amdgcn_global_load_lds((glb_float*)src, (lds_float*)dst, 4, 0, 0);
}

#ifndef TAVSR_GEMM_SB
#define TAVSR_GEMM_SB 1
#endif
#if TAVSR_GEMM_SB
#define GEMM_SB() __builtin_amdgcn_sched_barrier(0)
#else
#define GEMM_SB()
#endif

template <int ROWS, bool KMAJOR>
__device__ __forceinline__ void read_frag_g(const float* __restrict__ s, int row, int g, int lk, float (&f)[4]) {
  if (KMAJOR) {
    const float* p = s + (g * 8 + 4 * lk) * ROWS + row;
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = p[j * ROWS];
  } else {
    const float4 v = *reinterpret_cast<const float4*>(s + row * 32 + (((2 * g + lk) ^ ((row >> 1) & 7)) << 2));
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
}

// ---------------------------------------------------------------------------------------------- split operands (x6)
// bf16 MFMA on three-way split fp32 operands (tavsr_gemm_desc.conv_posmajor, bit 4): x = h + m + l, every part a bf16 value rounded to
// nearest from what the parts before it left (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); the subtractions are exact and
// so is the sum for normal-range x).  A product a b is the six MFMAs hl, lh, mm, hm, mh, hh of one 16-k block, small to large
// into the ONE fp32 accumulator; ml, lm, ll (<= 2^-23 |a b|) are dropped.  Zeros split to zeros, NaN to NaN; +-inf gives
// inf - inf = NaN in m.
//   A stays the fp32 image above and is split in registers: the lane's two read_frag_g chunks of a 16-k block (k-groups 2b and
//     2b + 1: k = 16b + 4 lk + j and + 8) are the 8 values of its MFMA operand, in that order.
//   B arrives split (tavsr_conv_wsplit): three planes [N][K] bf16 in which the 16 k of a block are stored in the order the A
//     lanes hold them - 16-byte chunk lk of block b = k 16b + 4 lk + {0..3}, 16b + 8 + 4 lk + {0..3} - so one ds_read_b128 is a
//     lane's operand of one plane.  LDS image: [plane][row][4 chunks] (64 bytes per row and plane), chunk c = 2b + lk of row r
//     stored at chunk c ^ ((r >> 2) & 3) (the SOURCE address is permuted, as above): the 16 lanes of a ds_read_b128 group are
//     rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of one chunk - r & 3 picks one of 4 64-byte rows of the 256-byte bank
//     window, (r >> 2) & 3 is different in each of the group's four quads: 16 distinct slots.
// A k-major fragment reader can join by filling the same 8-value registers (split_frag takes them from anywhere).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kX6RowFloats = 48;      // a B row of a K-step in LDS: 3 planes x 32 bf16

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {      // (bf16(a), bf16(b)) rounded to nearest even, a in the low half
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
// (gemm_conv.hip is built with SLP vectorisation off, csrc/Makefile: left to itself hipcc pairs the neighbouring subtractions below into
// v_pk_add_f32, which costs an MFMA gap far more than two v_sub_f32 do - profiles/r15_notes.md.  The same exact arithmetic either way.)
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = pk_bf16(a, b);
  a -= __uint_as_float(h << 16);
  b -= __uint_as_float(h & 0xffff0000u);
  m = pk_bf16(a, b);
  a -= __uint_as_float(m << 16);
  b -= __uint_as_float(m & 0xffff0000u);
  l = pk_bf16(a, b);
}
// the 8 fp32 values of a lane's operand of one 16-k block -> its three bf16 operands
__device__ __forceinline__ void split_frag(const float (&f)[8], uint4& h, uint4& m, uint4& l) {
  split_pair(f[0], f[1], h.x, m.x, l.x);
  split_pair(f[2], f[3], h.y, m.y, l.y);
  split_pair(f[4], f[5], h.z, m.z, l.z);
  split_pair(f[6], f[7], h.w, m.w, l.w);
}
__device__ __forceinline__ f32x16 mfma_bf16(const uint4& a, const uint4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// LDS-DMA of the B planes' K-step (BN rows x 3 planes x 4 chunks of 16 bytes) into the image above
template <int ROWS, int NT>
struct PlaneLoader {
  static constexpr int NR = ROWS * 12 / NT;
  static_assert(ROWS * 12 % NT == 0 && (ROWS * 4) % 64 == 0, "a wave instruction stays inside one plane");
  // float offsets of this thread's chunks at k = 0 (planes of n rows x K bf16 each, fewer than 2^31 bytes in all)
  __device__ static __forceinline__ void offsets(int K, int row0, int nrows, int tid, int (&off)[NR]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int q = i * NT + tid, plane = q / (ROWS * 4), r = q % (ROWS * 4);
      const int row = r >> 2, cl = (r & 3) ^ ((row >> 2) & 3);
      off[i] = (plane * nrows + min(row0 + row, nrows - 1)) * (K / 2) + cl * 4;
    }
  }
  // gk: the planes at the K-step's k (2 bf16 per float)
  __device__ static __forceinline__ void issue(const float* __restrict__ gk, const int (&off)[NR], float* __restrict__ img, int wave) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
      __builtin_amdgcn_global_load_lds((glb_float*)(gk + off[i]), (lds_float*)(img + (i * NT + wave * 64) * 4), 16, 0, 0);
  }
};
// a lane's operand of plane p, row `row`, 16-k block b
template <int ROWS>
__device__ __forceinline__ uint4 read_plane(const float* __restrict__ s, int p, int row, int b, int lk) {
  return *reinterpret_cast<const uint4*>(s + ((p * ROWS + row) * 4 + ((2 * b + lk) ^ ((row >> 2) & 3))) * 4);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

#ifdef TAVSR_GEMM_TRACE
// Debug build only (scripts/gpu_trace.sh): per-workgroup timestamps of the LDS-DMA kernel's phases, one table per translation unit.
constexpr int kTraceMax = 1 << 15;
static __device__ unsigned long long g_trace[kTraceMax][6];
static __device__ unsigned int g_trace_n;
#define TAVSR_TRACE_DECL unsigned long long tr_t[4], tr_c[4]; tr_t[0] = wall_clock64(); tr_t[1] = tr_t[0]; tr_c[1] = tr_c[2] = 0;
#define TAVSR_TRACE_AT(i) { tr_t[i] = wall_clock64(); tr_c[i] = __builtin_readcyclecounter(); }
// copy out (and reset) this unit's table. out: [max_rows][6] uint64. Returns rows.
static int trace_read_unit(unsigned long long* out, int max_rows) {
  unsigned int n = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_trace_n), sizeof(n)) != hipSuccess) return -1;
  int rows = (int)(n < (unsigned)kTraceMax ? n : kTraceMax);
  if (rows > max_rows) rows = max_rows;
  if (rows > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), (size_t)rows * 6 * sizeof(unsigned long long)) != hipSuccess) return -1;
  n = 0;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_trace_n), &n, sizeof(n)) != hipSuccess) return -1;
  return rows;
}
int conv_trace_read(unsigned long long* out, int max_rows);      // gemm_conv.hip's table
#else
#define TAVSR_TRACE_DECL
#define TAVSR_TRACE_AT(i)
#endif

// ---------------------------------------------------------------------------------------------- operand sources
// A source owns ONE fetch scheme's per-tile state and address arithmetic, and nothing else.  glds_tile needs of it:
//   Src(const TileCtx&)       per-tile set-up
//   kDma                      LDS-DMA instructions per thread per K-step (the counted vmcnt wait is derived from it)
//   steps()                   K-steps this tile runs
//   issue(kt, stage)          the LDS-DMA of its kt-th K-step into a ring stage: A image at stage, B image at stage + BM * 32
// and, with the defaults of SourceDefaults: fix_last (K tail), rowsum_n0, kPosMajorRows / row_map (position-major rows).
// Where the two operands are fetched independently of each other, a source is a PairSource of two operand halves
// (Half(const TileCtx&), kDma, issue(kt, image)); the position-major modes walk both operands with one cursor and are whole
// sources.  SourceFor picks the type from (CONV, PM, AK, BKM): the plain source here, the K tail in gemm.hip, the convolution
// and Conv3d stem sources in gemm_conv.hip.
struct TileCtx {             // what a source may know of its tile (workgroup-uniform but for tid)
  const tavsr_gemm_desc& d;
  const float* A;            // the batch's operands
  const float* B;
  int m0, n0;                // first row of op(A) / column of op(B)
  int kbeg, kend;            // the K slice
  int tid, wave;
};

struct SourceDefaults {
  static constexpr bool kPosMajorRows = false;                                                  // the epilogue maps virtual rows ...
  __device__ __forceinline__ const PosMajor* row_map() const { return nullptr; }                // ... with this
  __device__ __forceinline__ static int rowsum_n0(const tavsr_gemm_desc&) { return 0; }         // the column tile that takes the row sums of op(A)
  // (stage, klen, kt, tid): called in front of the last K-step kt's MFMAs where the slice's klen k values do not end on a 16-byte chunk
  __device__ __forceinline__ void fix_last(float*, int, int, int) const {}
};

// The plain fetch of one operand: the thread's chunk offsets are fixed, a K-step moves the base.
template <int ROWS, bool KMAJOR, int NT, bool B_SIDE>
struct PlainOperand {
  using L = GLoader<ROWS, KMAJOR, NT>;
  static constexpr int kDma = L::NR;
  const TileCtx& c;
  int64_t off[L::NR];
  const float* gk;          // the operand at k = kbeg
  int64_t kstep;
  __device__ __forceinline__ explicit PlainOperand(const TileCtx& c_) : c(c_) {
    const int64_t ld = B_SIDE ? c.d.ldb : c.d.lda;
    L::offsets(ld, B_SIDE ? c.n0 : c.m0, B_SIDE ? c.d.N : c.d.M, c.tid, off);
    kstep = KMAJOR ? (int64_t)kBK * ld : kBK;
    gk = (B_SIDE ? c.B : c.A) + (KMAJOR ? (int64_t)c.kbeg * ld : c.kbeg);
  }
  __device__ __forceinline__ void issue(int kt, float* img) { L::issue(gk + kt * kstep, off, img, c.wave); }
};

// The B operand as the three bf16 planes behind B [N][K] (kConvX6; the image is described at "split operands" above)
constexpr int kConvX6 = 16;      // tavsr_gemm_desc.conv_posmajor, bit 4
constexpr int kConvX6Dw = 32;    // ... bit 5: the weight gradient on split operands, both split in registers (gemm_conv.hip, conv_x6_dw)
__device__ __forceinline__ const float* x6_planes(const tavsr_gemm_desc& d) { return d.B + (int64_t)d.N * d.K; }
template <int ROWS, int NT>
struct PlaneOperand {
  using L = PlaneLoader<ROWS, NT>;
  static constexpr int kDma = L::NR;
  const TileCtx& c;
  int off[L::NR];
  const float* gk;          // the planes at k = kbeg
  __device__ __forceinline__ explicit PlaneOperand(const TileCtx& c_) : c(c_) {
    L::offsets(c.d.K, c.n0, c.d.N, c.tid, off);
    gk = x6_planes(c.d) + c.kbeg / 2;
  }
  __device__ __forceinline__ void issue(int kt, float* img) { L::issue(gk + kt * (kBK / 2), off, img, c.wave); }
};

template <class HA, class HB, int BM>
struct PairSource : SourceDefaults {
  static constexpr int kDma = HA::kDma + HB::kDma;
  HA a;
  HB b;
  int nk;                   // whole K-steps (host guarantees it)
  __device__ __forceinline__ explicit PairSource(const TileCtx& c) : a(c), b(c), nk((c.kend - c.kbeg) / kBK) {}
  __device__ __forceinline__ int steps() const { return nk; }
  __device__ __forceinline__ void issue(int kt, float* stage) {
    a.issue(kt, stage);
    b.issue(kt, stage + BM * kBK);
  }
};

template <int CONV, bool PM, int BM, int BN, int NT, bool AK, bool BKM, bool X6 = false>
struct SourceFor;           // ::type, specialised next to each source (X6: CONV 1 with B as bf16 planes; CONV 2 with its fp32 sources)
template <int BM, int BN, int NT, bool AK, bool BKM>
struct SourceFor<0, false, BM, BN, NT, AK, BKM> {
  using type = PairSource<PlainOperand<BM, AK, NT, false>, PlainOperand<BN, BKM, NT, true>, BM>;
};

// ---------------------------------------------------------------------------------------------- the ring
// One output tile of one problem: `bid` is the (already remapped) linear tile index inside the problem.  The source's K-steps go
// through a ring of S LDS stages: S-1 of them are in flight after the prologue, a counted vmcnt wait and ONE barrier per K-step
// hand the oldest to the MFMAs while the DMA of the step S-1 ahead is issued into the stage everyone has just left.
// KW > 1: the k-groups of every K-step are dealt to KW wave sets (intra-block K split, summed through LDS at the end):
// a lone 64x64 tile on a CU then runs 2 waves per SIMD with half the dependent-MFMA chain per K-step each.
// Two slice lengths (plan_conv, gemm_conv.hip): the first n_big slices are kunit longer; n_big = 0 everywhere else.
// X6 (CONV 1 with both operands k-contiguous): the K-step runs on bf16 MFMAs over split operands ("split operands" above); the
// stage's B image is then the three planes (BN * 192 bytes instead of BN * 128).
// X6 with CONV 2 (weight gradient, both operands k-major): both operands are activations, so the stage holds the two fp32 k-major
// images as without X6 and both are split in registers; the row sums stay fp32 in the fp32 path's association.
template <int BM, int BN, int WM, int WN, int S, bool AK, bool BKM, int KW = 1, int CONV = 0, bool PM = false, bool X6 = false>
__device__ __forceinline__ void glds_tile(const tavsr_gemm_desc& d, int kchunk, int nsplit, int tiles_n, int bid, bool vec_epi,
                                          int zidx, int n_big = 0, int kunit = 0) {
  constexpr int BK = kBK, NG = BK / 8;
  static_assert(NG % KW == 0, "k-groups must divide over the wave sets");
  static_assert(!PM || KW == 1, "position-major order: one wave set");
  static_assert(!X6 || (KW == 1 && ((CONV == 1 && !AK && !BKM) || (CONV == 2 && AK && BKM))),
                "split operands: CONV 1 with both operands k-contiguous or CONV 2 with both k-major, one wave set");
  constexpr int NT = WM * WN * KW * 64;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  using Src = typename SourceFor<CONV, PM, BM, BN, NT, AK, BKM, X6>::type;
  constexpr int ASZ = BM * BK, STAGE = BM * BK + BN * (X6 && !AK ? kX6RowFloats : BK);      // (the weight gradient's B stays an fp32 image)
  constexpr int G = Src::kDma;                  // LDS-DMA instructions per wave per tile
  static_assert((S - 2) * G <= 63, "vmcnt field");
  __shared__ __attribute__((aligned(1024))) float smem[S * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kw = wave / (WM * WN), w2 = wave % (WM * WN);
  const int wm = w2 / WN, wn = w2 % WN;
  const int lr = lane & 31, lk = lane >> 5;

  TAVSR_TRACE_DECL
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int z1 = blockIdx.y / d.nb2, z2 = blockIdx.y % d.nb2;
  const float* A = d.A + z1 * d.sA1 + z2 * d.sA2;
  const float* B = d.B + z1 * d.sB1 + z2 * d.sB2;
  const int64_t coff = z1 * d.sC1 + z2 * d.sC2;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float asum[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) asum[i] = 0.f;
  float bpre[TN];      // the epilogue's bias values, fetched under the K loop instead of in front of the stores
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * TN * 32 + j * 32 + lr;
    bpre[j] = (d.bias && nsplit == 1 && n < d.N) ? d.bias[n] : 0.f;
  }

  const int kbeg = zidx * kchunk + min(zidx, n_big) * kunit;
  const int kend = min(d.K, kbeg + kchunk + (zidx < n_big ? kunit : 0));
  const TileCtx ctx{d, A, B, m0, n0, kbeg, kend, tid, wave};
  Src src(ctx);
  const int nk = src.steps();
  const bool want_rowsum = d.a_rowsum != nullptr && n0 == Src::rowsum_n0(d) && wn == 0;

  const int arow = wm * TM * 32 + lr, brow = wn * TN * 32 + lr;
  auto compute = [&](int st) {
    const float* a_s = smem + st * STAGE;
    const float* b_s = a_s + ASZ;
    if constexpr (X6 && AK) {
      // weight gradient: both operands are activations in the fp32 k-major images, both split here; the 8 values of a lane are
      // k = 16b + 4 lk + {0..3} and + 8 for A and for B alike
      float af[2][TM][8], bf[2][TN][8];
      auto read_block = [&](int b, float (&fa)[TM][8], float (&fb)[TN][8]) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          float lo[4], hi[4];
          read_frag_g<BM, true>(a_s, arow + i * 32, 2 * b, lk, lo);
          read_frag_g<BM, true>(a_s, arow + i * 32, 2 * b + 1, lk, hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) { fa[i][e] = lo[e]; fa[i][4 + e] = hi[e]; }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float lo[4], hi[4];
          read_frag_g<BN, true>(b_s, brow + j * 32, 2 * b, lk, lo);
          read_frag_g<BN, true>(b_s, brow + j * 32, 2 * b + 1, lk, hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) { fb[j][e] = lo[e]; fb[j][4 + e] = hi[e]; }
        }
      };
      read_block(0, af[0], bf[0]);
#pragma unroll
      for (int b = 0; b < BK / 16; ++b) {
        const int c = b & 1;
        if (b + 1 < BK / 16) read_block(b + 1, af[c ^ 1], bf[c ^ 1]);
        GEMM_SB();        // as below: the next block's fragment reads, then this block's splits and MFMAs
        uint4 aq[TM][3], bq[TN][3];
#pragma unroll
        for (int i = 0; i < TM; ++i) split_frag(af[c][i], aq[i][0], aq[i][1], aq[i][2]);
#pragma unroll
        for (int j = 0; j < TN; ++j) split_frag(bf[c][j], bq[j][0], bq[j][1], bq[j][2]);
#pragma unroll
        for (int pr = 0; pr < 6; ++pr) {
          constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = mfma_bf16(aq[i][PA[pr]], bq[j][PB[pr]], acc[i][j]);
        }
        // the bias gradient stays fp32, in the fp32 path's association: one add per 8-k group, in group order (bit-identical)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          asum[i] += (af[c][i][0] + af[c][i][1]) + (af[c][i][2] + af[c][i][3]);
          asum[i] += (af[c][i][4] + af[c][i][5]) + (af[c][i][6] + af[c][i][7]);
        }
        GEMM_SB();
      }
      return;
    } else if constexpr (X6) {
      float af[2][TM][8];
      uint4 bq[2][TN][3];
      auto read_block = [&](int b, float (&fa)[TM][8], uint4 (&qb)[TN][3]) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          float lo[4], hi[4];
          read_frag_g<BM, false>(a_s, arow + i * 32, 2 * b, lk, lo);
          read_frag_g<BM, false>(a_s, arow + i * 32, 2 * b + 1, lk, hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) { fa[i][e] = lo[e]; fa[i][4 + e] = hi[e]; }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int p = 0; p < 3; ++p) qb[j][p] = read_plane<BN>(b_s, p, brow + j * 32, b, lk);
      };
      read_block(0, af[0], bq[0]);
#pragma unroll
      for (int b = 0; b < BK / 16; ++b) {
        const int c = b & 1;
        if (b + 1 < BK / 16) read_block(b + 1, af[c ^ 1], bq[c ^ 1]);
        GEMM_SB();        // as below: the next block's fragment reads, then this block's split and MFMAs
        uint4 ah[TM], am[TM], al[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) split_frag(af[c][i], ah[i], am[i], al[i]);
        // hl, lh, mm, hm, mh, hh: small to large (index 0 / 1 / 2 = h / m / l)
#pragma unroll
        for (int pr = 0; pr < 6; ++pr) {
          constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = mfma_bf16(PA[pr] == 0 ? ah[i] : PA[pr] == 1 ? am[i] : al[i], bq[c][j][PB[pr]], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
          asum[i] += ((af[c][i][0] + af[c][i][1]) + (af[c][i][2] + af[c][i][3])) + ((af[c][i][4] + af[c][i][5]) + (af[c][i][6] + af[c][i][7]));
        GEMM_SB();
      }
      return;
    }
    float af[2][TM][4], bf[2][TN][4];
#pragma unroll
    for (int i = 0; i < TM; ++i) read_frag_g<BM, AK>(a_s, arow + i * 32, kw, lk, af[0][i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) read_frag_g<BN, BKM>(b_s, brow + j * 32, kw, lk, bf[0][j]);
#pragma unroll
    for (int q = 0; q < NG / KW; ++q) {      // this wave set's k-groups: kw, kw + KW, ...
      const int c = q & 1;
      if (q + 1 < NG / KW) {
#pragma unroll
        for (int i = 0; i < TM; ++i) read_frag_g<BM, AK>(a_s, arow + i * 32, kw + (q + 1) * KW, lk, af[c ^ 1][i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) read_frag_g<BN, BKM>(b_s, brow + j * 32, kw + (q + 1) * KW, lk, bf[c ^ 1][j]);
      }
      // keep the order "next group's fragment reads, then this group's MFMAs": left alone, hipcc sinks the reads to just in
      // front of their first use and waits lgkmcnt(0) there - one exposed LDS latency per k-group (TAVSR_GEMM_SB=0 at build
      // time restores that)
      GEMM_SB();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][i][kk], bf[c][j][kk], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i) asum[i] += (af[c][i][0] + af[c][i][1]) + (af[c][i][2] + af[c][i][3]);
      GEMM_SB();
    }
  };

  // prologue: tiles 0 .. S-2 in flight
#pragma unroll
  for (int j = 0; j < S - 1; ++j)
    if (j < nk) src.issue(j, smem + j * STAGE);
  int st = 0;             // stage of tile kt
  int kt = 0;
  // steady state: tile kt landed when at most (S-2) tiles issued after it are still in flight
  for (; kt + S - 1 < nk; ++kt) {
    wait_vmcnt<(S - 2) * G>();
    __builtin_amdgcn_s_barrier();      // every wave's part of tile kt is in LDS; everyone left stage (kt-1) % S
#ifdef TAVSR_GEMM_TRACE
    if (kt == 0) TAVSR_TRACE_AT(1)
#endif
    const int sn = st == 0 ? S - 1 : st - 1;
    src.issue(kt + S - 1, smem + sn * STAGE);
    compute(st);
    st = st + 1 == S ? 0 : st + 1;
  }
  // drain: nothing left to issue
  for (; kt < nk; ++kt) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    // (the test stays out here, joined to the step's: inside fix_last it cost the K-tail kernels 5 - 24 spilled SGPRs)
    if (kt == nk - 1 && ((kend - kbeg) & 3) != 0) src.fix_last(smem + st * STAGE, kend - kbeg, kt, tid);
    compute(st);
    st = st + 1 == S ? 0 : st + 1;
  }
  TAVSR_TRACE_AT(2)
  if (KW > 1) {     // sum the wave sets' accumulators (and row sums) through LDS; set 0 runs the epilogue
    constexpr int PER = TM * TN * 16;
    float* red = smem;                                         // [KW-1][WM*WN][PER][64]
    float* rsum = smem + (KW - 1) * WM * WN * PER * 64;        // [KW-1][WM*WN][TM][64]
    static_assert(((KW - 1) * WM * WN * (PER + TM) * 64) <= S * STAGE, "reduction must fit in the staging ring");
    __syncthreads();                                           // all LDS reads of the K loop are done
    if (kw > 0) {
      float* r0 = red + ((kw - 1) * WM * WN + w2) * PER * 64 + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) r0[((i * TN + j) * 16 + r) * 64] = acc[i][j][r];
#pragma unroll
      for (int i = 0; i < TM; ++i) rsum[(((kw - 1) * WM * WN + w2) * TM + i) * 64 + lane] = asum[i];
    }
    __syncthreads();
    if (kw > 0) return;
#pragma unroll
    for (int s2 = 0; s2 < KW - 1; ++s2) {
      const float* r0 = red + (s2 * WM * WN + w2) * PER * 64 + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += r0[((i * TN + j) * 16 + r) * 64];
#pragma unroll
      for (int i = 0; i < TM; ++i) asum[i] += rsum[((s2 * WM * WN + w2) * TM + i) * 64 + lane];
    }
  }
  if (KW == 1 && vec_epi) {
    static_assert(KW > 1 || BM * BN <= S * STAGE, "the output tile image must fit in the staging ring");
    if (want_rowsum) {              // bias gradients (row sums of op(A)): as finish_tile
#pragma unroll
      for (int i = 0; i < TM; ++i) asum[i] += __shfl_xor(asum[i], 32, 64);
      if (lk == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int m = m0 + wm * TM * 32 + i * 32 + lr;
          if (m < d.M) {
            if (nsplit > 1) (d.ws + (int64_t)nsplit * gridDim.y * d.M * d.N)[(int64_t)zidx * d.M + m] = asum[i];
            else d.a_rowsum[m] = d.alpha * asum[i];
          }
        }
      }
    }
    finish_tile_vec<BM, BN, NT, TM, TN, Src::kPosMajorRows>(d, nsplit, acc, smem, m0, n0, wm, wn, lr, lk, z1, z2, coff, tid, zidx, src.row_map());
  } else {
    finish_tile<TM, TN, Src::kPosMajorRows>(d, nsplit, acc, asum, want_rowsum, m0, n0, wm, wn, lr, lk, z1, z2, coff, zidx, bpre, src.row_map());
  }
#ifdef TAVSR_GEMM_TRACE
  __builtin_amdgcn_s_waitcnt(0);
  TAVSR_TRACE_AT(3)
  if (tid == 0) {
    unsigned int slot = atomicAdd(&g_trace_n, 1u);
    if (slot < (unsigned)kTraceMax) {
      for (int i = 0; i < 4; ++i) g_trace[slot][i] = tr_t[i];
      g_trace[slot][4] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | __builtin_amdgcn_s_getreg((31 << 11) | 4);
      g_trace[slot][5] = ((tr_c[2] - tr_c[1]) & 0xFFFFFFFFFFull) | ((unsigned long long)nk << 40);      // K loop: shader-clock cycles, K-steps executed above bit 40
    }
  }
#endif
}

// XCD-aware tile order: blocks b, b+8, b+16, ... share an XCD (its L2): give them neighbouring tiles.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Which tile a workgroup computes: the plain launches take xcd_remap's; the convolution launches (gemm_conv.hip) add their
// slice and tile orders, and the position-major forward carries its order behind the common arguments (GemmArgsOrd).
struct GemmArgsOrd;
template <int CONV, bool PM, bool CONV_LAUNCH = (CONV != 0 && CONV != 3)>
struct TileMap;
template <int CONV, bool PM>
struct TileMap<CONV, PM, false> {
  __device__ __forceinline__ static const GemmArgs& map(const GemmArgs& args, int& bid, int& zidx) {
    bid = xcd_remap(blockIdx.x, gridDim.x);
    zidx = blockIdx.z;
    return args;
  }
};

template <int BM, int BN, int WM, int WN, int S, int MINW, bool AK, bool BKM, int KW = 1, int CONV = 0, bool PM = false, bool X6 = false>
__global__ __launch_bounds__(WM* WN * KW * 64, MINW)
void gemm_glds_kernel(const std::conditional_t<PM && CONV == 1, GemmArgsOrd, GemmArgs> xargs) {
  int bid, zidx;
  const GemmArgs& args = TileMap<CONV, PM>::map(xargs, bid, zidx);
  glds_tile<BM, BN, WM, WN, S, AK, BKM, KW, CONV, PM, X6>(args.d, args.kchunk, args.nsplit, args.tiles_n, bid, args.vec_epi != 0, zidx,
                                                      args.n_big, args.kunit);
}

// ---------------------------------------------------------------------------------------------- host side, shared
template <typename F>
static int launch_layout(const tavsr_gemm_desc& d, F&& f) {
  if (!d.a_kmajor && !d.b_kmajor) return f(std::false_type{}, std::false_type{});
  if (!d.a_kmajor && d.b_kmajor) return f(std::false_type{}, std::true_type{});
  if (d.a_kmajor && d.b_kmajor) return f(std::true_type{}, std::true_type{});
  return f(std::true_type{}, std::false_type{});
}

struct Plan {
  int cfg, nsplit, kchunk;
  int n_big = 0, kunit = 0;     // two slice lengths (plan_conv): the first n_big slices hold kchunk + kunit
};
Plan plan(const tavsr_gemm_desc& d, bool allow_split, bool fast);                       // gemm.hip
int launch_epilogue(const GemmArgs& a, hipStream_t s);                                  // gemm.hip: the split-K slab sum, where there is one
Plan plan_conv(const tavsr_gemm_desc& d, bool can_split, int force_split = 0);          // gemm_conv.hip
int launch_conv(const tavsr_gemm_desc& d, const Plan& p, hipStream_t s);                // gemm_conv.hip

}  // namespace tavsr
