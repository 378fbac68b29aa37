// fp32 MFMA GEMM for gfx950 (v_mfma_f32_32x32x2_f32: exact f32, a k-ordered fmaf chain per output).
//
// One kernel family serves every contraction on the hot path:
//   NT  C[M,N] = A[M,K] * W[N,K]^T          torch Linear forward (espnet Linear leaves)
//   NN  C[M,N] = A[M,K] * B[K,N]            data gradients, attention P*V
//   TN  C[M,N] = A[K,M]^T * B[K,N]          weight gradients, dK/dV
// with two batch dimensions given by element strides (attention heads are addressed in place inside
// the [B*T, 3*256] QKV buffer: no transposes are ever materialised) and a fused epilogue
// (bias, ReLU/Swish/GELU, pre-activation store, residual + alpha, multiply by act'(z) for backward,
// row sums of op(A) = bias gradients of the weight-gradient GEMMs).
//
// Tiling: BM x BN x BK block tile, WM x WN wavefronts (64 lanes), each wave owns TM x TN MFMA tiles
// of 32x32.  LDS images (double buffered):
//   k-contiguous operand  : [row][BK+4]   filled by ds_write_b128, fragments read by ds_read_b128:
//                           lane (r = lane&31, h = lane>>5) gets k = 8g+4h .. 8g+4h+3 of row r, i.e. the
//                           operands of FOUR consecutive MFMAs in one LDS instruction (conflict free:
//                           144-byte row stride puts the 16 lanes of a b128 group on 16 distinct slots)
//   row-contiguous operand: [k][rows+4]   filled by ds_write_b128, fragments read by ds_read_b32 at the
//                           same k = 8g+4h+j (the MFMA sums over k in any order as long as A and B agree)
// Pipeline per K-step (register staging, one barrier): tile t+1, fetched from global memory during the
// previous step, is written to the other LDS buffer at the TOP of step t, the global loads of tile t+2
// are issued right behind it, and only then the MFMAs of tile t run - so the loads have a whole step to
// land and the LDS writes overlap the first MFMAs.
//
// Few-tile / long-K problems are split over K (gridDim.z slices): every slice stores its raw fp32
// accumulators to a slab and a second, fully parallel kernel sums the slabs in slice order (deterministic)
// and runs the epilogue.  (An in-kernel "last arriver reduces" variant was measured and lost: the reduction
// of a 64x64 tile over 24 slices by ONE workgroup serialises ~400 KB of reads - profiles/r01_gemm_sweep_v2.txt.)
// This unit: the plain, K-tail and grouped LDS-DMA kernels, the register-staged fallback, the epilogue kernels, the planner and
// the tavsr_gemm* entry points.  gemm_glds.h: the shared device code (the LDS-DMA ring glds_tile and its operand sources);
// gemm_conv.hip: the implicit-convolution and Conv3d-stem sources and their launches.
#include <algorithm>

#include <cstdlib>
#include "gemm_glds.h"

namespace tavsr {

// Fixed-order sum of the split-K slabs + the fused epilogue (same math as the in-kernel one); one thread per
// 4 consecutive columns when N % 4 == 0 (16-byte slab reads), else per element.
template <int V>
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const GemmArgs args) {
  const tavsr_gemm_desc& d = args.d;
  const int64_t mn = (int64_t)d.M * d.N;
  const int nbatch = d.nb1 * d.nb2;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  const int z = blockIdx.y, z1 = z / d.nb2, z2 = z % d.nb2;
  if (d.a_rowsum && z == 0 && i < d.M) {   // bias gradient: sum of the slices' row sums
    const float* rs = d.ws + (int64_t)args.nsplit * nbatch * mn;
    for (int q = 0; q < V && i + q < d.M; ++q) {
      float v = 0.f;
      for (int s = 0; s < args.nsplit; ++s) v += rs[(int64_t)s * d.M + i + q];
      d.a_rowsum[i + q] = d.alpha * v;
    }
  }
  if (i >= mn) return;
  const int m = (int)(i / d.N), n = (int)(i % d.N);
  float v[V];
#pragma unroll
  for (int q = 0; q < V; ++q) v[q] = 0.f;
  const float* p = d.ws + (int64_t)z * mn + i;
#pragma unroll 4
  for (int s = 0; s < args.nsplit; ++s) {
    if (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + (int64_t)s * nbatch * mn);
      v[0] += t.x; v[1 % V] += t.y; v[2 % V] += t.z; v[3 % V] += t.w;
    } else {
      v[0] += p[(int64_t)s * nbatch * mn];
    }
  }
  const int64_t o = z1 * d.sC1 + z2 * d.sC2 + (int64_t)m * d.ldc + n;
  const int64_t ro = z1 * d.sR1 + z2 * d.sR2 + (int64_t)m * d.ldr + n;
  uint32_t keep[4] = {1u, 1u, 1u, 1u};
  float inv_keep = 1.f;
  if (V == 4 && d.drop_p > 0.f) {        // the four columns of this thread are one Philox call (host: unbatched, N % 4 == 0)
    const uint64_t sd = d.drop_seed[0], ctr = (d.drop_offset >> 2) + (uint64_t)(i >> 2);
    const uint32_t thr = (uint32_t)((double)d.drop_p * 4294967296.0);
    uint32_t w[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), w);
#pragma unroll
    for (int q = 0; q < 4; ++q) keep[q] = w[q] >= thr;
    inv_keep = 1.f / (1.f - d.drop_p);
  }
#pragma unroll
  for (int q = 0; q < V; ++q) {
    float x = v[q];
    if (d.bias) x += d.bias[n + q];
    if (d.Z) d.Z[o + q] = x;
    x = act_fwd(d.act, x);
    if (d.DZ) x *= act_bwd(d.dact, d.DZ[o + q]);
    x = keep[q % 4] ? x * inv_keep : 0.f;
    x *= d.alpha;
    if (d.R) x += d.R[ro + q];
    d.C[o + q] = x;
  }
}

// MINW: waves per SIMD the register allocation must leave room for (blocks per CU x waves per block / 4):
// 4 blocks/CU for the 64x64 tile (its K-step is short: latency is hidden by co-resident blocks), 2 for the
// larger tiles (LDS admits two of them per CU).
template <int BM, int BN, int BK, int WM, int WN, int PF, int MINW, bool AK, bool BKM, bool VEC>
__global__ __launch_bounds__(WM* WN * 64, MINW)
void gemm_kernel(const GemmArgs args) {
  const tavsr_gemm_desc& d = args.d;
  constexpr int NT = WM * WN * 64;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int NG = BK / 8;
  using TA = Tile<BM, BK, AK>;
  using TB = Tile<BN, BK, BKM>;
  using LA = Loader<BM, BK, AK, VEC, NT>;
  using LB = Loader<BN, BK, BKM, VEC, NT>;
  constexpr int STAGE = TA::SIZE + TB::SIZE;  // stage s: A at smem + s*STAGE, B right after it
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lk = lane >> 5;

  // XCD-aware tile order: blocks b, b+8, b+16, ... share an XCD (its L2), give them neighbouring tiles.
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  // n fastest: neighbouring tiles share the A panel
  const int m0 = (bid / args.tiles_n) * BM;
  const int n0 = (bid % args.tiles_n) * BN;
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
  const bool want_rowsum = d.a_rowsum != nullptr && n0 == 0 && wn == 0;

  // split-K: slice z covers k in [kbeg, kend)
  const int kbeg = blockIdx.z * args.kchunk;
  const int kend = min(d.K, kbeg + args.kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;

  // a tile may use the unpredicated loads when it lies inside the operand (k-contiguous rows are clamped)
  const bool fastA = VEC && (AK ? (m0 + BM <= d.M) : true);
  const bool fastB = VEC && (BKM ? (n0 + BN <= d.N) : true);
  const int64_t kstepA = AK ? (int64_t)BK * d.lda : BK;
  const int64_t kstepB = BKM ? (int64_t)BK * d.ldb : BK;
  int64_t offA[LA::NV], offB[LB::NV];
  LA::offsets(d.lda, m0, d.M, tid, offA);
  LB::offsets(d.ldb, n0, d.N, tid, offB);
  const float* Ak = A + (AK ? (int64_t)kbeg * d.lda : kbeg);
  const float* Bk = B + (BKM ? (int64_t)kbeg * d.ldb : kbeg);

  // register ring: tile j is staged in set j % PF, PF K-steps before its MFMAs.
  float4 ra[PF][LA::NV], rb[PF][LB::NV];
  // A block whose tiles lie inside both operands and whose K range is whole K-steps runs a branch-free
  // steady-state loop (FAST): any branch inside the K loop splits it into basic blocks, and hipcc then
  // drains vmcnt/lgkmcnt at every join - the loads turn synchronous (measured: 2x on the whole kernel).
  const bool fast = fastA && fastB && (kend - kbeg) % BK == 0;
  auto load_tile = [&](int kt, float4 (&qa)[LA::NV], float4 (&qb)[LB::NV], auto fast_tag) {
    if constexpr (decltype(fast_tag)::value) {
      LA::load_fast(Ak + kt * kstepA, offA, qa);
      LB::load_fast(Bk + kt * kstepB, offB, qb);
    } else {
      const int k0 = kbeg + kt * BK;
      LA::load_safe(A, d.lda, m0, k0, d.M, kend, tid, qa);
      LB::load_safe(B, d.ldb, n0, k0, d.N, kend, tid, qb);
    }
  };
  const int arow = wm * TM * 32 + lr, brow = wn * TN * 32 + lr;
  // one K-step on LDS buffer (kt & 1); STORE: write ring set `rs` (tile kt+1) to the other buffer first,
  // LOAD: refill that set with tile kt+1+PF
  auto kstep = [&](int kt, float4 (&qa)[LA::NV], float4 (&qb)[LB::NV], bool do_store, bool do_load, auto fast_tag) {
    const int cur = kt & 1;
    const float* a_s = smem + cur * STAGE;
    const float* b_s = a_s + TA::SIZE;
    float af[2][TM][4], bf[2][TN][4];
#pragma unroll
    for (int i = 0; i < TM; ++i) read_frag<BM, BK, AK>(a_s, arow + i * 32, 0, lk, af[0][i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) read_frag<BN, BK, BKM>(b_s, brow + j * 32, 0, lk, bf[0][j]);
    if (do_store) {   // tile kt+1 -> the other buffer (its readers finished at the previous barrier)
      LA::store(smem + (cur ^ 1) * STAGE, tid, qa);
      LB::store(smem + (cur ^ 1) * STAGE + TA::SIZE, tid, qb);
      if (do_load) load_tile(kt + 1 + PF, qa, qb, fast_tag);
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int c = g & 1;
      if (g + 1 < NG) {
#pragma unroll
        for (int i = 0; i < TM; ++i) read_frag<BM, BK, AK>(a_s, arow + i * 32, g + 1, lk, af[c ^ 1][i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) read_frag<BN, BK, BKM>(b_s, brow + j * 32, g + 1, lk, bf[c ^ 1][j]);
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][i][kk], bf[c][j][kk], acc[i][j], 0, 0, 0);
      // row sums of op(A) ride along unconditionally (TM adds per 16*TM*TN MFMA cycles; no branch in the loop)
#pragma unroll
      for (int i = 0; i < TM; ++i) asum[i] += (af[c][i][0] + af[c][i][1]) + (af[c][i][2] + af[c][i][3]);
    }
    __syncthreads();
  };
  auto run_loop = [&](auto fast_tag) {
    if (nk > 0) {
      load_tile(0, ra[0], rb[0], fast_tag);
      LA::store(smem, tid, ra[0]);
      LB::store(smem + TA::SIZE, tid, rb[0]);
#pragma unroll
      for (int j = 1; j <= PF; ++j)
        if (j < nk) load_tile(j, ra[j % PF], rb[j % PF], fast_tag);
    }
    __syncthreads();
    int kt0 = 0;
    // steady state: every step stores and refills, no conditions
    for (; kt0 + 2 * PF < nk; kt0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) kstep(kt0 + u, ra[(u + 1) % PF], rb[(u + 1) % PF], true, true, fast_tag);
    }
    // drain: the last (at most 2*PF) steps
    for (; kt0 < nk; kt0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int kt = kt0 + u;
        if (kt < nk) kstep(kt, ra[(u + 1) % PF], rb[(u + 1) % PF], kt + 1 < nk, kt + 1 + PF < nk, fast_tag);
      }
    }
  };
  if (fast) run_loop(std::true_type{});
  else run_loop(std::false_type{});

  finish_tile<TM, TN>(d, args.nsplit, acc, asum, want_rowsum, m0, n0, wm, wn, lr, lk, z1, z2, coff, (int)blockIdx.z);
}

// ---------------------------------------------------------------------------------------------- K tail source
// 16 readable zero floats for LDS-DMA loads that must deliver zeros (K tails)
__device__ float g_zero_page[16];

// CONV 3 (K tail: K % 32 != 0), one operand: chunks whose first k lies at or past K are fetched from a zero page; a k-contiguous
// chunk that straddles K (K % 4 != 0) is fetched whole and its k >= K elements are zeroed in LDS before the last K-step.
template <int ROWS, bool KMAJOR, int NT, bool B_SIDE>
struct TailOperand : PlainOperand<ROWS, KMAJOR, NT, B_SIDE> {
  using P = PlainOperand<ROWS, KMAJOR, NT, B_SIDE>;
  int kofs[P::L::NR];       // first k, inside a K-step, of each chunk of this thread
  __device__ __forceinline__ explicit TailOperand(const TileCtx& c_) : P(c_) {
#pragma unroll
    for (int i = 0; i < P::L::NR; ++i) {
      const int q = i * NT + this->c.tid;
      kofs[i] = KMAJOR ? q / (ROWS / 4) : ((q & 7) ^ (((q >> 3) >> 1) & 7)) * 4;
    }
  }
  __device__ __forceinline__ void issue(int kt, float* img) {
    const TileCtx& c = this->c;
    const int kleft = c.kend - (c.kbeg + kt * kBK);                 // k values of this step that exist
    const float* g = this->gk + kt * this->kstep;
#pragma unroll
    for (int i = 0; i < P::L::NR; ++i) {
      const float* chunk = g + this->off[i];
      dma16(kofs[i] < kleft ? chunk : g_zero_page, img + (i * NT + c.wave * 64) * 4);
    }
  }
  // k-contiguous operand: the chunk that straddles K brought 1..3 elements of k >= K along: zero them (row r, element kk of
  // an image lives at r*32 + (((kk >> 2) ^ ((r >> 1) & 7)) << 2) + (kk & 3)); kt_len = the k values of the last K-step that exist
  __device__ __forceinline__ static void zero_past(float* img, int kt_len, int tid) {
    const int k4 = (kt_len + 3) & ~3;
    if (!KMAJOR)
      for (int r = tid; r < ROWS; r += NT)
        for (int kk = kt_len; kk < k4; ++kk) img[r * 32 + ((((kk >> 2) ^ ((r >> 1) & 7))) << 2) + (kk & 3)] = 0.f;
  }
};

// ... and both operands: the K-steps are rounded up, and the last one is mended in LDS where K % 4 != 0.
template <int BM, int BN, int NT, bool AK, bool BKM>
struct TailSource : SourceDefaults {
  using HA = TailOperand<BM, AK, NT, false>;
  using HB = TailOperand<BN, BKM, NT, true>;
  static constexpr int kDma = HA::kDma + HB::kDma;
  const TileCtx& c;
  HA a;
  HB b;
  __device__ __forceinline__ explicit TailSource(const TileCtx& c_) : c(c_), a(c_), b(c_) {}
  __device__ __forceinline__ int steps() const { return (c.kend - c.kbeg + kBK - 1) / kBK; }
  __device__ __forceinline__ void issue(int kt, float* stage) {
    a.issue(kt, stage);
    b.issue(kt, stage + BM * kBK);
  }
  // the slice's klen k values do not end on a 16-byte chunk, and kt is its last K-step
  __device__ __forceinline__ void fix_last(float* stage, int klen, int kt, int tid) const {
    const int kt_len = klen - kt * kBK;
    HA::zero_past(stage, kt_len, tid);
    HB::zero_past(stage + BM * kBK, kt_len, tid);
    __syncthreads();
  }
};
template <int BM, int BN, int NT, bool AK, bool BKM>
struct SourceFor<3, false, BM, BN, NT, AK, BKM> {
  using type = TailSource<BM, BN, NT, AK, BKM>;
};

// Grouped launch: up to kMaxGroup independent problems of one layout share ONE grid (tile ranges by prefix sums).
// The weight gradients of a layer have 16-128 tiles each: alone they need a K split (slabs + a second launch);
// together they fill the chip without one.
constexpr int kMaxGroup = 12;
struct GroupArgs {
  tavsr_gemm_desc d[kMaxGroup];
  int tile_start[kMaxGroup + 1];
  int tiles_n[kMaxGroup];
  int n;
  int vec_epi;    // every problem of the group qualifies for finish_tile_vec
};

template <int BM, int BN, int WM, int WN, int S, int MINW, bool AK, bool BKM>
__global__ __launch_bounds__(WM* WN * 64, MINW)
void gemm_glds_grouped_kernel(const GroupArgs g) {
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  int pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i)
    if (i < g.n && bid >= g.tile_start[i]) pi = i;
  glds_tile<BM, BN, WM, WN, S, AK, BKM>(g.d[pi], g.d[pi].K, 1, g.tiles_n[pi], bid - g.tile_start[pi], g.vec_epi != 0, 0);
}

// ---------------------------------------------------------------------------------------------- host side
struct Cfg {
  int bm, bn, wm, wn, stages;
};
// LDS-DMA tile configurations (index = cfg id of tavsr_gemm_tune); id kFallbackCfg = the register-staged,
// fully predicated 64x64 kernel that serves unaligned operands, K tails and ragged row-contiguous operands.
static const Cfg kCfgs[] = {
    {128, 128, 2, 2, 3},   // 0: wave tile 64x64, 96 KB LDS, one block per CU
    {128, 128, 2, 4, 3},   // 1: 8 waves, wave tile 64x32 (two waves per SIMD inside the block)
    {128, 64, 2, 2, 3},    // 2: wave tile 64x32, 72 KB, two blocks per CU
    {64, 128, 2, 2, 3},    // 3: wave tile 32x64
    {64, 64, 2, 2, 3},     // 4: wave tile 32x32, 48 KB, three blocks per CU
    {64, 64, 2, 2, 4},     // 5: wave tile 32x32, four stages (three tiles in flight), two blocks per CU
    {128, 64, 2, 2, 4},    // 6: wave tile 64x32, four stages, one block per CU
    {64, 64, 2, 2, 3},     // 7: as 4 with the K-step split over 2 wave sets (8 waves)
    {64, 64, 2, 2, 2},     // 8: two stages (32 KB): five blocks per CU
};
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
constexpr int kFallbackCfg = 9;

// tavsr_gemm_ln: the LayerNorm that follows a Linear, taken where the result row is finished.  A one-token step of a batched search
// (640 hypothesis rows) runs its N = 256 / 512 projections with K split over workgroups: the slabs are summed by an epilogue launch
// and the next block's LayerNorm is another launch over the same rows - 38 + 38 launches of ~5 us per token at batch 64.  Here one
// wave per row sums the slabs (fixed order), applies the same epilogue arithmetic as splitk_epilogue_kernel, stores C and, with the
// row still in registers, its LayerNorm (two-pass statistics, as layernorm_fwd_kernel).  nsplit == 1: C is final; the wave reads it.
struct LnTail {
  const float* gamma; const float* beta; float eps; float* out; int64_t ld;
};
static const LnTail* g_ln_tail = nullptr;      // set by tavsr_gemm_ln around its run(): the library is not re-entrant; launch_epilogue reads it

constexpr int kLnTailMaxN = 2048;
__global__ __launch_bounds__(256) void epilogue_ln_kernel(const GemmArgs args, const LnTail ln) {
  const tavsr_gemm_desc& d = args.d;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + wave;
  if (m >= d.M) return;
  constexpr int Q = kLnTailMaxN / 256;             // float4s per lane
  const int n4 = d.N >> 2;
  const int64_t mn = (int64_t)d.M * d.N;
  float4 x[Q];
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c4 = lane + 64 * q;
    x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < n4) {
      const int n = 4 * c4;
      const int64_t o = (int64_t)m * d.ldc + n;
      float4 v;
      if (args.nsplit > 1) {
        v = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = d.ws + (int64_t)m * d.N + n;
        for (int sidx = 0; sidx < args.nsplit; ++sidx) {
          const float4 t = *reinterpret_cast<const float4*>(p + (int64_t)sidx * mn);
          v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float y = e[k];
          if (d.bias) y += d.bias[n + k];
          y = act_fwd(d.act, y);
          y *= d.alpha;
          if (d.R) y += d.R[(int64_t)m * d.ldr + n + k];
          e[k] = y;
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
        *reinterpret_cast<float4*>(d.C + o) = v;
      } else {
        v = *reinterpret_cast<const float4*>(d.C + o);
      }
      x[q] = v;
      sum += (v.x + v.y) + (v.z + v.w);
    }
  }
  const float mean = wave_sum(sum) / (float)d.N;
  float sq = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if (lane + 64 * q < n4) {
      const float a = x[q].x - mean, b = x[q].y - mean, c = x[q].z - mean, e = x[q].w - mean;
      sq += (a * a + b * b) + (c * c + e * e);
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)d.N + ln.eps);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c4 = lane + 64 * q;
    if (c4 < n4) {
      const float4 g = *reinterpret_cast<const float4*>(ln.gamma + 4 * c4), b = *reinterpret_cast<const float4*>(ln.beta + 4 * c4);
      *reinterpret_cast<float4*>(ln.out + (int64_t)m * ln.ld + 4 * c4) =
          make_float4((x[q].x - mean) * rstd * g.x + b.x, (x[q].y - mean) * rstd * g.y + b.y, (x[q].z - mean) * rstd * g.z + b.z,
                      (x[q].w - mean) * rstd * g.w + b.w);
    }
  }
}

int launch_epilogue(const GemmArgs& a, hipStream_t s) {
  const tavsr_gemm_desc& d = a.d;
  if (g_ln_tail) {                 // tavsr_gemm_ln: slab sum + epilogue + the next LayerNorm, one wave per row
    hipLaunchKernelGGL(epilogue_ln_kernel, dim3(cdiv(d.M, 4)), dim3(256), 0, s, a, *g_ln_tail);
    TAVSR_LAUNCH_CHECK();
    return TAVSR_OK;
  }
  if (a.nsplit > 1) {
    const int64_t mn = (int64_t)d.M * d.N;
    if (d.N % 4 == 0)
      hipLaunchKernelGGL(splitk_epilogue_kernel<4>, dim3(cdiv(mn / 4, 256), d.nb1 * d.nb2), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(splitk_epilogue_kernel<1>, dim3(cdiv(mn, 256), d.nb1 * d.nb2), dim3(256), 0, s, a);
    TAVSR_LAUNCH_CHECK();
  }
  return TAVSR_OK;
}

template <int BM, int BN, int WM, int WN, int S, int MINW, int KW = 1>
static int launch_glds(const tavsr_gemm_desc& d, int nsplit, int kchunk, hipStream_t s) {
  GemmArgs a{d, kchunk, nsplit, cdiv(d.M, BM), cdiv(d.N, BN), (int)vec_epi_ok(d)};
  dim3 grid(a.tiles_m * a.tiles_n, d.nb1 * d.nb2, nsplit);
  int rc = launch_layout(d, [&](auto ak, auto bk) {
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, S, MINW, decltype(ak)::value, decltype(bk)::value, KW>), grid,
                       dim3(WM * WN * KW * 64), 0, s, a);
    TAVSR_LAUNCH_CHECK();
    return (int)TAVSR_OK;
  });
  return rc ? rc : launch_epilogue(a, s);
}

static int launch_fallback(const tavsr_gemm_desc& d, bool vec, int nsplit, int kchunk, hipStream_t s) {
  GemmArgs a{d, kchunk, nsplit, cdiv(d.M, 64), cdiv(d.N, 64), 0};
  dim3 grid(a.tiles_m * a.tiles_n, d.nb1 * d.nb2, nsplit);
  int rc = launch_layout(d, [&](auto ak, auto bk) {
    if (vec)
      hipLaunchKernelGGL((gemm_kernel<64, 64, 32, 2, 2, 2, 4, decltype(ak)::value, decltype(bk)::value, true>), grid,
                         dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((gemm_kernel<64, 64, 32, 2, 2, 2, 4, decltype(ak)::value, decltype(bk)::value, false>), grid,
                         dim3(256), 0, s, a);
    TAVSR_LAUNCH_CHECK();
    return (int)TAVSR_OK;
  });
  return rc ? rc : launch_epilogue(a, s);
}

static int launch_tail(const tavsr_gemm_desc& d, int nsplit, int kchunk, hipStream_t s) {
  GemmArgs a{d, kchunk, nsplit, cdiv(d.M, 64), cdiv(d.N, 64), (int)vec_epi_ok(d)};
  dim3 grid(a.tiles_m * a.tiles_n, d.nb1 * d.nb2, nsplit);
  int rc = launch_layout(d, [&](auto ak, auto bk) {
    hipLaunchKernelGGL((gemm_glds_kernel<64, 64, 2, 2, 2, 5, decltype(ak)::value, decltype(bk)::value, 1, 3>), grid, dim3(256), 0, s, a);
    TAVSR_LAUNCH_CHECK();
    return (int)TAVSR_OK;
  });
  return rc ? rc : launch_epilogue(a, s);
}

static int launch(int cfg, const tavsr_gemm_desc& d, bool vec, int nsplit, int kchunk, hipStream_t s) {
  switch (cfg) {
    case 0: return launch_glds<128, 128, 2, 2, 3, 1>(d, nsplit, kchunk, s);
    case 1: return launch_glds<128, 128, 2, 4, 3, 2>(d, nsplit, kchunk, s);
    case 2: return launch_glds<128, 64, 2, 2, 3, 2>(d, nsplit, kchunk, s);
    case 3: return launch_glds<64, 128, 2, 2, 3, 2>(d, nsplit, kchunk, s);
    case 4: return launch_glds<64, 64, 2, 2, 3, 3>(d, nsplit, kchunk, s);
    case 5: return launch_glds<64, 64, 2, 2, 4, 2>(d, nsplit, kchunk, s);
    case 6: return launch_glds<128, 64, 2, 2, 4, 1>(d, nsplit, kchunk, s);
    case 7: return launch_glds<64, 64, 2, 2, 3, 4, 2>(d, nsplit, kchunk, s);
    case 8: return launch_glds<64, 64, 2, 2, 2, 5>(d, nsplit, kchunk, s);
    default: return launch_fallback(d, vec, nsplit, kchunk, s);
  }
}

// Can the LDS-DMA kernel take this problem?  (unpredicated 16-byte loads: aligned operands, whole K-steps per
// K slice, row-contiguous operands with a row count that is a multiple of 4)
static bool glds_ok(const tavsr_gemm_desc& d, bool vec) {
  return vec && d.K % 32 == 0 && d.K >= 32 && (!d.a_kmajor || d.M % 4 == 0) && (!d.b_kmajor || d.N % 4 == 0);
}

// K % 32 != 0 on the LDS-DMA kernel (tail variant): 16-byte chunks past K come from a zero page; a k-contiguous operand
// must hold the (up to 3) elements between K and the next multiple of 4 inside its rows (ld >= roundup4(K))
static bool tail_ok(const tavsr_gemm_desc& d, bool vec) {
  const int64_t k4 = (d.K + 3) / 4 * 4;
  return vec && d.K % 32 != 0 && d.K >= 32 && (!d.a_kmajor || d.M % 4 == 0) && (!d.b_kmajor || d.N % 4 == 0) &&
         (d.a_kmajor || d.lda >= k4) && (d.b_kmajor || d.ldb >= k4) && d.conv_mode == 0;
}

// Planner (fitted to profiles/r01_gemm_sweep_v3/v4.txt and end-to-end A/B runs, MI355X).  The 64x64 tile wins or ties every
// hot-path shape (larger tiles lose more to tile quantisation at M = 3168 than they gain).  Few-tile, long-K problems
// (weight gradients: K = B*T; the N = 256 projections with K >= 2048) are split over K until about 1000 blocks exist
// (four of the five block slots of every CU: 5 slices for the 200-tile shapes); more slices than that cost more in
// slab traffic than they gain in balance.
Plan plan(const tavsr_gemm_desc& d, bool allow_split, bool fast) {
  const long nbatch = (long)d.nb1 * d.nb2;
  Plan p{kFallbackCfg, 1, d.K};
  const long tiles = (long)cdiv(d.M, 64) * cdiv(d.N, 64) * nbatch;
  // tile variant: two LDS stages (32 KB, five blocks per CU cover each other's epilogues).  The K-step-split variant
  // (cfg 7) wins isolated one-block-per-CU launches by 5-8 % but loses inside the two-stream step (end-to-end A/B).
  // (tavsr_gemm_tune forces a variant for tests / sweeps)
  p.cfg = fast ? 8 : kFallbackCfg;
  if (!allow_split || tiles >= 384 || d.K < 512) return p;
  if (d.K <= 1024 && tiles >= 150) return p;
  constexpr long target = 1000L;
  long want = std::min<long>((target + tiles / 2) / tiles, d.K / 256);
  if (want < 2) return p;
  p.kchunk = cdiv(cdiv(d.K, want), 32) * 32;
  p.nsplit = cdiv(d.K, p.kchunk);
  if (p.nsplit < 2) p = Plan{p.cfg, 1, d.K};
  return p;
}

// Descriptor normalisation of every entry point: absent batch dimensions count 1, an absent residual has no strides.
static void normalise(tavsr_gemm_desc& d) {
  if (d.nb1 <= 0) d.nb1 = 1;
  if (d.nb2 <= 0) d.nb2 = 1;
  if (d.R == nullptr) { d.ldr = 0; d.sR1 = d.sR2 = 0; }
}

// vector (16-B) operand loads need aligned bases, leading dims and, where the problem may be batched, batch strides
static bool vec_operands(const tavsr_gemm_desc& d, bool batched = true) {
  return aligned16(d.A) && aligned16(d.B) && d.lda % 4 == 0 && d.ldb % 4 == 0 &&
         (!batched || (d.sA1 % 4 == 0 && d.sA2 % 4 == 0 && d.sB1 % 4 == 0 && d.sB2 % 4 == 0));
}

static int64_t ws_floats_for(const tavsr_gemm_desc& d, int nsplit) {
  if (nsplit <= 1) return 0;
  return (int64_t)nsplit * d.nb1 * d.nb2 * d.M * d.N + (d.a_rowsum ? (int64_t)nsplit * d.M : 0);
}

// Epilogue of the activations the GEMM kernels' switch does not hold (tanh / hardtanh / SELU, common.h): the product was stored
// with its bias only (C, and Z); this applies act, act'(DZ), the dropout mask, alpha and the residual in the fused epilogue's
// order and with its mask (word n & 3 of Philox counter drop_offset/4 + (m*N + n)/4).  One thread per 4 columns of a row.
__global__ __launch_bounds__(256) void ext_epilogue_kernel(const tavsr_gemm_desc d) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= (int64_t)d.M * d.N) return;
  const int m = (int)(i / d.N), n = (int)(i % d.N);
  uint32_t keep[4] = {1u, 1u, 1u, 1u};
  float inv_keep = 1.f;
  if (d.drop_p > 0.f) {
    const uint64_t sd = d.drop_seed[0], ctr = (d.drop_offset >> 2) + (uint64_t)(i >> 2);
    const uint32_t thr = (uint32_t)((double)d.drop_p * 4294967296.0);
    uint32_t w[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), w);
#pragma unroll
    for (int q = 0; q < 4; ++q) keep[q] = w[q] >= thr;
    inv_keep = 1.f / (1.f - d.drop_p);
  }
  float* c = d.C + (int64_t)m * d.ldc + n;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float x = act_fwd_all(d.act, c[q]);
    if (d.DZ) x *= act_bwd_all(d.dact, d.DZ[(int64_t)m * d.ldc + n + q]);
    x = keep[q] ? x * inv_keep : 0.f;
    x *= d.alpha;
    if (d.R) x += d.R[(int64_t)m * d.ldr + n + q];
    c[q] = x;
  }
}

static int run(const tavsr_gemm_desc* dp, int force_cfg, int force_split, hipStream_t s);

// act or dact among tanh / hardtanh / SELU: the product through the unchanged kernels with bias (and Z) only, then
// ext_epilogue_kernel over C - one more pass over the result; the encoders' feed-forward blocks take it only off the
// streaming route (csrc/ffn2.hip holds these activations in its own instantiations).
static int run_ext(const tavsr_gemm_desc* dp, int force_cfg, int force_split, hipStream_t s) {
  const tavsr_gemm_desc& d = *dp;
  TAVSR_REQUIRE(d.nb1 * d.nb2 <= 1 && d.conv_mode == 0 && !d.a_rowsum && !d.rowstat && !g_ln_tail, TAVSR_EUNSUPPORTED,
                "tavsr_gemm: tanh / hardtanh / SELU epilogues on plain unbatched products only (no row sums or statistics)");
  TAVSR_REQUIRE((act_base_ok(d.act) || act_is_ext(d.act)) && (!d.DZ || act_base_ok(d.dact) || act_is_ext(d.dact)), TAVSR_EINVAL,
                "tavsr_gemm: unknown activation %d / %d", d.act, d.dact);
  TAVSR_REQUIRE(d.N % 4 == 0 && (!d.R || d.R != d.C) && (!d.DZ || d.DZ != d.C), TAVSR_EUNSUPPORTED,
                "tavsr_gemm: tanh / hardtanh / SELU epilogues need N %% 4 == 0 and R, DZ apart from C");
  TAVSR_REQUIRE(d.drop_p == 0.f || d.drop_seed, TAVSR_EINVAL, "tavsr_gemm: dropout needs a device seed");
  if (d.M == 0 || d.N == 0) return TAVSR_OK;
  tavsr_gemm_desc g = d;
  g.act = g.dact = TAVSR_ACT_NONE;
  g.DZ = nullptr; g.R = nullptr; g.alpha = 1.f; g.drop_p = 0.f; g.drop_seed = nullptr;
  int rc = run(&g, force_cfg, force_split, s);
  if (rc != TAVSR_OK) return rc;
  hipLaunchKernelGGL(ext_epilogue_kernel, dim3(cdiv((int64_t)d.M * d.N / 4, 256)), dim3(256), 0, s, d);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

static int run(const tavsr_gemm_desc* dp, int force_cfg, int force_split, hipStream_t s) {
  TAVSR_REQUIRE(dp != nullptr, TAVSR_EINVAL, "tavsr_gemm: null descriptor");
  if (act_is_ext(dp->act) || (dp->DZ && act_is_ext(dp->dact))) return run_ext(dp, force_cfg, force_split, s);
  tavsr_gemm_desc d = *dp;
  TAVSR_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0, TAVSR_EINVAL, "tavsr_gemm: negative dims");
  normalise(d);
  if (d.M == 0 || d.N == 0) return TAVSR_OK;
  TAVSR_REQUIRE(d.A && d.B && d.C, TAVSR_EINVAL, "tavsr_gemm: null operand");
  TAVSR_REQUIRE((long)d.nb1 * d.nb2 <= 65535, TAVSR_EINVAL, "tavsr_gemm: batch too large");
  TAVSR_REQUIRE(d.a_rowsum == nullptr || d.nb1 * d.nb2 == 1, TAVSR_EUNSUPPORTED,
                "tavsr_gemm: a_rowsum needs an unbatched problem");
  const bool vec = vec_operands(d);
  const bool can_split = d.ws != nullptr;
  const bool fast = glds_ok(d, vec);
  if (d.conv_mode != 0) {       // implicit 3x3/s1/p1 convolution: only the LDS-DMA kernel reads images as patch operands
    TAVSR_REQUIRE(d.conv_mode == 1 || d.conv_mode == 2 || (d.conv_mode >= 4 && d.conv_mode <= 7), TAVSR_EINVAL,
                  "tavsr_gemm: conv_mode must be 0, 1, 2 or 4..7");
    TAVSR_REQUIRE(d.drop_p == 0.f, TAVSR_EUNSUPPORTED, "tavsr_gemm: no epilogue dropout on convolution operands");
    TAVSR_REQUIRE(d.conv_zero && aligned16(d.conv_zero) && d.conv_H > 0 && d.conv_W > 0 && d.conv_C > 0, TAVSR_EINVAL,
                  "tavsr_gemm: conv needs H, W, C and a 16-byte aligned zero page");
    TAVSR_REQUIRE(d.nb1 * d.nb2 == 1 && fast && force_cfg < 0, TAVSR_EUNSUPPORTED,
                  "tavsr_gemm: conv operands need an unbatched, aligned problem with K %% 32 == 0");
    if (d.conv_mode >= 6) {       // Conv3d stem over padded clips [clips][conv_C = T + 5][conv_H = H + 6][conv_W = W + 8], 288 tap columns
      TAVSR_REQUIRE(d.conv_C > 5 && d.conv_H > 6 && d.conv_W > 8 && (d.conv_H - 6) % 2 == 0 && (d.conv_W - 8) % 2 == 0 &&
                        d.conv_W % 4 == 0, TAVSR_EINVAL, "tavsr_gemm: padded stem clips are [T + 5][H + 6][W + 8], H and W even");
      const int64_t per_clip = (int64_t)(d.conv_C - 5) * ((d.conv_H - 6) / 2) * ((d.conv_W - 8) / 2);
      const int64_t pixels = d.conv_mode == 6 ? d.M : d.K;
      TAVSR_REQUIRE(pixels % per_clip == 0 && pixels / per_clip * d.conv_C * d.conv_H * d.conv_W < (1ll << 31), TAVSR_EINVAL,
                    "tavsr_gemm: stem rows must be whole clips (fewer than 2^31 padded input pixels)");
      if (d.conv_mode == 6)
        TAVSR_REQUIRE(!d.a_kmajor && !d.b_kmajor && d.K == 288 && d.ldb >= 288, TAVSR_EUNSUPPORTED,
                      "tavsr_gemm: conv mode 6 needs the NT layout with K = 288 (35 x 8 tap columns + padding)");
      else
        TAVSR_REQUIRE(d.a_kmajor && d.b_kmajor && d.N == 288 && d.M % 4 == 0, TAVSR_EUNSUPPORTED,
                      "tavsr_gemm: conv mode 7 needs the TN layout with N = 288 (35 x 8 tap columns + padding)");
    } else if (d.conv_mode >= 4) {       // Conv3d stem: conv_H x conv_W input frames, conv_C frames per clip, 245 taps padded to 256
      const int64_t per_frame = (int64_t)((d.conv_H - 1) / 2 + 1) * ((d.conv_W - 1) / 2 + 1);
      const int64_t pixels = d.conv_mode == 4 ? d.M : d.K;
      TAVSR_REQUIRE(pixels % (per_frame * d.conv_C) == 0 && d.conv_C < 1024 && d.conv_H < 1000 && d.conv_W < 1000 &&
                        pixels / per_frame * d.conv_H * d.conv_W < (1ll << 31),
                    TAVSR_EINVAL, "tavsr_gemm: stem rows must be whole clips of conv_C frames (fewer than 2^31 input pixels)");
      if (d.conv_mode == 4)
        TAVSR_REQUIRE(!d.a_kmajor && !d.b_kmajor && d.K == 256 && d.ldb >= 256, TAVSR_EUNSUPPORTED,
                      "tavsr_gemm: conv mode 4 needs the NT layout with K = 256 (245 taps + padding)");
      else
        TAVSR_REQUIRE(d.a_kmajor && d.b_kmajor && d.N == 256 && d.M % 4 == 0, TAVSR_EUNSUPPORTED,
                      "tavsr_gemm: conv mode 5 needs the TN layout with N = 256 (245 taps + padding)");
    } else {
      const int cs = d.conv_stride > 1 ? d.conv_stride : 1, taps = d.conv_taps == 1 ? 1 : 9;
      TAVSR_REQUIRE(d.conv_taps == 0 || d.conv_taps == 1 || d.conv_taps == 9 || d.conv_taps == 90, TAVSR_EINVAL,
                    "tavsr_gemm: conv_taps must be 1, 9 or 90 (3x3 without padding)");
      const int p0 = d.conv_taps == 90 ? 1 : 0;
      TAVSR_REQUIRE(!p0 || (d.conv_H >= 3 && d.conv_W >= 3), TAVSR_EINVAL, "tavsr_gemm: an unpadded 3x3 window needs a 3x3 image");
      const int64_t pixels = d.conv_mode == 1 ? d.M : d.K;       // output pixels
      const int64_t per_image = (int64_t)((d.conv_H - 1 - 2 * p0) / cs + 1) * ((d.conv_W - 1 - 2 * p0) / cs + 1);
      TAVSR_REQUIRE(pixels % per_image == 0, TAVSR_EINVAL, "tavsr_gemm: conv rows are not whole images");
      if (d.conv_mode == 1)
        TAVSR_REQUIRE(!d.a_kmajor && d.K == taps * d.conv_C && d.conv_C % 32 == 0 && d.lda == d.conv_C, TAVSR_EUNSUPPORTED,
                      "tavsr_gemm: conv mode 1 needs a row-major image operand A, K = taps * C, C %% 32 == 0");
      else
        TAVSR_REQUIRE(d.a_kmajor && d.b_kmajor && d.N == taps * d.conv_C && d.conv_C % 64 == 0 && d.ldb == d.conv_C,
                      TAVSR_EUNSUPPORTED, "tavsr_gemm: conv mode 2 needs the TN layout, N = taps * C, C %% 64 == 0");
    }
    Plan pc = plan_conv(d, can_split, force_split);
    if (pc.nsplit > 1 && d.ws_floats < ws_floats_for(d, pc.nsplit)) pc = plan(d, false, true);
    return launch_conv(d, pc, s);
  }
  const bool tail = !fast && force_cfg < 0 && tail_ok(d, vec);
  if (d.drop_p > 0.f) {
    TAVSR_REQUIRE(d.drop_p < 1.f && d.drop_seed && d.drop_offset % 4 == 0, TAVSR_EINVAL,
                  "tavsr_gemm: dropout needs p in (0, 1), a device seed and an offset %% 4 == 0");
    TAVSR_REQUIRE((fast || tail) && force_cfg < 0 && d.nb1 * d.nb2 == 1 && vec_epi_ok(d), TAVSR_EUNSUPPORTED,
                  "tavsr_gemm: epilogue dropout needs an unbatched problem on the 16-byte path");
  }
  TAVSR_REQUIRE((d.rowdot_a == nullptr) == (d.rowdot_b == nullptr) && (!d.rowdot_a || d.rowstat), TAVSR_EINVAL,
                "tavsr_gemm: rowdot_a and rowdot_b go together, with rowstat as their output");
  if (d.rowstat) {
    TAVSR_REQUIRE(fast && force_cfg < 0 && d.nb1 * d.nb2 == 1 && vec_epi_ok(d) && aligned16(d.rowstat) && aligned16(d.rowdot_a) &&
                      aligned16(d.rowdot_b), TAVSR_EUNSUPPORTED,
                  "tavsr_gemm: row statistics / row dots need an unbatched problem on the 16-byte path");
    return launch(8, d, vec, 1, d.K, s);             // 64-wide tiles, no K split: the statistics are taken where the tile is stored
  }
  Plan p = plan(d, can_split, fast || tail);
  if (tail) {
    if (p.nsplit > 1 && d.ws_floats < ws_floats_for(d, p.nsplit)) p = plan(d, false, true);
    return launch_tail(d, p.nsplit, p.kchunk, s);
  }
  if (force_cfg >= 0) {
    TAVSR_REQUIRE(force_cfg < kNumCfgs || force_cfg == kFallbackCfg, TAVSR_EINVAL, "tavsr_gemm_tune: cfg %d out of range",
                  force_cfg);
    p.cfg = fast ? force_cfg : kFallbackCfg;
    const int bk = 32;
    int ns = std::max(1, force_split);
    p.kchunk = cdiv(cdiv(d.K, ns), bk) * bk;
    p.nsplit = std::max(1, cdiv(d.K, p.kchunk));
  }
  if (p.nsplit > 1) {
    if (!can_split || d.ws_floats < ws_floats_for(d, p.nsplit)) {
      TAVSR_REQUIRE(force_cfg < 0, TAVSR_EINVAL, "tavsr_gemm_tune: workspace too small for the forced split");
      p = plan(d, false, fast);
    }
  }
  return launch(p.cfg, d, vec, p.nsplit, p.kchunk, s);
}

}  // namespace tavsr

extern "C" int tavsr_gemm(const tavsr_gemm_desc* dp, tavsr_stream_t stream) {
  return tavsr::run(dp, -1, 0, static_cast<hipStream_t>(stream));
}

extern "C" int tavsr_gemm_ln(const tavsr_gemm_desc* dp, const float* gamma, const float* beta, float eps, float* ln_out, int64_t ld_ln,
                             tavsr_stream_t stream) {
  using namespace tavsr;
  TAVSR_REQUIRE(dp && gamma && beta && ln_out, TAVSR_EINVAL, "tavsr_gemm_ln: null pointer");
  const tavsr_gemm_desc& d = *dp;
  TAVSR_REQUIRE(d.nb1 * d.nb2 <= 1 && d.conv_mode == 0 && d.drop_p == 0.f && !d.Z && !d.DZ && !d.a_rowsum && !d.rowstat,
                TAVSR_EUNSUPPORTED, "tavsr_gemm_ln: a plain unbatched Linear (bias / activation / alpha / residual) only");
  TAVSR_REQUIRE(d.N % 4 == 0 && d.N <= kLnTailMaxN && d.ldc % 4 == 0 && ld_ln % 4 == 0 && (!d.R || d.ldr % 4 == 0) &&
                    aligned16(d.C) && aligned16(ln_out) && aligned16(gamma) && aligned16(beta) && ln_out != d.C,
                TAVSR_EALIGN, "tavsr_gemm_ln: N %% 4 == 0, N <= %d, 16-byte aligned rows of C / ln_out / gamma / beta", kLnTailMaxN);
  const LnTail ln{gamma, beta, eps, ln_out, ld_ln};
  g_ln_tail = &ln;
  const int rc = run(dp, -1, 0, static_cast<hipStream_t>(stream));
  g_ln_tail = nullptr;
  return rc;
}

extern "C" int tavsr_gemm_grouped(const tavsr_gemm_desc* descs, int32_t n, tavsr_stream_t stream) {
  using namespace tavsr;
  TAVSR_REQUIRE(descs != nullptr && n >= 1 && n <= kMaxGroup, TAVSR_EINVAL, "tavsr_gemm_grouped: 1..%d problems", kMaxGroup);
  GroupArgs g;
  g.n = n;
  int total = 0;
  for (int i = 0; i < n; ++i) {
    tavsr_gemm_desc d = descs[i];
    normalise(d);
    TAVSR_REQUIRE(d.A && d.B && d.C && d.M > 0 && d.N > 0 && d.K > 0, TAVSR_EINVAL, "tavsr_gemm_grouped: bad problem %d", i);
    TAVSR_REQUIRE(d.a_kmajor == descs[0].a_kmajor && d.b_kmajor == descs[0].b_kmajor, TAVSR_EUNSUPPORTED,
                  "tavsr_gemm_grouped: all problems must share one layout");
    TAVSR_REQUIRE(d.nb1 * d.nb2 == 1 && d.drop_p == 0.f, TAVSR_EUNSUPPORTED, "tavsr_gemm_grouped: unbatched problems without epilogue dropout only");
    TAVSR_REQUIRE(glds_ok(d, vec_operands(d, false)), TAVSR_EUNSUPPORTED,      // (no batch strides: batched problems were refused above)
                  "tavsr_gemm_grouped: problem %d needs the predicated kernel (alignment / K %% 32 / rows %% 4)", i);
    g.d[i] = d;
    g.tile_start[i] = total;
    g.tiles_n[i] = cdiv(d.N, 64);
    total += cdiv(d.M, 64) * g.tiles_n[i];
  }
  for (int i = n; i <= kMaxGroup; ++i) g.tile_start[i] = total;
  g.vec_epi = 1;
  for (int i = 0; i < n; ++i) g.vec_epi &= (int)vec_epi_ok(g.d[i]);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = launch_layout(descs[0], [&](auto ak, auto bk) {
    hipLaunchKernelGGL((gemm_glds_grouped_kernel<64, 64, 2, 2, 2, 5, decltype(ak)::value, decltype(bk)::value>), dim3(total),
                       dim3(256), 0, s, g);
    TAVSR_LAUNCH_CHECK();
    return (int)TAVSR_OK;
  });
  return rc;
}

extern "C" int tavsr_gemm_tune(const tavsr_gemm_desc* dp, int32_t cfg, int32_t nsplit, tavsr_stream_t stream) {
  return tavsr::run(dp, cfg, nsplit, static_cast<hipStream_t>(stream));
}

// Workspace the planner would like for this problem: floats of split-K slabs (0: no split) and, through
// *sync_ints, the number of zero-initialised int32 tile counters.
extern "C" int64_t tavsr_gemm_ws(const tavsr_gemm_desc* dp) {
  using namespace tavsr;
  if (!dp) return 0;
  tavsr_gemm_desc d = *dp;
  normalise(d);
  if (d.M <= 0 || d.N <= 0) return 0;
  const bool vec = vec_operands(d);
  Plan p = d.conv_mode != 0 ? plan_conv(d, true) : plan(d, true, glds_ok(d, vec) || tail_ok(d, vec));
  return ws_floats_for(d, p.nsplit);
}

#ifdef TAVSR_GEMM_TRACE
// Debug build only: copy out (and reset) the per-workgroup phase timestamps of both units. out: [max_rows][6] uint64. Returns rows.
extern "C" int tavsr_gemm_trace_read(unsigned long long* out, int max_rows) {
  const int n0 = tavsr::trace_read_unit(out, max_rows);
  if (n0 < 0) return -1;
  const int n1 = tavsr::conv_trace_read(out + (size_t)n0 * 6, max_rows - n0);
  return n1 < 0 ? -1 : n0 + n1;
}
#endif
