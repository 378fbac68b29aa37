// Implicit convolutions and the Conv3d stem on the LDS-DMA GEMM (gemm_glds.h: the ring, the epilogues, struct PosMajor): their
// operand sources - the image is read in place as a patch operand, no im2col matrix in HBM -, the tile and slice orders of the
// position-major launches, the convolution planner and launcher.  tavsr_gemm (gemm.hip) validates the descriptor and calls
// plan_conv / launch_conv.
#include <algorithm>
#include <vector>

#include "gemm_glds.h"

namespace tavsr {

// Tile order of the position-major forward / data gradient.  The hardware deals the workgroups of a launch to the 8 XCDs
// round-robin (workgroup b runs on XCD b % 8 as its (b / 8)-th), and xcd_remap hands every XCD one contiguous range of tiles.
// Position-major rows put the 9-tap positions first and the 4-tap corners last, so contiguous ranges give the first XCD only
// 9-tap tiles and the last only 4-tap ones: the launch lasts as long as the unskipped one on the first XCD, whatever the others
// skip (profiles/r07_notes.md).  Here the m-tiles are SORTED by falling tap count (a tile that straddles positions has the OR
// of their taps, so the virtual order alone is not sorted) and dealt in rounds of 8 m-tiles: in a round of equal tap counts
// XCD x takes the x-th m-tile with all its n-tiles back to back (they share the tile's image rows in that XCD's L2); a round
// of mixed counts and the last, partial round are dealt tile by tile.  Every XCD then runs its heaviest tiles first and the
// XCDs' tap totals differ by less than one 9-tap tile (mixed rounds are falling sequences dealt round-robin: the differences
// telescope).  The host describes the sorted order as runs of consecutive m-tiles of one tap count (at most 2 per position);
// the tile contents and their K order do not change, so results stay bit-identical.
constexpr int kOrdRuns = 80;
struct TileOrder {
  int nruns;                 // 0: no order given, the launch keeps xcd_remap's
  int start[kOrdRuns];       // run i: m-tiles start[i] ... of w[i] taps, runs ordered by falling w
  int cum[kOrdRuns + 1];     // m-tiles in the runs before run i
  int w[kOrdRuns];
};

// workgroup b of a grid of tiles_m * tiles_n -> its tile (mt, nt); a permutation of the tiles (tests/test_gpu_conv_tileorder.py)
__host__ __device__ inline void tile_order_map(const TileOrder& o, int b, int tiles_m, int tiles_n, int& mt, int& nt) {
  const int per = 8 * tiles_n;                      // workgroups of a round: 8 m-tiles
  const int g = b / per, j = b - g * per, s0 = 8 * g;
  int r0 = 0;                                       // run of sorted m-tile s0
  while (r0 + 1 < o.nruns && o.cum[r0 + 1] <= s0) ++r0;
  bool uniform = s0 + 8 <= tiles_m;
  if (uniform) {
    int r7 = r0;
    while (r7 + 1 < o.nruns && o.cum[r7 + 1] <= s0 + 7) ++r7;
    uniform = o.w[r7] == o.w[r0];
  }
  const int s = s0 + (uniform ? (j & 7) : j / tiles_n);
  nt = uniform ? (j >> 3) : j % tiles_n;
  int r = r0;
  while (r + 1 < o.nruns && o.cum[r + 1] <= s) ++r;
  mt = o.start[r] + s - o.cum[r];
}

// Position-major weight gradient: the q-th tile a K slice hands out.  A slice's tiles run on one XCD (zmap), three per CU, and a
// tile's K-steps go with the positions at which its tap is inside the map: (H - |dy|) (W - |dx|), 9 / 6 / 4 on a 3x3 map.  In
// the plain order (row block, tap, channel block) the centre tap's tiles start in the middle of every row block and the XCD
// waits for the last of them; here the taps go out heaviest first (centre, the two edge pairs, corners), each for all row
// blocks.  Same tiles, same K order inside each: bit-identical.  Applied where a slice's tiles share an XCD (zmap: a multiple of 8
// slices) and the column tiles are whole taps (conv_C % 64 == 0, which the launch requires, so tiles_n = 9 channel blocks; any
// other tiles_n keeps the plain order, and a tiles_n % 9 == 0 that is not whole taps would still be a permutation of the tiles).
// (Stride 2, bit 3: the launch passes the INPUT map, and the rank by (H - |dy|)(W - |dx|) is then not the tap's cost on the output
// map - on 6 -> 3 the taps with dy = +1 or dx = +1 lose no position.  Still a permutation of the same tiles, so results do not
// change, but "heaviest first" does not hold there; the stride-2 weight gradient ships switched off, ops.CONV_TAPSKIP_STRIDE2_DW.)
__host__ __device__ inline int dw_tile_order(int q, int tiles_m, int tiles_n, int H, int W) {
  if (tiles_n % 9 != 0) return q;
  const int tpt = tiles_n / 9, per = tiles_m * tpt;
  const int rank = q / per, rem = q - rank * per;
  // taps by falling weight, one per nibble: 4, then (1, 7) = (H - 1) W and (3, 5) = H (W - 1), the larger first, then the corners
  const unsigned long long taps = (H - 1) * W >= H * (W - 1) ? 0x862053714ull : 0x862071534ull;
  const int tap = (int)((taps >> (4 * rank)) & 15);
  return (rem / tpt) * tiles_n + tap * tpt + rem % tpt;
}

// Two slice lengths (plan_conv): the j-th workgroup of an XCD that holds ns slices of tiles_m * tiles_n tiles each.  A tile
// costs (positions at which its tap is inside the map) x (slice length), and the XCD's longer slices are its first ones (slice
// z runs on XCD z % 8, the first n_big slices are the long ones), so handing out tap rank by tap rank, each rank for the
// slices in turn, is the order of falling cost: long centre, short centre, long edges, short edges, ...  (6x6 map, 13 and 12
// units on 96 block slots: 64.3 units of makespan against 67.5 slice by slice and a mean of 62.7; arithmetic.)  zs = the XCD's
// zs-th slice, q = the tile's place in dw_tile_order's order inside it; a bijection of [0, ns * tiles).  Any tiles_n that
// dw_tile_order leaves alone keeps the slices one after the other.
__host__ __device__ inline void dw_xcd_order(int j, int tiles_m, int tiles_n, int ns, int& zs, int& q) {
  const int tiles = tiles_m * tiles_n;
  zs = j / tiles;
  q = j - zs * tiles;
  if (tiles_n % 9 != 0) return;
  const int per = tiles_m * (tiles_n / 9);            // a slice's tiles of one tap
  const int rank = j / (ns * per), rem = j - rank * (ns * per);
  zs = rem / per;
  q = rank * per + rem - zs * per;
}

// ---------------------------------------------------------------------------------------------- 3x3 / 1x1 convolution sources
// Geometry of a conv_mode 1 / 2 descriptor: 9 taps (3x3, pad 1) or 1 (1x1, pad 0) at stride cs over a conv_H x conv_W map.
// conv_taps 90: the 3x3 window without padding (espnet Conv2dSubsampling's second convolution): output pixel (ho, wo) is
// centred on input pixel (cs*ho + 1, cs*wo + 1) and every tap is inside the image.
struct ConvGeom {
  int cs, p0, Ho, Wo;       // stride, 1 for the unpadded window, output map
  bool c9;
  __device__ __forceinline__ explicit ConvGeom(const tavsr_gemm_desc& d) {
    cs = d.conv_stride > 1 ? d.conv_stride : 1;
    c9 = d.conv_taps != 1;
    p0 = d.conv_taps == 90 ? 1 : 0;
    Ho = (d.conv_H - 1 - 2 * p0) / cs + 1;
    Wo = (d.conv_W - 1 - 2 * p0) / cs + 1;
  }
};

// The rows of a channels-last image X [n*H*W][C] as the A operand, shared by both CONV 1 sources:
// A(m, k = tap*C + c) = X[m + (tap/3-1)*W + (tap%3-1)][c] inside the image, 0 outside.  Per K-step the tap is uniform, so the row
// offsets of the plain loader move by one scalar and out-of-image rows are pointed at a zero page.
template <int BM, int NT>
struct ImageRows {
  using L = GLoader<BM, false, NT>;
  int64_t off[L::NR];       // this thread's chunks at the window's centre, channel block 0
  uint32_t mask[L::NR];     // bit tap = the tap's neighbour of this thread's row is inside the image
  // the K-step at k = kk, which lies in tap `tap`
  __device__ __forceinline__ void issue(const TileCtx& c, bool c9, int kk, int tap, float* img) const {
    const tavsr_gemm_desc& d = c.d;
    const int toff = c9 ? (tap / 3 - 1) * d.conv_W + (tap % 3 - 1) : 0;
    const int64_t delta = (int64_t)toff * d.conv_C + (kk - tap * d.conv_C);
#pragma unroll
    for (int i = 0; i < L::NR; ++i)
      dma16(((mask[i] >> tap) & 1u) ? c.A + off[i] + delta : d.conv_zero, img + (i * NT + c.wave * 64) * 4);
  }
};

// CONV 1 (forward and data gradient; 3x3 or 1x1, any stride): the image rows in their own order, K-steps in k order.
template <int BM, int NT>
struct ConvRowsA {
  using R = ImageRows<BM, NT>;
  static constexpr int kDma = R::L::NR;
  const TileCtx& c;
  bool c9;
  R rows;
  __device__ __forceinline__ explicit ConvRowsA(const TileCtx& c_) : c(c_) {
    const tavsr_gemm_desc& d = c.d;
    const ConvGeom g(d);
    c9 = g.c9;
    R::L::offsets(d.lda, c.m0, d.M, c.tid, rows.off);
#pragma unroll
    for (int i = 0; i < R::L::NR; ++i) {
      const int m = min(c.m0 + ((i * NT + c.tid) >> 3), d.M - 1);
      // row m = output pixel (n, ho, wo), centred on input pixel (cs*ho, cs*wo)
      const int x = (m % g.Wo) * g.cs + g.p0, y = ((m / g.Wo) % g.Ho) * g.cs + g.p0;
      if (g.cs > 1 || g.p0) rows.off[i] += ((int64_t)((m / (g.Wo * g.Ho)) * d.conv_H + y) * d.conv_W + x - m) * d.conv_C;
      uint32_t mk = 0;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        mk |= (uint32_t)((unsigned)(y + tap / 3 - 1) < (unsigned)d.conv_H && (unsigned)(x + tap % 3 - 1) < (unsigned)d.conv_W) << tap;
      rows.mask[i] = g.c9 ? mk : 1u;
    }
  }
  __device__ __forceinline__ void issue(int kt, float* img) {
    const int kk = c.kbeg + kt * kBK;
    rows.issue(c, c9, kk, kk / c.d.conv_C, img);
  }
};
template <int BM, int BN, int NT, bool BKM>
struct SourceFor<1, false, BM, BN, NT, false, BKM> {
  using type = PairSource<ConvRowsA<BM, NT>, PlainOperand<BN, BKM, NT, true>, BM>;
};
template <int BM, int BN, int NT>
struct SourceFor<1, false, BM, BN, NT, false, false, true> {      // B as bf16 planes (kConvX6)
  using type = PairSource<ConvRowsA<BM, NT>, PlaneOperand<BN, NT>, BM>;
};

// CONV 1 + PM (3x3 / pad 1, stride 1 or 2 - conv_pm): position-major virtual rows (struct PosMajor, gemm_glds.h).  The tile's
// tap set `taps` = OR over the positions its rows span (workgroup-uniform); the ring runs over the K-steps of these taps only,
// in their old order: K-steps of all-padding taps are skipped.  One cursor (tap, cb) = tap and 32-channel block of the next step
// to issue serves both operands: B is fetched at the same compacted k (X6: from its bf16 planes, gemm_glds.h "split operands").
template <int BM, int BN, int NT, bool BKM, bool X6 = false>
struct PosMajorRowsSource : SourceDefaults {
  using R = ImageRows<BM, NT>;
  using LB = std::conditional_t<X6, PlaneLoader<BN, NT>, GLoader<BN, BKM, NT>>;
  static constexpr int kDma = R::L::NR + LB::NR;
  static constexpr bool kPosMajorRows = true;
  const TileCtx& c;
  PosMajor pm{};
  uint32_t taps = 0;
  int tap, cb, nk;
  bool c9;
  R rows;
  std::conditional_t<X6, int, int64_t> offB[LB::NR];
  __device__ __forceinline__ explicit PosMajorRowsSource(const TileCtx& c_) : c(c_) {
    const tavsr_gemm_desc& d = c.d;
    const ConvGeom g(d);
    c9 = g.c9;
    if constexpr (X6) LB::offsets(d.K, c.n0, d.N, c.tid, offB);
    else LB::offsets(d.ldb, c.n0, d.N, c.tid, offB);
    pm.H = g.Ho; pm.W = g.Wo;                         // the rows are output pixels (stride 1: the input map)
    pm.st = g.cs; pm.HI = d.conv_H; pm.WI = d.conv_W;
    pm.n = d.M / (g.Ho * g.Wo);
    const int vlo = c.m0 / pm.n, vhi = min(c.m0 + BM - 1, d.M - 1) / pm.n;
    for (int v = vlo; v <= vhi; ++v) {
      int y, x;
      pm.pos(v, y, x);
      taps |= pm.taps(y, x);
      pm.rp = y * g.Wo + x;
    }
    pm.uni = vlo == vhi;
    pm.base = vlo * pm.n;
    nk = 0;
    for (int t = 0; t < 9; ++t) {                     // the K-steps of this slice that lie in a tap of the set
      const int lo = max(c.kbeg, t * d.conv_C), hi = min(c.kend, (t + 1) * d.conv_C);
      if (((taps >> t) & 1u) && hi > lo) nk += (hi - lo) / kBK;
    }
    tap = c.kbeg / d.conv_C;
    cb = (c.kbeg - tap * d.conv_C) / kBK;
    if (!((taps >> tap) & 1u)) {
      const uint32_t up = taps >> (tap + 1) << (tap + 1);
      tap = up ? __builtin_ctz(up) : 9;
      cb = 0;
    }
#pragma unroll
    for (int i = 0; i < R::L::NR; ++i) {
      const int q = i * NT + c.tid, row = q >> 3;
      const int r = min(c.m0 + row, d.M - 1);
      int y, x, img;
      if (pm.uni) {
        y = pm.rp / g.Wo; x = pm.rp - y * g.Wo; img = r - pm.base;
      } else {
        const int v = r / pm.n;
        pm.pos(v, y, x);
        img = r - v * pm.n;
      }
      rows.off[i] = ((int64_t)img * (d.conv_H * d.conv_W) + g.cs * y * d.conv_W + g.cs * x) * d.lda + ((q & 7) ^ ((row >> 1) & 7)) * 4;
      rows.mask[i] = pm.taps(y, x);
    }
  }
  __device__ __forceinline__ int steps() const { return nk; }
  __device__ __forceinline__ const PosMajor* row_map() const { return &pm; }
  __device__ __forceinline__ void issue(int, float* stage) {
    const tavsr_gemm_desc& d = c.d;
    const int ktap = tap, kk = tap * d.conv_C + cb * kBK;      // the tap and the k of this (compacted) step
    const int wrap = (cb + 1) * kBK >= d.conv_C;
    const uint32_t up = taps >> (tap + 1) << (tap + 1);
    cb = wrap ? 0 : cb + 1;
    tap = !wrap ? tap : up ? __builtin_ctz(up) : 9;
    rows.issue(c, c9, kk, ktap, stage);
    if constexpr (X6) LB::issue(x6_planes(d) + kk / 2, offB, stage + BM * kBK, c.wave);
    else LB::issue(c.B + (BKM ? (int64_t)kk * d.ldb : kk), offB, stage + BM * kBK, c.wave);
  }
};
template <int BM, int BN, int NT, bool BKM>
struct SourceFor<1, true, BM, BN, NT, false, BKM> {
  using type = PosMajorRowsSource<BM, BN, NT, BKM>;
};
template <int BM, int BN, int NT>
struct SourceFor<1, true, BM, BN, NT, false, false, true> {
  using type = PosMajorRowsSource<BM, BN, NT, false, true>;
};

// CONV 2 (weight gradient dW = dY^T patches): the k-major B operand is the image, B(k = m, n = tap*C + c); a 64-wide n tile lies
// in one tap, validity is per k row.  The output pixel (image, oy, ox) of every chunk of this thread is CARRIED from K-step to
// K-step (tiles are issued in k order; a step moves on by BK pixels = (sahi * Ho + salo) rows + sb pixels, at most one wrap
// each): the three divisions per chunk that recomputed it were ~170 integer instructions per K-step beside 32 MFMAs per wave.
template <int BN, int NT>
struct PatchB {
  using L = GLoader<BN, true, NT>;
  static constexpr int kDma = L::NR;
  const TileCtx& c;
  const ConvGeom g;
  int ox[L::NR], oy[L::NR], img[L::NR];
  int sb, salo, sahi, tapoff, cb, dy, dx;
  __device__ __forceinline__ explicit PatchB(const TileCtx& c_) : c(c_), g(c_.d) {
    const tavsr_gemm_desc& d = c.d;
    const int sa = kBK / g.Wo;
    sb = kBK - sa * g.Wo;
    sahi = sa / g.Ho;
    salo = sa - sahi * g.Ho;
    const int tap = c.n0 / d.conv_C;
    cb = c.n0 - tap * d.conv_C;
    dy = g.c9 ? tap / 3 - 1 : 0;
    dx = g.c9 ? tap % 3 - 1 : 0;
    tapoff = dy * d.conv_W + dx;
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      const int m = c.kbeg + (i * NT + c.tid) / (BN / 4);
      const int t = m / g.Wo;
      ox[i] = m - t * g.Wo;
      img[i] = t / g.Ho;
      oy[i] = t - img[i] * g.Ho;
    }
  }
  __device__ __forceinline__ void issue(int, float* dst) {
    const tavsr_gemm_desc& d = c.d;
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      const int r = (((i * NT + c.tid) % (BN / 4)) * 4);
      const int x = ox[i] * g.cs + g.p0, y = oy[i] * g.cs + g.p0;
      const bool ok = (unsigned)(y + dy) < (unsigned)d.conv_H && (unsigned)(x + dx) < (unsigned)d.conv_W;
      const int64_t pix = (int64_t)(img[i] * d.conv_H + y) * d.conv_W + x;
      dma16(ok ? c.B + (pix + tapoff) * d.conv_C + cb + r : d.conv_zero, dst + (i * NT + c.wave * 64) * 4);
      // the next K-step's pixel
      int nx = ox[i] + sb;
      const int w1 = nx >= g.Wo ? 1 : 0;
      nx -= w1 ? g.Wo : 0;
      int ny = oy[i] + salo + w1;
      const int w2 = ny >= g.Ho ? 1 : 0;
      ny -= w2 ? g.Ho : 0;
      ox[i] = nx; oy[i] = ny; img[i] += sahi + w2;
    }
  }
};
template <int BM, int BN, int NT>
struct SourceFor<2, false, BM, BN, NT, true, true> {
  using type = PairSource<PlainOperand<BM, true, NT, false>, PatchB<BN, NT>, BM>;
};
template <int BM, int BN, int NT>
struct SourceFor<2, false, BM, BN, NT, true, true, true> {      // split operands (kConvX6Dw): the same two fp32 images, split in registers
  using type = PairSource<PlainOperand<BM, true, NT, false>, PatchB<BN, NT>, BM>;
};

// CONV 2 + PM (conv_pm): K is the pixel axis and a K slice holds whole images (plan_conv), n of them from image i0 on.  The slice
// is walked position-major: step k' covers pixel position k' / n (row-major, y * W + x) of image i0 + k' % n, so 32 consecutive
// k' share their position (or straddle a few) and the steps at whose positions this tile's tap is padding are passed over:
// neither fetched nor multiplied.  Every pixel of the slice is still summed exactly once for every tap.  One cursor
// (v = y * W + x, img): where the next candidate step starts - workgroup-uniform - serves both operands: A's k rows are gathered
// at the walk's pixels.  Stride 2: the positions are those of the Ho x Wo OUTPUT map (K counts output pixels), position (y, x)
// reads input pixel (2 y + dy, 2 x + dx) of the conv_H x conv_W input map.
template <int BM, int BN, int NT>
struct PatchWalkSource : SourceDefaults {
  using LA = GLoader<BM, true, NT>;
  using LB = GLoader<BN, true, NT>;
  static constexpr int kDma = LA::NR + LB::NR;
  const TileCtx& c;
  const ConvGeom g;
  int64_t offA[LA::NR];     // the row part of A's chunks; k is gathered
  int tapoff, cb, dy, dx;   // this tile's tap and channel block
  int n, i0, nk;
  int v = 0, img = 0, x = 0, y = 0;      // the cursor
  // (the centre tap's tile is the one that skips no pixel)
  __device__ __forceinline__ static int rowsum_n0(const tavsr_gemm_desc& d) { return 4 * d.conv_C; }
  __device__ __forceinline__ bool ok(int py, int px) const {
    return (unsigned)(g.cs * py + dy) < (unsigned)c.d.conv_H && (unsigned)(g.cs * px + dx) < (unsigned)c.d.conv_W;
  }
  __device__ __forceinline__ explicit PatchWalkSource(const TileCtx& c_) : c(c_), g(c_.d) {
    const tavsr_gemm_desc& d = c.d;
    const int tap = c.n0 / d.conv_C;
    cb = c.n0 - tap * d.conv_C;
    dy = g.c9 ? tap / 3 - 1 : 0;
    dx = g.c9 ? tap % 3 - 1 : 0;
    tapoff = dy * d.conv_W + dx;
    const int P = g.Ho * g.Wo;
    i0 = c.kbeg / P;
    n = (c.kend - c.kbeg) / P;
    LA::offsets(d.lda, c.m0, d.M, c.tid, offA);
#pragma unroll
    for (int i = 0; i < LA::NR; ++i) offA[i] -= (int64_t)((i * NT + c.tid) / (BM / 4)) * d.lda;
    if (n % kBK == 0) {         // every step lies on one position
      int ny = 0, nx = 0;       // rows / columns of positions at which the tap is inside the image
      for (int py = 0; py < g.Ho; ++py) ny += (unsigned)(g.cs * py + dy) < (unsigned)d.conv_H;
      for (int px = 0; px < g.Wo; ++px) nx += (unsigned)(g.cs * px + dx) < (unsigned)d.conv_W;
      nk = (n / kBK) * ny * nx;
    } else {                    // the steps that touch a position where the tap is inside the image
      nk = 0;
      int prev = 0, py = 0, px = 0;
      for (int pv = 0; pv < P; ++pv) {
        if (ok(py, px)) {
          const int s_lo = max(pv * n / kBK, prev), s_hi = ((pv + 1) * n - 1) / kBK + 1;
          if (s_hi > s_lo) { nk += s_hi - s_lo; prev = s_hi; }
        }
        if (++px == g.Wo) { px = 0; ++py; }
      }
    }
  }
  __device__ __forceinline__ int steps() const { return nk; }
  __device__ __forceinline__ void advance() {
    img += kBK;
    while (img >= n) {
      img -= n;
      ++v;
      if (++x == g.Wo) { x = 0; ++y; }
    }
  }
  // output pixel of the step's k row kl: its position and image
  __device__ __forceinline__ int64_t locate(int kl, int& py, int& px, int& pimg) const {
    int pv = v;
    pimg = img + kl;
    py = y; px = x;
    while (pimg >= n) {
      pimg -= n;
      ++pv;
      if (++px == g.Wo) { px = 0; ++py; }
    }
    pimg += i0;
    return (int64_t)pimg * (g.Ho * g.Wo) + pv;
  }
  __device__ __forceinline__ void issue(int, float* stage) {
    const tavsr_gemm_desc& d = c.d;
    for (;;) {              // pass the steps whose tap is padding at every position they touch
      bool any = false;
      int end = img + kBK, py = y, px = x;
      for (;;) {
        any |= ok(py, px);
        if (end <= n) break;
        end -= n;
        if (++px == g.Wo) { px = 0; ++py; }
      }
      if (any) break;
      advance();
    }
#pragma unroll
    for (int i = 0; i < LA::NR; ++i) {
      int py, px, pimg;
      const int64_t pix = locate((i * NT + c.tid) / (BM / 4), py, px, pimg);
      dma16(c.A + pix * d.lda + offA[i], stage + (i * NT + c.wave * 64) * 4);
    }
#pragma unroll
    for (int i = 0; i < LB::NR; ++i) {
      const int r = (((i * NT + c.tid) % (BN / 4)) * 4);
      int py, px, pimg;
      locate((i * NT + c.tid) / (BN / 4), py, px, pimg);
      const int64_t pix = ((int64_t)pimg * d.conv_H + g.cs * py) * d.conv_W + g.cs * px;      // the position's input pixel (stride 1: the same pixel)
      dma16(ok(py, px) ? c.B + (pix + tapoff) * d.conv_C + cb + r : d.conv_zero, stage + BM * kBK + (i * NT + c.wave * 64) * 4);
    }
    advance();
  }
};
template <int BM, int BN, int NT>
struct SourceFor<2, true, BM, BN, NT, true, true> {
  using type = PatchWalkSource<BM, BN, NT>;
};
template <int BM, int BN, int NT>
struct SourceFor<2, true, BM, BN, NT, true, true, true> {
  using type = PatchWalkSource<BM, BN, NT>;
};

// ---------------------------------------------------------------------------------------------- Conv3d stem sources
// Conv3d stem (1 -> 64 channels, kernel (5,7,7), stride (1,2,2), padding (2,3,3); conv3d_resnet18.py:48-57) over clips
// x [clips][T = conv_C][H][W], single input channel, 245 taps padded to K / N = 256 - every operand element is its own
// 4-byte LDS-DMA gather (a patch row is 35 runs of 7 floats), so no patch matrix is ever written:
//   4: A(m = output pixel (clip, t, ho, wo), k = (kt*7 + kh)*7 + kw) = x[clip][t + kt - 2][2 ho - 3 + kh][2 wo - 3 + kw];
//   5: the k-major B operand (weight gradient): B(k = pixel, n = tap), as 4 with the roles of rows and columns swapped.
struct StemGeom {
  int T, H, W, Ho, Wo;
  __device__ __forceinline__ explicit StemGeom(const tavsr_gemm_desc& d)
      : T(d.conv_C), H(d.conv_H), W(d.conv_W), Ho((d.conv_H - 1) / 2 + 1), Wo((d.conv_W - 1) / 2 + 1) {}
};

// CONV 4: gather i of this thread fills LDS float (i NT + tid) of the k-contiguous image: row 8 i + (tid >> 5), physical
// column p = tid & 31, i.e. (XOR swizzle) k = 32 kt + kk with kk = (((p >> 2) ^ ((4 i + wave) & 7)) << 2) + (p & 3) - two
// values per thread (i even / odd), so a K-step decodes two taps, not eight.  Per gather stay: the pixel's offset in x and
// one validity mask (bit a: frame t + a - 2 exists; bit 8 + b: row 2 ho - 3 + b; bit 16 + c: column 2 wo - 3 + c).
template <int BM, int NT>
struct Stem4A {
  static_assert(NT == 256, "the two-taps-per-thread decoding assumes 8 rows per gather instruction");
  static constexpr int kDma = BM * kBK / NT;      // 4-byte gathers per thread per tile
  const TileCtx& c;
  const StemGeom g;
  int base[kDma], mask[kDma];
  int kk0, kk1;
  __device__ __forceinline__ explicit Stem4A(const TileCtx& c_) : c(c_), g(c_.d) {
    const int p = c.tid & 31;
    kk0 = ((((p >> 2) ^ (c.wave & 7))) << 2) + (p & 3);
    kk1 = ((((p >> 2) ^ ((c.wave + 4) & 7))) << 2) + (p & 3);
#pragma unroll
    for (int i = 0; i < kDma; ++i) {
      const int row = i * 8 + (c.tid >> 5);
      const int m = min(c.m0 + row, c.d.M - 1);
      const int wo = m % g.Wo, ho = (m / g.Wo) % g.Ho, ft = m / (g.Wo * g.Ho);          // ft = clip * T + t
      const int t = ft % g.T, hy = 2 * ho - 3, wx = 2 * wo - 3;
      base[i] = (ft * g.H + hy) * g.W + wx;
      int mk = 0;
#pragma unroll
      for (int q = 0; q < 5; ++q) mk |= (int)((unsigned)(t + q - 2) < (unsigned)g.T) << q;
#pragma unroll
      for (int q = 0; q < 7; ++q)
        mk |= ((int)((unsigned)(hy + q) < (unsigned)g.H) << (8 + q)) | ((int)((unsigned)(wx + q) < (unsigned)g.W) << (16 + q));
      mask[i] = mk;
    }
  }
  __device__ __forceinline__ void issue(int kt, float* img) {
    int tapoff[2], sh[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = c.kbeg + kt * kBK + (q ? kk1 : kk0);
      const int a = k / 49, r = k - 49 * a, b = r / 7, cc = r - 7 * b;
      tapoff[q] = ((a - 2) * g.H + b) * g.W + cc;
      sh[q] = k < 245 ? (a | ((8 + b) << 8) | ((16 + cc) << 16)) : -1;
    }
#pragma unroll
    for (int i = 0; i < kDma; ++i) {
      const int q = i & 1, mk = mask[i];
      const bool ok = sh[q] >= 0 && (((mk >> (sh[q] & 31)) & (mk >> ((sh[q] >> 8) & 31)) & (mk >> ((sh[q] >> 16) & 31))) & 1);
      dma4(ok ? c.A + (base[i] + tapoff[q]) : c.d.conv_zero, img + i * NT + c.wave * 64);
    }
  }
};
template <int BM, int BN, int NT>
struct SourceFor<4, false, BM, BN, NT, false, false> {
  using type = PairSource<Stem4A<BM, NT>, PlainOperand<BN, false, NT, true>, BM>;
};

// CONV 5: gather (i, wave) of a tile is B(k = 32 kt + 4 i + wave, n = n0 + lane): the tap is fixed per lane, the pixel is
// the same for the whole wave and walks on by 4 per gather (tiles are issued in k order): its coordinates and its offset
// in x are carried (wave-uniform), not divided out.  Needs even H and W (host).
template <int BN, int NT>
struct Stem5B {
  static_assert(BN == 64 && NT == 256, "one k row per wave instruction");
  static constexpr int kDma = BN * kBK / NT;
  const TileCtx& c;
  const StemGeom g;
  int wo, ho, t, off, tapoff, c3, a, b;
  bool nok;
  bool th;                  // frame t + a - 2 and row 2 ho - 3 + b exist (changes only when the pixel changes row)
  __device__ __forceinline__ bool frame_row_ok() const {
    return nok && (unsigned)(t + a - 2) < (unsigned)g.T && (unsigned)(2 * ho - 3 + b) < (unsigned)g.H;
  }
  __device__ __forceinline__ explicit Stem5B(const TileCtx& c_) : c(c_), g(c_.d) {
    const int nn = c.n0 + (c.tid & 63);
    a = nn / 49; b = (nn % 49) / 7;
    const int cc = nn % 7;
    c3 = cc - 3;
    nok = nn < 245;
    tapoff = ((a - 2) * g.H + b - 3) * g.W + cc - 3;
    const int m = c.kbeg + c.wave;
    wo = m % g.Wo; ho = (m / g.Wo) % g.Ho;
    const int ft = m / (g.Wo * g.Ho);
    t = ft % g.T;
    off = (ft * g.H + 2 * ho) * g.W + 2 * wo;
    th = frame_row_ok();
  }
  __device__ __forceinline__ void issue(int, float* img) {
#pragma unroll
    for (int i = 0; i < kDma; ++i) {
      const bool ok = th && (unsigned)(2 * wo + c3) < (unsigned)g.W;
      dma4(ok ? c.B + (off + tapoff) : c.d.conv_zero, img + i * NT + c.wave * 64);
      wo += 4;
      off += 8;
      if (wo >= g.Wo) {                            // wave-uniform: next output row (W = 2 Wo, H = 2 Ho: the offset in x
        wo -= g.Wo;                                // moves on by one input row, also across frames and clips)
        off += g.W;
        if (++ho == g.Ho) {
          ho = 0;
          if (++t == g.T) t = 0;
        }
        th = frame_row_ok();
      }
    }
  }
};
template <int BM, int BN, int NT>
struct SourceFor<5, false, BM, BN, NT, true, true> {
  using type = PairSource<PlainOperand<BM, true, NT, false>, Stem5B<BN, NT>, BM>;
};

// The same stem over ZERO-PADDED clips xp [clips][T + 5][H + 6][W + 8] (2 / 3 frames, 3 / 3 rows, 3 / 5 columns of zeros
// around every clip, tavsr_stem_pad) with the taps laid out k = ((kt*7 + kh) * 8 + kw), K / N = 288 (kw = 7 and the last
// 8 columns carry zero weights): every tap is inside the buffer and four consecutive k are four consecutive floats, so the
// operand is fetched with the GEMM's ordinary 16-byte LDS-DMA (two per thread and K-step instead of eight 4-byte gathers; the
// source is only 8-byte aligned, which gfx950's global_load_lds takes) and no validity test is left:
//   6: A(m, k) = xp[clip][t + kt][2 ho + kh][2 wo + kw];   7: B(k = pixel, n = tap) likewise (weight gradient).
struct PaddedStemGeom {     // Hp x Wp padded frame, Tp padded frames per clip (conv_H, conv_W, conv_C)
  int Hp, Wp, Tp, Ho, Wo, T;
  __device__ __forceinline__ explicit PaddedStemGeom(const tavsr_gemm_desc& d)
      : Hp(d.conv_H), Wp(d.conv_W), Tp(d.conv_C), Ho((d.conv_H - 6) / 2), Wo((d.conv_W - 8) / 2), T(d.conv_C - 5) {}
  __device__ __forceinline__ int pixel(int m) const {      // offset in xp of output pixel m's window (tap 0)
    const int wo = m % Wo, ho = (m / Wo) % Ho, ft = m / (Wo * Ho);
    return (((ft / T) * Tp + ft % T) * Hp + 2 * ho) * Wp + 2 * wo;
  }
};

// CONV 6: the pixel is fixed per chunk, the K-step decodes the chunk's tap.
template <int BM, int NT>
struct Stem6A {
  using L = GLoader<BM, false, NT>;
  static constexpr int kDma = L::NR;
  const TileCtx& c;
  const PaddedStemGeom g;
  int base[L::NR], cl[L::NR];
  __device__ __forceinline__ explicit Stem6A(const TileCtx& c_) : c(c_), g(c_.d) {
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      const int q = i * NT + c.tid, row = q >> 3;
      cl[i] = (q & 7) ^ ((row >> 1) & 7);                    // logical 16-byte chunk of the K-step this DMA fetches
      base[i] = g.pixel(min(c.m0 + row, c.d.M - 1));
    }
  }
  __device__ __forceinline__ void issue(int kt, float* img) {
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      const int ch = (c.kbeg >> 2) + kt * 8 + cl[i], r = ch >> 1, a = r / 7, b = r - 7 * a;
      dma16(c.A + (base[i] + (a * g.Hp + b) * g.Wp + 4 * (ch & 1)), img + (i * NT + c.wave * 64) * 4);
    }
  }
};
template <int BM, int BN, int NT>
struct SourceFor<6, false, BM, BN, NT, false, false> {
  using type = PairSource<Stem6A<BM, NT>, PlainOperand<BN, false, NT, true>, BM>;
};

// CONV 7: the chunk's tap is fixed per thread, its pixel walks on by NT / (BN / 4) per gather (tiles are issued in k order)
template <int BN, int NT>
struct Stem7B {
  using L = GLoader<BN, true, NT>;
  static constexpr int kDma = L::NR;
  const TileCtx& c;
  const PaddedStemGeom g;
  int wo[L::NR], ho[L::NR], t[L::NR], off[L::NR];
  int tapoff;
  __device__ __forceinline__ explicit Stem7B(const TileCtx& c_) : c(c_), g(c_.d) {
    constexpr int CPR = BN / 4;                               // chunks per k row
    int ch = (c.n0 >> 2) + (c.tid % CPR);
    if (ch >= 72) ch = 0;                                     // columns >= 288 are never stored: any valid address
    const int r = ch >> 1, a = r / 7, b = r - 7 * a;
    tapoff = (a * g.Hp + b) * g.Wp + 4 * (ch & 1);
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      const int m = c.kbeg + (i * NT + c.tid) / CPR;
      wo[i] = m % g.Wo; ho[i] = (m / g.Wo) % g.Ho; t[i] = (m / (g.Wo * g.Ho)) % g.T;
      off[i] = g.pixel(m);
    }
  }
  __device__ __forceinline__ void issue(int, float* img) {
    constexpr int STEP = 32;                                  // a thread's gather i of the next tile is 32 pixels further on
#pragma unroll
    for (int i = 0; i < L::NR; ++i) {
      dma16(c.B + (off[i] + tapoff), img + (i * NT + c.wave * 64) * 4);
      wo[i] += STEP;
      off[i] += 2 * STEP;
      while (wo[i] >= g.Wo) {                                 // next output row: 2 rows of the padded frame further down
        wo[i] -= g.Wo;
        off[i] += 2 * g.Wp - 2 * g.Wo;
        if (++ho[i] == g.Ho) {                                // next frame, at the end of a clip over its padding frames
          ho[i] = 0;
          off[i] += (g.Hp - 2 * g.Ho) * g.Wp;
          if (++t[i] == g.T) { t[i] = 0; off[i] += (g.Tp - g.T) * g.Hp * g.Wp; }
        }
      }
    }
  }
};
template <int BM, int BN, int NT>
struct SourceFor<7, false, BM, BN, NT, true, true> {
  using type = PairSource<PlainOperand<BM, true, NT, false>, Stem7B<BN, NT>, BM>;
};

// ---------------------------------------------------------------------------------------------- which tile a workgroup computes
// (the position-major forward / data gradient launches carry their tile order behind the common arguments)
struct GemmArgsOrd {
  GemmArgs g;
  TileOrder ord;
};
template <int CONV, bool PM>
struct TileMap<CONV, PM, true> {
  __device__ __forceinline__ static const GemmArgs& map(const GemmArgsOrd& x, int& bid, int& zidx) {
    bid = xcd_remap(blockIdx.x, gridDim.x);
    zidx = blockIdx.z;
    if (x.ord.nruns > 0) {          // tiles sorted by tap count, dealt evenly to the XCDs (struct TileOrder)
      int mt, nt;
      tile_order_map(x.ord, blockIdx.x, x.g.tiles_m, x.g.tiles_n, mt, nt);
      bid = mt * x.g.tiles_n + nt;
    }
    return x.g;
  }
  __device__ __forceinline__ static const GemmArgs& map(const GemmArgs& args, int& bid, int& zidx) {
    bid = xcd_remap(blockIdx.x, gridDim.x);
    zidx = blockIdx.z;
    if (args.zmap) {
      // Workgroups go to the XCDs round-robin in launch order (x fastest, then z).  The tiles of one K slice of a convolution
      // weight gradient read the same dY rows and overlapping image rows (one tile per tap / channel block): give ALL tiles
      // of a slice to one XCD, back to back, so that the slice is fetched from HBM once and served from that XCD's L2 to the
      // others.  Launch l = x + tiles * z runs on XCD l % 8 as that XCD's (l / 8)-th block: slice (l % 8) + 8 * ((l / 8) /
      // tiles), tile (l / 8) % tiles - a bijection when the number of slices is a multiple of 8 (host).
      const int tiles = gridDim.x, l = blockIdx.x + tiles * blockIdx.z, j = l >> 3;
      int zs = j / tiles;
      bid = j % tiles;
      if constexpr (PM && CONV == 2) {
        if (!(args.d.conv_posmajor & 2)) {
          if (args.n_big > 0) dw_xcd_order(j, args.tiles_m, args.tiles_n, args.nsplit >> 3, zs, bid);
          bid = dw_tile_order(bid, args.tiles_m, args.tiles_n, args.d.conv_H, args.d.conv_W);
        }
      }
      zidx = (l & 7) + 8 * zs;
    }
    return args;
  }
};

// ---------------------------------------------------------------------------------------------- host side
// output map of a padded 3x3 convolution descriptor
static int conv_ho(const tavsr_gemm_desc& d) { return (d.conv_H - 1) / std::max(d.conv_stride, 1) + 1; }
static int conv_wo(const tavsr_gemm_desc& d) { return (d.conv_W - 1) / std::max(d.conv_stride, 1) + 1; }

// tavsr_gemm_desc.conv_posmajor applies: 3x3 / pad 1, forward / data gradient (no row sums there) or weight gradient, at stride 1,
// or at stride 2 where bit 3 asks for it and the output map has at most kPmStride2MaxPos positions (trunk layers 3 and 4 open
// with 11 -> 6 and 6 -> 3: 0.79 of the taps inside the image; at 22 -> 11 it is 0.94 and the position bookkeeping costs more
// than the skipped K-steps give, as it did on the 11x11 map at stride 1 - such a descriptor gets the launch without the flag)
constexpr int kPmStride2MaxPos = 36;
static bool conv_pm(const tavsr_gemm_desc& d) {
  const bool stride_ok = d.conv_stride <= 1 || (d.conv_stride == 2 && (d.conv_posmajor & 8) && conv_ho(d) * conv_wo(d) <= kPmStride2MaxPos);
  return (d.conv_posmajor & ~(kConvX6 | kConvX6Dw)) && (d.conv_mode == 1 || d.conv_mode == 2) && stride_ok && (d.conv_taps == 0 || d.conv_taps == 9) &&
         (d.conv_mode == 2 || !d.a_rowsum);
}

// The sorted tile order of a position-major forward / data gradient launch with BM-row tiles (struct TileOrder).  nruns stays 0,
// and the launch keeps its old order, for a K split (the grid's z axis moves the workgroups' XCDs), where conv_posmajor's bit 1
// asks for it (A/B aid: ops.CONV_TILEORDER) and on a map with more runs than the table holds.  The bound is kOrdRuns = 80 runs
// of consecutive m-tiles with one tap count, counted BEFORE sorting.  Tiles that sit on one position each give one run per
// class of positions (an 11x11 map at 3200 frames: 3 runs).  Where tiles straddle positions the count changes from tile to
// tile along the left / right border, whose positions alternate: a tile over both sides has 9 taps, its neighbour on one
// side 6.  An 11x11 map stays within the bound at every image count from 1 to 200; tall maps do not (60x3 from 84 images,
// 22x22 at 119 - 129 images), and then the whole launch keeps the plain order - the same tiles with the same K-steps,
// bit-identical - rather than a truncated table.
static void tile_order_build(const tavsr_gemm_desc& d, int BM, int nsplit, TileOrder& o) {
  o.nruns = 0;
  const int cs = std::max(d.conv_stride, 1);
  const int P = conv_ho(d) * conv_wo(d);            // the rows are output pixels
  if (nsplit != 1 || (d.conv_posmajor & 2) || P <= 0 || d.M < P) return;
  // the order depends on (H, W, stride, M, BM) alone and a step repeats a handful of them: keep the last one built per thread
  struct Key { int H, W, cs, M, BM; };
  static thread_local Key last{0, 0, 0, 0, 0};
  static thread_local TileOrder last_o;
  if (last.H == d.conv_H && last.W == d.conv_W && last.cs == cs && last.M == d.M && last.BM == BM) { o = last_o; return; }
  PosMajor pm{};
  pm.H = conv_ho(d); pm.W = conv_wo(d); pm.n = d.M / P;
  pm.st = cs; pm.HI = d.conv_H; pm.WI = d.conv_W;
  std::vector<uint32_t> tp(P);
  for (int v = 0; v < P; ++v) {
    int y, x;
    pm.pos(v, y, x);
    tp[v] = pm.taps(y, x);
  }
  struct Run { int start, len, w; };
  std::vector<Run> runs;
  const int tiles_m = cdiv(d.M, BM);
  for (int i = 0; i < tiles_m; ++i) {
    const int vlo = (int)((int64_t)i * BM / pm.n);
    const int vhi = std::min((int)(std::min<int64_t>((int64_t)i * BM + BM - 1, d.M - 1) / pm.n), P - 1);    // (M = whole images: already so)
    uint32_t mk = 0;
    for (int v = vlo; v <= vhi; ++v) mk |= tp[v];
    const int w = __builtin_popcount(mk);
    if (!runs.empty() && runs.back().w == w) ++runs.back().len;
    else runs.push_back(Run{i, 1, w});
    if ((int)runs.size() > kOrdRuns) return;
  }
  std::stable_sort(runs.begin(), runs.end(), [](const Run& a, const Run& b) { return a.w > b.w; });
  int cum = 0;
  for (size_t r = 0; r < runs.size(); ++r) {
    o.start[r] = runs[r].start; o.cum[r] = cum; o.w[r] = runs[r].w;
    cum += runs[r].len;
  }
  o.cum[runs.size()] = cum;
  o.nruns = (int)runs.size();
  last = Key{d.conv_H, d.conv_W, cs, d.M, BM};
  last_o = o;
}

// Implicit-convolution launches.  Tiles (in-call A/B of rounds 1-2; the run-time switches are gone, this records the winners):
//   two LDS stages throughout (the Conv3d stem too: three stages and a 128x64 stem tile lost);
//   forward / data gradient: a 64x128 tile reads the image rows once for two column tiles of weights (unsplit NT, Cout % 128 == 0):
//     +0.6 % on the AV step (128x64 and 128x128 tiles: nothing / worse);
//   weight gradient: a 128x64 tile (Cout % 128 == 0) shares one patch tile between 128 output channels: +1.6 %, and
//     another +0.7 % with the K split re-fitted to its three block slots per CU (2304 blocks);
//   64x64 everywhere else.  All tiles of a K slice of a weight gradient go to one XCD (zmap) where the slices are a multiple of 8.
template <int BM, int BN, int MINW, bool AK, bool BKM, int CONV, bool PM, bool X6 = false, int WM = 2, int WN = 2, int S = 2>
static int launch_conv_tile(const tavsr_gemm_desc& d, const Plan& p, hipStream_t s) {
  const int zmap = (CONV == 2 || CONV == 5 || CONV == 7) && p.nsplit >= 8 && p.nsplit % 8 == 0;
  const bool two = PM && CONV == 2;        // two slice lengths: the position-major weight gradient's alone
  GemmArgs a{d, p.kchunk, p.nsplit, cdiv(d.M, BM), cdiv(d.N, BN), (int)vec_epi_ok(d), zmap, two ? p.n_big : 0, two ? p.kunit : 0};
  const dim3 grid(a.tiles_m * a.tiles_n, 1, p.nsplit);
  if constexpr (PM && CONV == 1) {
    GemmArgsOrd ao{a, {}};
    tile_order_build(d, BM, p.nsplit, ao.ord);
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, S, MINW, AK, BKM, 1, CONV, true, X6>), grid, dim3(WM * WN * 64), 0, s, ao);
  } else {
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, S, MINW, AK, BKM, 1, CONV, PM, X6>), grid, dim3(WM * WN * 64), 0, s, a);
  }
  TAVSR_LAUNCH_CHECK();
  return launch_epilogue(a, s);
}

// conv_posmajor: honoured for the 9 padded taps at stride 1, and at stride 2 on small maps where bit 3 asks (conv_pm; ignored
// elsewhere, include/tavsr.h): same tiles; forward / data gradient keep their K split, the weight gradient's slices are
// whole images (plan_conv)
template <int BM, int BN, int MINW, bool AK, bool BKM, int CONV, bool X6 = false, int WM = 2, int WN = 2, int S = 2>
static int launch_conv_pm(const tavsr_gemm_desc& d, const Plan& p, hipStream_t s) {
  return conv_pm(d) ? launch_conv_tile<BM, BN, MINW, AK, BKM, CONV, true, X6, WM, WN, S>(d, p, s)
                    : launch_conv_tile<BM, BN, MINW, AK, BKM, CONV, false, X6, WM, WN, S>(d, p, s);
}

// conv_posmajor's bit 4 applies: forward / data gradient with both operands k-contiguous, the 9 padded taps or a 1x1 of at least
// 256 channels (the 64- and 128-channel downsamples are 2 and 4 K-steps long and lost 10 % to the wider B stage), a dense B whose
// planes are 16-byte chunks the LDS-DMA can address with 32-bit offsets.  A K split keeps its slices (whole K-steps).
// Tiles (launch_conv; profiles/r14_notes.md): the split costs VALU per A sub-tile and K-step, the MFMAs of a wave grow with its
// tile's columns, and a 64-row block re-reads the whole B for 64 rows - so, where there are tiles enough, 128x128 with 64x64 wave
// tiles (Cout % 128 == 0) and 128x64 with four 32x64 wave tiles (Cout = 64): +7 to +18 % on every trunk row over the fp32
// launch's 64x128 / 64x64, which stay for short launches.  A stage holds BM * 128 + BN * 192 bytes, two stages: 128x128 80 KB and
// 128x64 56 KB (two blocks per CU), 64x128 64 KB (two), 64x64 40 KB (four).
static bool conv_x6(const tavsr_gemm_desc& d, const Plan& p) {
  return (d.conv_posmajor & kConvX6) && d.conv_mode == 1 && !d.a_kmajor && !d.b_kmajor && d.ldb == d.K &&
         (d.conv_taps == 0 || d.conv_taps == 9 || (d.conv_taps == 1 && d.K >= 256)) && aligned16(d.B) && (int64_t)d.N * d.K * 6 < (1ll << 31);
}

// conv_posmajor's bit 5 applies: the weight gradient (conv_mode 2, both operands k-major) of the 9 padded taps, at stride 1 or 2, or
// of the 1x1; not the unpadded window (conv_taps 90: Conv2dSubsampling keeps its launch) and no stem mode.  Both operands are
// activations, so both are split in registers from the fp32 images the fp32 launch stages: same sources, same stage size, same
// tiles, same K split, slabs and orders - only the K-step's arithmetic changes (gemm_glds.h, glds_tile).
static bool conv_x6_dw(const tavsr_gemm_desc& d, const Plan&) {
  return (d.conv_posmajor & kConvX6Dw) && d.conv_mode == 2 && d.a_kmajor && d.b_kmajor && (d.conv_taps == 0 || d.conv_taps == 9 || d.conv_taps == 1);
}

// the weight gradient's tile: what launch_conv runs and what tavsr_conv_dw_tile reports
struct DwTile { int bm, bn, waves, x6; };
static DwTile conv_dw_tile(const tavsr_gemm_desc& d, const Plan& p) {
  const int x6 = conv_x6_dw(d, p);
  return d.M % 128 == 0 ? DwTile{128, 64, 4, x6} : DwTile{64, 64, 4, x6};
}

int launch_conv(const tavsr_gemm_desc& d, const Plan& p, hipStream_t s) {
  switch (d.conv_mode) {
    case 1:       // A patches (NT / NN)
      if (d.b_kmajor) return launch_conv_pm<64, 64, 5, false, true, 1>(d, p, s);
      if (conv_x6(d, p)) {
        // a full round of the 128-row tiles' two block slots per CU: below it the 64-row tiles spread over more CUs
        const bool big = p.nsplit == 1 && (int64_t)cdiv(d.M, 128) * cdiv(d.N, d.N % 128 == 0 ? 128 : 64) >= 512;
        if (big && d.N % 128 == 0) return launch_conv_pm<128, 128, 2, false, false, 1, true>(d, p, s);
        if (big) return launch_conv_pm<128, 64, 2, false, false, 1, true, 4, 1>(d, p, s);
        if (p.nsplit == 1 && d.N % 128 == 0) return launch_conv_pm<64, 128, 2, false, false, 1, true>(d, p, s);
        return launch_conv_pm<64, 64, 4, false, false, 1, true>(d, p, s);
      }
      if (p.nsplit == 1 && d.N % 128 == 0) return launch_conv_pm<64, 128, 3, false, false, 1>(d, p, s);
      return launch_conv_pm<64, 64, 5, false, false, 1>(d, p, s);
    case 2: {     // B patches (TN)
      const DwTile t = conv_dw_tile(d, p);
      if (t.x6 && t.bm == 128) return launch_conv_pm<128, 64, 3, true, true, 2, true>(d, p, s);
      if (t.x6) return launch_conv_pm<64, 64, 5, true, true, 2, true>(d, p, s);
      if (t.bm == 128) return launch_conv_pm<128, 64, 3, true, true, 2>(d, p, s);
      return launch_conv_pm<64, 64, 5, true, true, 2>(d, p, s);
    }
    case 4: return launch_conv_tile<64, 64, 5, false, false, 4, false>(d, p, s);      // Conv3d stem: 4-byte gathers
    case 5: return launch_conv_tile<64, 64, 5, true, true, 5, false>(d, p, s);
    case 6: return launch_conv_tile<64, 64, 5, false, false, 6, false>(d, p, s);      // Conv3d stem over padded clips: 16-byte chunks
    default: return launch_conv_tile<64, 64, 5, true, true, 7, false>(d, p, s);
  }
}

// plan of an implicit-convolution launch: the weight gradient (mode 2) has an enormous K = frames*H*W and few tiles, so K
// is split until all five block slots of every CU are filled (the slabs stay tiny)
Plan plan_conv(const tavsr_gemm_desc& d, bool can_split, int force_split) {
  Plan pc = plan(d, can_split, true);
  if ((d.conv_mode == 2 || d.conv_mode == 5 || d.conv_mode == 7) && can_split) {
    const bool wide = d.conv_mode == 2 && d.M % 128 == 0;     // 128x64 tiles (launch_conv): three block slots per CU
    const long tiles = (long)cdiv(d.M, wide ? 128 : 64) * cdiv(d.N, 64);
    constexpr long target64 = 2560L;
    constexpr long target128 = 2304L;
    const long target = wide ? target128 : target64;
    // position-major weight gradient: a slice holds whole images and whole K-steps (it is walked position-major inside, so a
    // tap's tile costs the same in every slice and the XCDs stay balanced): slices of lcm(H * W, 32) pixels
    int unit = 32;
    if (conv_pm(d)) {
      const int P = conv_ho(d) * conv_wo(d);         // K counts output pixels
      int g = P, b = 32;
      while (b) { const int t = g % b; g = b; b = t; }
      unit = P / g * 32;
      if (pc.nsplit > 1) {
        pc.kchunk = cdiv(pc.kchunk, unit) * unit;
        pc.nsplit = cdiv(d.K, pc.kchunk);
      }
    }
    const long want = std::min<long>(std::max<long>(1, target / tiles), d.K / 512);
    if (want > pc.nsplit) {
      pc.kchunk = cdiv(cdiv(d.K, want), unit) * unit;
      pc.nsplit = cdiv(d.K, pc.kchunk);
    }
    if (pc.nsplit >= 16 && pc.nsplit % 8 != 0) {        // a multiple of 8 slices lets launch_conv keep each slice on one XCD
      for (long w8 = pc.nsplit / 8 * 8; w8 >= 8; w8 -= 8) {
        const int kc = cdiv(cdiv(d.K, w8), unit) * unit;
        if (cdiv(d.K, kc) % 8 == 0) { pc.kchunk = kc; pc.nsplit = cdiv(d.K, kc); break; }
        if (w8 < pc.nsplit / 2) break;
      }
    }
    // Two slice lengths (position-major weight gradient; conv_posmajor's bit 2 keeps the equal slices, A/B aid
    // ops.CONV_DW_UNEVEN).  K is a whole number U of units, and where no multiple of 8 divides U well the equal slices above
    // leave block slots empty: layer 3 at 3200 frames is U = 400, 24 slices of 17 units (the last of 9) = 1728 blocks = 2.25
    // rounds of the 768 slots, and the launch lasts 3 rounds of 17-unit tiles.  With w slices, w a multiple of 8, the first
    // U % w of them one unit longer than the rest, the target is met exactly (32 slices, 16 of 13 and 16 of 12 units: 2304
    // blocks) and every XCD gets the same mix of long and short slices to within one (slice z runs on XCD z % 8).  Taken only
    // where the equal plan misses the target by more than a quarter of a round of block slots and this one does not; an
    // equal plan that fills its rounds (layer 4 at 8 slices) is left alone.  force_split (tavsr_gemm_tune; tests) asks for
    // that many slices, rounded down to a multiple of 8, whatever the targets say.
    if (conv_pm(d) && d.conv_mode == 2 && !(d.conv_posmajor & 4) && d.K % unit == 0) {
      const long U = d.K / unit, round4 = (wide ? 768 : 1280) / 4;
      const long w = std::min<long>(force_split > 0 ? force_split : want, U) / 8 * 8;
      const bool missed = target - (long)pc.nsplit * tiles > round4, hits = target - w * tiles <= round4;
      if (w >= 8 && U % w != 0 && (force_split > 0 || (missed && hits))) {
        pc.nsplit = (int)w;
        pc.kchunk = (int)(U / w) * unit;
        pc.n_big = (int)(U % w);
        pc.kunit = unit;
      }
    }
  }
  return pc;
}

}  // namespace tavsr

// The two entry points below exist for tests/test_gpu_conv_tileorder.py and are deliberately NOT declared in include/tavsr.h: the
// binding resolves every prototype of the header when it loads a library, and the A/B runs load the previous commit's library
// (TAVSR_LIB), which does not have them.  The test declares their signatures itself.
// Host-side view of the position-major tile order (struct TileOrder), for tests: the tile (tile_m[b], tile_n[b]) that
// workgroup b of a forward / data gradient launch over `images` H x W maps computes, with bm-row tiles and tiles_n column
// tiles.  Returns the number of workgroups (the arrays are filled up to max_blocks), 0 when the launch keeps its old order.
extern "C" int tavsr_conv_tile_order(int H, int W, int images, int bm, int tiles_n, int32_t* tile_m, int32_t* tile_n, int max_blocks) {
  using namespace tavsr;
  if (H <= 0 || W <= 0 || images <= 0 || bm <= 0 || tiles_n <= 0) return 0;
  tavsr_gemm_desc d{};
  d.conv_H = H; d.conv_W = W; d.M = images * H * W; d.conv_posmajor = 1;
  TileOrder o;
  tile_order_build(d, bm, 1, o);
  if (o.nruns == 0) return 0;
  const int tiles_m = cdiv(d.M, bm), nwg = tiles_m * tiles_n;
  for (int b = 0; b < nwg && b < max_blocks; ++b) tile_order_map(o, b, tiles_m, tiles_n, tile_m[b], tile_n[b]);
  return nwg;
}

// The same for the position-major weight gradient's order inside a K slice (dw_tile_order): tile[q] = row block * tiles_n + column tile.
extern "C" int tavsr_conv_dw_tile_order(int H, int W, int tiles_m, int tiles_n, int32_t* tile, int max_tiles) {
  if (H <= 0 || W <= 0 || tiles_m <= 0 || tiles_n <= 0) return 0;
  for (int q = 0; q < tiles_m * tiles_n && q < max_tiles; ++q) tile[q] = tavsr::dw_tile_order(q, tiles_m, tiles_n, H, W);
  return tiles_m * tiles_n;
}

// The K split the planner gives the weight gradient of a 3x3 / stride 1 / pad 1 convolution over `images` H x W maps (Cin ->
// Cout channels) with conv_posmajor = posmajor, as tavsr_gemm would launch it with a workspace large enough: returns the number
// of slices, out = {kchunk, n_big, kunit} (slices z < n_big hold kchunk + kunit pixels, the others kchunk; the last one
// whatever is left of K).  Like the two above: for tests, not in the header.
extern "C" int tavsr_conv_dw_plan(int H, int W, int cin, int cout, int images, int posmajor, int force_split, int32_t* out) {
  using namespace tavsr;
  if (H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || images <= 0 || !out) return 0;
  tavsr_gemm_desc d{};
  d.conv_mode = 2; d.conv_H = H; d.conv_W = W; d.conv_C = cin; d.conv_stride = 1; d.conv_taps = 9; d.conv_posmajor = posmajor;
  d.M = cout; d.N = 9 * cin; d.K = images * H * W; d.a_kmajor = d.b_kmajor = 1; d.nb1 = d.nb2 = 1;
  const Plan p = plan_conv(d, true, force_split);
  out[0] = p.kchunk; out[1] = p.n_big; out[2] = p.kunit;
  return p.nsplit;
}

// The tile of that launch (conv_dw_tile) for any stride (1, 2) and taps (9, 1, 90): out = {block rows, block columns, waves, 1 where it
// runs on split operands - conv_posmajor's bit 5 set and honoured}.  For tests, like the above.
extern "C" int tavsr_conv_dw_tile(int H, int W, int cin, int cout, int images, int stride, int taps, int posmajor, int32_t* out) {
  using namespace tavsr;
  if (H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || images <= 0 || stride <= 0 || !out) return 0;
  tavsr_gemm_desc d{};
  d.conv_mode = 2; d.conv_H = H; d.conv_W = W; d.conv_C = cin; d.conv_stride = stride; d.conv_taps = taps; d.conv_posmajor = posmajor;
  const int p0 = taps == 90 ? 1 : 0, nt = taps == 1 ? 1 : 9;
  d.M = cout; d.N = nt * cin; d.K = images * ((H - 1 - 2 * p0) / stride + 1) * ((W - 1 - 2 * p0) / stride + 1);
  d.a_kmajor = d.b_kmajor = 1; d.nb1 = d.nb2 = 1;
  const DwTile t = conv_dw_tile(d, plan_conv(d, true, 0));
  out[0] = t.bm; out[1] = t.bn; out[2] = t.waves; out[3] = t.x6;
  return 1;
}

// ... and the order in which an XCD with ns slices of two lengths hands out their tiles (dw_xcd_order, then dw_tile_order):
// slice[j] = the XCD's slice of its j-th workgroup, tile[j] = row block * tiles_n + column tile.
extern "C" int tavsr_conv_dw_xcd_order(int H, int W, int tiles_m, int tiles_n, int ns, int32_t* slice, int32_t* tile, int max_tiles) {
  if (H <= 0 || W <= 0 || tiles_m <= 0 || tiles_n <= 0 || ns <= 0) return 0;
  for (int j = 0; j < ns * tiles_m * tiles_n && j < max_tiles; ++j) {
    int zs, q;
    tavsr::dw_xcd_order(j, tiles_m, tiles_n, ns, zs, q);
    slice[j] = zs;
    tile[j] = tavsr::dw_tile_order(q, tiles_m, tiles_n, H, W);
  }
  return ns * tiles_m * tiles_n;
}

#ifdef TAVSR_GEMM_TRACE
namespace tavsr {
int conv_trace_read(unsigned long long* out, int max_rows) { return trace_read_unit(out, max_rows); }
}  // namespace tavsr
#endif
