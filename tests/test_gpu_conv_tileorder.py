"""Tile order of the position-major 3x3 forward / data-gradient launches (csrc/gemm_conv.hip, struct TileOrder; ops.CONV_TILEORDER):
the tiles are sorted by tap count and dealt to the 8 XCDs in rounds, instead of one contiguous range of tiles per XCD.

* The order is a pure function of the grid: ``tavsr_conv_tile_order`` evaluates the kernel's own ``tile_order_map`` on the host.
  It must be a permutation of the tiles, and the XCDs' tap totals (workgroup b runs on XCD b % 8; a tile's taps are counted
  HERE, from the position order the header documents, not taken from the library) may differ by at most one tile's worth: 9.
  The bound is not fitted: a falling sequence dealt round-robin gives XCD x at least what XCD y > x gets in every row and at
  most what y got one row earlier, so the differences telescope to less than the first (heaviest) tile; rounds of 8 equal
  m-tiles add nothing to any difference.
* On the GPU the tile contents and their K order are unchanged, so every launch must be BIT-identical to conv_posmajor = 0
  (validated against fp64 by test_gpu_conv_tapskip.py), with both orders (flag 1: sorted, flag 3: the contiguous ranges kept
  as the A/B switch), into an output poisoned with NaN: a tile nobody computes leaves NaN behind.
* The position-major weight gradient hands out the tiles of a K slice heaviest tap first (``dw_tile_order``): again a
  permutation of the same tiles, so the result is BIT-identical to the plain order (flag 3) and, like it, within the 2e-5 of
  test_gpu_conv_tapskip.py of conv_posmajor = 0 (another summation order), bias gradient included."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import ROOT, rel_err

# (images, H, W, bm, tiles_n): the GPU cases below, then trunk layers 4 and 3 at the benchmark's batch (3200 frames)
GRIDS = [(70, 3, 3, 64, 1), (70, 3, 3, 64, 2), (9, 3, 3, 64, 1), (40, 6, 6, 64, 1), (40, 6, 6, 64, 2), (576, 3, 3, 64, 1),
         (3200, 3, 3, 64, 4), (3200, 3, 3, 64, 8), (3200, 6, 6, 64, 2), (3200, 6, 6, 64, 4), (3201, 6, 6, 64, 2), (1, 3, 3, 64, 1)]


def _positions(H, W):
    """(y, x) of virtual position v: interior first, then the left / right border of the interior rows, then the top / bottom
    rows without and with their corners (include/tavsr.h: interior, edges, corners)"""
    Hi, Wi = max(H - 2, 0), max(W - 2, 0)
    ys_b = [0] if H == 1 else ([0, H - 1] if H >= 2 else [])
    xs_b = [0] if W == 1 else ([0, W - 1] if W >= 2 else [])
    pos = [(y, x) for y in range(1, 1 + Hi) for x in range(1, 1 + Wi)]
    pos += [(y, x) for y in range(1, 1 + Hi) for x in xs_b]
    pos += [(y, x) for y in ys_b for x in range(1, 1 + Wi)]
    pos += [(y, x) for y in ys_b for x in xs_b]
    assert sorted(pos) == [(y, x) for y in range(H) for x in range(W)]
    return pos


def _tile_taps(n, H, W, bm):
    """tap count of every m-tile: the OR, over the positions its virtual rows v * n + image span, of the taps inside the map"""
    masks = []
    for y, x in _positions(H, W):
        masks.append(sum(1 << t for t in range(9) if 0 <= y + t // 3 - 1 < H and 0 <= x + t % 3 - 1 < W))
    M = n * H * W
    out = []
    for i in range(-(-M // bm)):
        mk = 0
        for v in range(i * bm // n, min(i * bm + bm - 1, M - 1) // n + 1):
            mk |= masks[v]
        out.append(bin(mk).count("1"))
    return out


@pytest.mark.parametrize("n,H,W,bm,tiles_n", GRIDS)
def test_remap_is_a_permutation_and_balances_the_xcds(n, H, W, bm, tiles_n):
    lib = ctypes.CDLL(f"{ROOT}/tailored-avsr_amd/tavsr/lib/libtavsr_hip.so")
    fn = lib.tavsr_conv_tile_order
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    taps = _tile_taps(n, H, W, bm)
    nwg = len(taps) * tiles_n
    tm, tn = np.full(nwg, -1, np.int32), np.full(nwg, -1, np.int32)
    assert fn(H, W, n, bm, tiles_n, tm.ctypes.data, tn.ctypes.data, nwg) == nwg
    assert sorted(zip(tm.tolist(), tn.tolist())) == [(i, j) for i in range(len(taps)) for j in range(tiles_n)]
    w = np.array(taps)[tm]
    per_xcd = [int(w[x::8].sum()) for x in range(8)]
    print(f"tap units per XCD {per_xcd}, contiguous ranges would give "
          f"{[int(s.sum()) for s in np.array_split(np.repeat(taps, tiles_n), 8)]}")
    assert max(per_xcd) - min(per_xcd) <= 9
    for x in range(8):            # heaviest first on every XCD
        assert (np.diff(w[x::8]) <= 0).all()


@pytest.mark.parametrize("H,W,tiles_m,tiles_n", [(3, 3, 4, 72), (6, 6, 2, 36), (3, 3, 1, 9), (7, 5, 1, 9), (5, 7, 2, 18), (3, 3, 2, 10)])
def test_weight_gradient_order_is_a_permutation_heaviest_tap_first(H, W, tiles_m, tiles_n):
    lib = ctypes.CDLL(f"{ROOT}/tailored-avsr_amd/tavsr/lib/libtavsr_hip.so")
    fn = lib.tavsr_conv_dw_tile_order
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int]
    tile = np.full(tiles_m * tiles_n, -1, np.int32)
    assert fn(H, W, tiles_m, tiles_n, tile.ctypes.data, tile.size) == tile.size
    assert sorted(tile.tolist()) == list(range(tile.size))
    if tiles_n % 9:               # no whole taps per column tile: the order is left alone
        assert tile.tolist() == list(range(tile.size))
        return
    tap = (tile % tiles_n) // (tiles_n // 9)
    steps = (H - abs(tap // 3 - 1)) * (W - abs(tap % 3 - 1))      # positions at which the tap is inside the map
    assert (np.diff(steps) <= 0).all() and tap[0] == 4


# (images, H, W, Cin, Cout): a partial last image block with tiles that straddle two positions; fewer tiles than XCDs; the 6x6
# map with tiles over 2 - 3 positions; Cout 256 = two 64x128 column tiles; the 64x64 tile; rounds of 8 equal m-tiles
# ``bk``: the weights as [K, Cout] (b_kmajor): the 64x64 position-major tile, with two and three column tiles at Cout 128 / 192
SHAPES = [(70, 3, 3, 64, 128, False), (9, 3, 3, 64, 128, False), (40, 6, 6, 64, 128, False), (70, 3, 3, 64, 256, False),
          (40, 6, 6, 64, 64, False), (576, 3, 3, 32, 128, False), (70, 3, 3, 64, 128, True), (576, 3, 3, 32, 192, True),
          (40, 6, 6, 64, 192, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cout,bk", SHAPES)
def test_sorted_tile_order_is_bit_identical_to_the_switch_off(N, H, W, Cin, Cout, bk):
    from tavsr import ops
    g = torch.Generator().manual_seed(N + 10 * H + Cin + Cout)
    M, K = N * H * W, 9 * Cin
    x = torch.randn(M, Cin, generator=g).cuda()
    w = (torch.randn(Cout, K, generator=g) / K ** 0.5).cuda()
    if bk:
        w = w.t().contiguous()
    bias = torch.randn(Cout, generator=g).cuda()
    res = torch.randn(M, Cout, generator=g).cuda()
    dzp = torch.randn(M, Cout, generator=g).cuda()
    # plain; bias; residual + ReLU; pre-activation store; data gradient's act'(DZ)
    variants = [dict(), dict(bias=bias), dict(act="relu", R=res, ldr=Cout), dict(bias=bias, act="relu", Z=True),
                dict(DZ=dzp, dact="relu", R=res, ldr=Cout)]
    for kw in variants:
        out = {}
        for flag in (0, 1, 3):
            c = torch.full((M, Cout), float("nan"), device="cuda")
            kw2 = dict(kw)
            if kw.get("Z"):
                kw2["Z"] = torch.full((M, Cout), float("nan"), device="cuda")
            ops.gemm(M, Cout, K, x, Cin, w, Cout if bk else K, c, Cout, b_kmajor=bk, conv=(1, H, W, Cin, 1, 9, flag), **kw2)
            assert not torch.isnan(c).any(), (sorted(kw), flag)
            out[flag] = (c, kw2.get("Z"))
        for flag in (1, 3):
            assert torch.equal(out[flag][0], out[0][0]), (sorted(kw), flag)
            if kw.get("Z"):
                assert not torch.isnan(out[flag][1]).any() and torch.equal(out[flag][1], out[0][1]), (sorted(kw), flag)


# 512 images: 8 K slices of 64 images, each on its own XCD (the reordered launch); 40 images of 6x6: slices of 24 and 16 images
@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(512, 3, 3, 64, 128), (40, 6, 6, 64, 64), (1024, 3, 3, 128, 64)])
def test_weight_gradient_tile_order_is_bit_identical(N, H, W, Cin, Cout):
    from tavsr import ops
    g = torch.Generator().manual_seed(7 * N + H + Cin + Cout)
    M, K = N * H * W, 9 * Cin
    x, dz = torch.randn(M, Cin, generator=g).cuda(), torch.randn(M, Cout, generator=g).cuda()
    out = {}
    for flag in (0, 1, 3):
        dw = torch.full((Cout, K), float("nan"), device="cuda")
        gb = torch.full((Cout,), float("nan"), device="cuda")
        ops.gemm(Cout, K, M, dz, Cout, x, Cin, dw, K, a_kmajor=True, b_kmajor=True, conv=(2, H, W, Cin, 1, 9, flag), a_rowsum=gb)
        assert not torch.isnan(dw).any() and not torch.isnan(gb).any(), flag
        out[flag] = (dw, gb)
    assert torch.equal(out[1][0], out[3][0]) and torch.equal(out[1][1], out[3][1])
    e = rel_err(out[1][0].cpu(), out[0][0].cpu().double())
    print(f"sorted order against conv_posmajor = 0: {e:.2e}")
    assert e < 2e-5 and rel_err(out[1][1].cpu(), dz.cpu().double().sum(0)) < 1e-5


def test_ops_switch_reaches_the_descriptor(monkeypatch):
    from tavsr import ops
    monkeypatch.setattr(ops, "CONV_TILEORDER", True)
    assert ops._tapskip(3, 3) == 1 and ops._tapskip(22, 22) == 0 and ops._tapskip(3, 3, stride=2) == 0
    monkeypatch.setattr(ops, "CONV_TILEORDER", False)
    assert ops._tapskip(3, 3) == 3 and ops._tapskip(22, 22) == 0
