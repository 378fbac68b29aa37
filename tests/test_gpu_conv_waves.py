"""Trunk convolutions, round 8 (csrc/gemm_conv.hip, plan_conv / dw_xcd_order; ops.CONV_DW_UNEVEN, ops.CONV_TAPSKIP_MAXPOS_DW).

* K slices of two lengths for the position-major weight gradient: where equal slices of whole lcm(H*W, 32)-pixel units leave
  block slots empty, the first ``n_big`` of a multiple of 8 slices are one unit longer than the rest (layer 3 at 3200 frames:
  32 slices, 16 of 3744 and 16 of 3456 pixels).  The host cases check the plan (no GPU); the GPU cases hold the weight
  gradient, bias gradient included, to the bar of test_gpu_conv_tapskip.py for a changed summation order: 2e-5 relative
  against torch conv2d in fp64, switch on and switch off alike.
* The 11x11 map of layer 2 under the per-direction gates: forward and data gradient bit-identical to the switch off through
  every epilogue test_gpu_conv_tapskip.py / test_gpu_conv_tileorder.py use, with whole tiles per position (64 images) and with
  straddling tiles (70 images).  The sorted order of an 11x11 map fits the launch arguments' 80 runs at every image count
  from 1 to 200 (checked through tavsr_conv_tile_order), so the fallback to the plain order is exercised where it does occur:
  a tall 60x3 map at 84 images, whose left / right border positions alternate and change the tap count from tile to tile.

* The stride-2 3x3 / pad 1 convolutions that open layers 3 and 4 (bit 3 of conv_posmajor, ops.CONV_TAPSKIP_STRIDE2 / _DW): rows
  position-major over the output map, taps from 2 * o + t - 1 inside the input map.  11 -> 6 (odd input: both borders padded)
  and 6 -> 3 (even input: one border): forward bit-identical to the switch off and within 2e-5 of conv2d in fp64, weight
  gradient within 2e-5 of fp64; on a 22 -> 11 map the library ignores the bit.

Image counts: a weight gradient needs K = images * H * W to be whole 32-pixel K-steps, which on a 6x6 map means images % 8 == 0,
i.e. K is always whole 288-pixel units; "a partial last slice" is therefore a last slice of fewer UNITS (120 images: 15 units,
the equal plan's 8th slice holds one unit where the others hold two), not a ragged unit."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from helpers import ROOT, rel_err

TOL = 2e-5


@functools.lru_cache(maxsize=None)
def _host():
    """the planner's test entry points (not in include/tavsr.h: the A/B runs load older libraries through the header's binding)"""
    lib = ctypes.CDLL(f"{ROOT}/tailored-avsr_amd/tavsr/lib/libtavsr_hip.so")
    lib.tavsr_conv_dw_plan.restype, lib.tavsr_conv_dw_plan.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.c_void_p]
    lib.tavsr_conv_dw_xcd_order.restype = ctypes.c_int
    lib.tavsr_conv_dw_xcd_order.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.tavsr_conv_tile_order.restype = ctypes.c_int
    lib.tavsr_conv_tile_order.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


def _plan(H, W, cin, cout, images, flag=1, force=0):
    """slice lengths of the weight gradient's K split, and n_big"""
    out = np.zeros(3, np.int32)
    ns = _host().tavsr_conv_dw_plan(H, W, cin, cout, images, flag, force, out.ctypes.data)
    kchunk, n_big, kunit = (int(v) for v in out)
    K, lens, k = images * H * W, [], 0
    for z in range(ns):
        n = min(kchunk + (kunit if z < n_big else 0), K - k)
        lens.append(n)
        k += n
    return lens, n_big


# trunk layer 3 at the benchmark's 3200 frames, the forced few-slice plans of the GPU cases below, a 22x22 map with the flag set
TWO_SIZE = [(6, 6, 256, 256, 3200, 0), (6, 6, 64, 64, 104, 8), (6, 6, 64, 128, 120, 8), (6, 6, 64, 128, 200, 16), (22, 22, 64, 64, 3200, 0)]


@pytest.mark.parametrize("H,W,cin,cout,images,force", TWO_SIZE)
def test_two_size_plan_covers_k_in_whole_units_evenly_over_the_xcds(H, W, cin, cout, images, force):
    lens, n_big = _plan(H, W, cin, cout, images, 1, force)
    unit = math.lcm(H * W, 32)
    print(f"{len(lens)} slices, {n_big} long: {sorted(set(lens), reverse=True)} pixels")
    assert n_big > 0 and sum(lens) == images * H * W and min(lens) > 0
    assert all(n % unit == 0 for n in lens)
    assert len(lens) % 8 == 0
    assert sorted(set(lens)) == [lens[-1], lens[-1] + unit] and lens == sorted(lens, reverse=True)
    long_per_xcd = [sum(n == lens[0] for n in lens[x::8]) for x in range(8)]         # slice z runs on XCD z % 8
    assert max(long_per_xcd) - min(long_per_xcd) <= 1
    if n_big % 8 == 0:
        assert len(set(long_per_xcd)) == 1


def test_layer3_at_3200_frames_is_32_slices_16_long_16_short():
    lens, n_big = _plan(6, 6, 256, 256, 3200)
    assert lens == [3744] * 16 + [3456] * 16 and n_big == 16
    assert [sum(n == 3744 for n in lens[x::8]) for x in range(8)] == [2] * 8
    off, nb_off = _plan(6, 6, 256, 256, 3200, flag=5)                   # bit 2: the equal slices of before
    assert off == [4896] * 23 + [2592] and nb_off == 0


@pytest.mark.parametrize("H,W,cin,cout", [(3, 3, 512, 512), (11, 11, 128, 128)])
def test_plans_that_fill_their_rounds_or_cannot_are_left_alone(H, W, cin, cout):
    """layer 4 (8 equal slices = 2304 blocks) and layer 2 (no multiple of 8 slices reaches the target) at 3200 frames"""
    on, nb = _plan(H, W, cin, cout, 3200, flag=1)
    off, _ = _plan(H, W, cin, cout, 3200, flag=5)
    assert on == off and nb == 0
    assert len(on) == (8 if H == 3 else 100)


@pytest.mark.parametrize("H,W,tiles_m,tiles_n,ns", [(6, 6, 2, 36, 4), (6, 6, 1, 9, 2), (3, 3, 4, 72, 3), (7, 5, 1, 18, 2), (3, 3, 2, 10, 2)])
def test_xcd_order_of_two_size_slices_is_a_permutation_by_falling_cost(H, W, tiles_m, tiles_n, ns):
    n = ns * tiles_m * tiles_n
    sl, tile = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    assert _host().tavsr_conv_dw_xcd_order(H, W, tiles_m, tiles_n, ns, sl.ctypes.data, tile.ctypes.data, n) == n
    assert sorted(zip(sl.tolist(), tile.tolist())) == [(s, t) for s in range(ns) for t in range(tiles_m * tiles_n)]
    if tiles_n % 9:               # no whole taps per column tile: slice after slice, plain order
        assert sl.tolist() == sorted(sl.tolist()) and tile.tolist() == list(range(tiles_m * tiles_n)) * ns
        return
    tap = (tile % tiles_n) // (tiles_n // 9)
    steps = (H - abs(tap // 3 - 1)) * (W - abs(tap % 3 - 1))
    assert (np.diff(steps) <= 0).all() and tap[0] == 4
    # a tap's tiles go to the XCD's slices in turn, the first (longer) ones first
    for t in range(9):
        assert (np.diff(sl[tap == t]) >= 0).all()


def test_ops_switches_reach_the_descriptor(monkeypatch):
    from tavsr import ops
    for name, v in (("CONV_TAPSKIP", True), ("CONV_TILEORDER", True), ("CONV_DW_UNEVEN", True), ("CONV_TAPSKIP_MAXPOS", 36),
                    ("CONV_TAPSKIP_MAXPOS_DW", 36)):
        monkeypatch.setattr(ops, name, v)
    assert ops._tapskip(6, 6) == 1 and ops._tapskip(6, 6, dw=True) == 1 and ops._tapskip(11, 11) == 0
    monkeypatch.setattr(ops, "CONV_DW_UNEVEN", False)
    assert ops._tapskip(6, 6, dw=True) == 5
    monkeypatch.setattr(ops, "CONV_TILEORDER", False)
    assert ops._tapskip(6, 6, dw=True) == 7
    monkeypatch.setattr(ops, "CONV_TAPSKIP_MAXPOS", 121)          # the gates are per direction
    assert ops._tapskip(11, 11) == 7 and ops._tapskip(11, 11, dw=True) == 0
    monkeypatch.setattr(ops, "CONV_TAPSKIP_MAXPOS", 36)
    monkeypatch.setattr(ops, "CONV_TAPSKIP_MAXPOS_DW", 121)
    assert ops._tapskip(11, 11) == 0 and ops._tapskip(11, 11, dw=True) == 7 and ops._tapskip(11, 11, stride=2, dw=True) == 0


# ---------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _case(N, H, W, Cin, Cout, stride=1):
    """inputs (fp32) and the fp64 CPU reference of one shape: computed once, shared, never modified"""
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + Cout + stride)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    zr = torch.nn.functional.conv2d(xr, wr, stride=stride, padding=1)
    dz = torch.randn(zr.shape, generator=g)
    zr.backward(dz.double())
    return x, w, b, dz, zr.detach(), xr.grad, wr.grad


def _rows(t):         # [N, C, H, W] -> channels-last rows [N*H*W, C] on the GPU
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()


def _img(rows, N, H, W):
    return rows.cpu().view(N, H, W, -1).permute(0, 3, 1, 2)


# (images, Cout, forced slices): 13 units in 8 slices (5 long); 15 units, where the equal plan's last slice is the short one
# (7 long, 1 short either way); Cout 128: the 128x64 tile; 25 units in 16 slices: two slices per XCD, 9 long (dw_xcd_order)
@pytest.mark.gpu
@pytest.mark.parametrize("N,Cout,force", [(104, 64, 8), (104, 128, 8), (120, 64, 8), (200, 128, 16), (200, 64, 16)])
def test_two_size_weight_gradient_vs_fp64_and_equal_slices(N, Cout, force, monkeypatch):
    from tavsr import ops
    from tavsr.functional_av import _w2d_grad
    H, W, Cin = 6, 6, 64
    lens, n_big = _plan(H, W, Cin, Cout, N, 1, force)
    assert n_big > 0 and len(lens) == force             # the launch below is the two-size one
    x, w, _, dz, _, _, dwr = _case(N, H, W, Cin, Cout)
    xl, dzl = _rows(x), _rows(dz)
    monkeypatch.setattr(ops, "CONV_TAPSKIP", True)
    monkeypatch.setattr(ops, "CONV_TILEORDER", True)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "CONV_DW_UNEVEN", on)
        dw, gb = ops.conv3x3_dw(dzl, xl, H, W, bias_grad=True, force=(-1, force) if on else None)
        ew, eb = rel_err(_w2d_grad(dw, w.shape).cpu(), dwr), rel_err(gb.cpu(), dzl.cpu().double().sum(0))
        print(f"uneven {on}: dw {ew:.2e} bias gradient {eb:.2e}")
        assert ew < TOL and eb < 1e-5, (on, ew, eb)
        got[on] = dw
    assert rel_err(got[True], got[False].double()) < TOL
    monkeypatch.setattr(ops, "CONV_DW_UNEVEN", True)
    monkeypatch.setattr(ops, "CONV_TILEORDER", False)   # the plain tile order: the same slices and K order, so the same bits
    assert torch.equal(ops.conv3x3_dw(dzl, xl, H, W, force=(-1, force)), got[True])


class _layer2:
    """the 11x11 map inside both gates (on) or the skip switched off"""

    def __init__(self, on, monkeypatch):
        from tavsr import ops
        monkeypatch.setattr(ops, "CONV_TAPSKIP", on)
        monkeypatch.setattr(ops, "CONV_TILEORDER", True)
        monkeypatch.setattr(ops, "CONV_DW_UNEVEN", True)
        monkeypatch.setattr(ops, "CONV_TAPSKIP_MAXPOS", 121)
        monkeypatch.setattr(ops, "CONV_TAPSKIP_MAXPOS_DW", 121)
        assert ops._tapskip(11, 11) == (1 if on else 0) and ops._tapskip(11, 11, dw=True) == (1 if on else 0)


def _sorted_order_given(N, H, W, tiles_n):
    tm, tn = np.zeros(1, np.int32), np.zeros(1, np.int32)
    return _host().tavsr_conv_tile_order(H, W, N, 64, tiles_n, tm.ctypes.data, tn.ctypes.data, 1) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 70])
def test_layer2_map_forward_data_gradient_weight_gradient(N, monkeypatch):
    from tavsr import ops
    from tavsr._lib import TavsrError
    from tavsr.functional_av import _w2d, _w2d_grad
    H, W, Cin, Cout = 11, 11, 64, 128
    # 64 images: every 64-row tile on one position, three runs; 70: straddling tiles, still within the table: both run sorted
    assert _sorted_order_given(N, H, W, 1)
    x, w, b, dz, zr, dxr, dwr = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    g = torch.Generator().manual_seed(5)
    res = torch.randn(N * H * W, Cin, generator=g).cuda()
    pre = torch.randn(N * H * W, Cin, generator=g).cuda()
    M, K = N * H * W, 9 * Cout
    out = {}
    for on in (True, False):
        _layer2(on, monkeypatch)
        flag = ops._tapskip(H, W)
        z = ops.conv3x3_fwd(xl, w2d, H, W)
        dx = ops.conv3x3_dx(dzl, wflip, H, W)
        dxres = ops.conv3x3_dx(dzl, wflip, H, W, res=res)
        y = ops.conv3x3_fwd(xl, w2d, H, W, bias=b.cuda(), act="relu")
        dact = []
        for act in ("relu", "swish"):       # the data gradient through act'(pre-activation), with the residual
            c = torch.full((M, Cin), float("nan"), device="cuda")
            ops.gemm(M, Cin, K, dzl, Cout, wflip, K, c, Cin, conv=(1, H, W, Cout, 0, 0, flag), DZ=pre, dact=act, R=res, ldr=Cin)
            assert not torch.isnan(c).any()
            dact.append(c)
        ez, ex = rel_err(_img(z, N, H, W), zr), rel_err(_img(dx, N, H, W), dxr)
        print(f"skip {on}: fwd {ez:.2e} dx {ex:.2e}")
        assert ez < TOL and ex < TOL
        assert rel_err(_img(dxres, N, H, W), dxr + _img(res, N, H, W).double()) < TOL
        assert rel_err(_img(y, N, H, W), torch.relu(zr + b.double().view(1, -1, 1, 1))) < TOL
        out[on] = [z, dx, dxres, y] + dact
        if M % 32 == 0:
            dw, gb = ops.conv3x3_dw(dzl, xl, H, W, bias_grad=True)
            ew = rel_err(_w2d_grad(dw, w.shape).cpu(), dwr)
            print(f"skip {on}: dw {ew:.2e}")
            assert ew < TOL and rel_err(gb.cpu(), dzl.cpu().double().sum(0)) < 1e-5
        else:               # whole 32-pixel K-steps only, with or without the skip
            with pytest.raises(TavsrError, match="tavsr_gemm failed"):
                ops.conv3x3_dw(dzl, xl, H, W)
    for a, c in zip(out[True], out[False]):
        assert torch.equal(a, c)


@pytest.mark.gpu
def test_more_runs_than_the_table_holds_keeps_the_plain_order(monkeypatch):
    """60x3 map, 84 images: 80 runs do not hold the sorted order, the launch keeps the plain one - complete and bit-identical"""
    from tavsr import ops
    from tavsr.functional_av import _w2d
    N, H, W, Cin, Cout = 84, 60, 3, 32, 64
    assert not _sorted_order_given(N, H, W, 1) and _sorted_order_given(64, H, W, 1)
    x, w, b, dz, zr, dxr, _ = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    out = {}
    for on in (True, False):
        for name, v in (("CONV_TAPSKIP", on), ("CONV_TILEORDER", True), ("CONV_DW_UNEVEN", True), ("CONV_TAPSKIP_MAXPOS", H * W)):
            monkeypatch.setattr(ops, name, v)
        assert ops._tapskip(H, W) == (1 if on else 0)
        y = ops.conv3x3_fwd(xl, w2d, H, W, bias=b.cuda(), act="relu")
        dx = ops.conv3x3_dx(dzl, wflip, H, W)
        assert rel_err(_img(y, N, H, W), torch.relu(zr + b.double().view(1, -1, 1, 1))) < TOL
        assert rel_err(_img(dx, N, H, W), dxr) < TOL
        out[on] = (y, dx)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def _stride2(fwd, dw, monkeypatch):
    from tavsr import ops
    for name, v in (("CONV_TAPSKIP", True), ("CONV_TILEORDER", True), ("CONV_DW_UNEVEN", True), ("CONV_TAPSKIP_STRIDE2", fwd),
                    ("CONV_TAPSKIP_STRIDE2_DW", dw)):
        monkeypatch.setattr(ops, name, v)


def test_stride2_switches_reach_the_descriptor(monkeypatch):
    from tavsr import ops
    _stride2(True, True, monkeypatch)
    assert ops._tapskip2(11, 11) == 9 and ops._tapskip2(6, 6, dw=True) == 9 and ops._tapskip2(22, 22) == 0
    assert ops._tapskip_any(11, 11, 2, 9, False) == 9 and ops._tapskip_any(11, 11, 2, 1, False) == 0
    assert ops._tapskip_any(11, 11, 2, 9, True) == 0 and ops._tapskip_any(6, 6, 1, 9, False) == 1
    _stride2(True, False, monkeypatch)
    assert ops._tapskip2(11, 11) == 9 and ops._tapskip2(11, 11, dw=True) == 0
    _stride2(False, True, monkeypatch)
    assert ops._tapskip2(11, 11) == 0 and ops._tapskip2(11, 11, dw=True) == 9
    monkeypatch.setattr(ops, "CONV_TAPSKIP", False)
    assert ops._tapskip2(11, 11, dw=True) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 70])
@pytest.mark.parametrize("H", [11, 6])
def test_stride2_forward_and_weight_gradient(H, N, monkeypatch):
    from tavsr import ops
    from tavsr._lib import TavsrError
    from tavsr.functional_av import _w2d, _w2d_grad
    W, Cin, Cout = H, 64, 128
    x, w, b, dz, zr, _, dwr = _case(N, H, W, Cin, Cout, 2)
    Ho, Wo = zr.shape[2:]
    assert (Ho, Wo) == ((6, 6) if H == 11 else (3, 3))
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    out = {}
    for on in (True, False):
        _stride2(on, on, monkeypatch)
        assert ops._tapskip2(H, W) == (9 if on else 0)
        z = ops.conv3x3_fwd(xl, w2d, H, W, 2)
        y = ops.conv3x3_fwd(xl, w2d, H, W, 2, bias=b.cuda(), act="relu")
        ez = rel_err(_img(z, N, Ho, Wo), zr)
        print(f"stride-2 skip {on}: fwd {ez:.2e}")
        assert ez < TOL and rel_err(_img(y, N, Ho, Wo), torch.relu(zr + b.double().view(1, -1, 1, 1))) < TOL
        out[on] = (z, y)
        if (N * Ho * Wo) % 32 == 0:
            dw, gb = ops.conv3x3_dw(dzl, xl, H, W, 2, bias_grad=True)
            ew = rel_err(_w2d_grad(dw, w.shape).cpu(), dwr)
            print(f"stride-2 skip {on}: dw {ew:.2e}")
            assert ew < TOL and rel_err(gb.cpu(), dzl.cpu().double().sum(0)) < 1e-5
        else:
            with pytest.raises(TavsrError, match="tavsr_gemm failed"):
                ops.conv3x3_dw(dzl, xl, H, W, 2)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


@pytest.mark.gpu
def test_stride2_bit_on_a_22_to_11_map_gives_the_old_launch():
    """raw descriptors (ops never sets the bit there): forward and weight gradient bit-identical to the field at 0, and right"""
    from tavsr import ops
    from tavsr.functional_av import _w2d, _w2d_grad
    N, H, W, Cin, Cout = 32, 22, 22, 64, 64
    x, w, _, dz, zr, _, dwr = _case(N, H, W, Cin, Cout, 2)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    Mo = N * 11 * 11
    assert Mo % 32 == 0
    out = {}
    for flag in (9, 0):
        z = torch.empty(Mo, Cout, device="cuda")
        dw = torch.empty(Cout, 9 * Cin, device="cuda")
        ops.gemm(Mo, Cout, 9 * Cin, xl, Cin, w2d, 9 * Cin, z, Cout, conv=(1, H, W, Cin, 2, 9, flag))
        ops.gemm(Cout, 9 * Cin, Mo, dzl, Cout, xl, Cin, dw, 9 * Cin, a_kmajor=True, b_kmajor=True, conv=(2, H, W, Cin, 2, 9, flag))
        assert rel_err(_img(z, N, 11, 11), zr) < TOL and rel_err(_w2d_grad(dw, w.shape).cpu(), dwr) < TOL
        out[flag] = (z, dw)
    assert torch.equal(out[9][0], out[0][0]) and torch.equal(out[9][1], out[0][1])
