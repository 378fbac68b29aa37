"""Padding taps of the stride-1 3x3 / pad 1 implicit convolution (tavsr_gemm_desc.conv_posmajor, ops.CONV_TAPSKIP): the forward
and data-gradient GEMMs walk their rows position-major and skip the K-steps of taps that are padding for a whole tile; the
weight gradient walks the pixels of a K slice position-major and skips the K-steps where its tile's tap is padding.  Every case
runs with the switch on and off: forward and data gradient must be BIT-identical between the two (only exact 0 * w terms are
dropped, the order of the rest is unchanged) and within 2e-5 of torch conv2d in fp64 on the CPU (the bar of
test_gpu_av.py::test_implicit_conv3x3_vs_conv2d); the weight gradient (another summation order) is held to the fp64 bar in both."""
import functools

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5


class _switch:
    """ops.CONV_TAPSKIP for the body; on = every map size (the default only takes maps of <= CONV_TAPSKIP_MAXPOS positions)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from tavsr import ops
        self.old = (ops.CONV_TAPSKIP, ops.CONV_TAPSKIP_MAXPOS)
        ops.CONV_TAPSKIP, ops.CONV_TAPSKIP_MAXPOS = self.on, 1 << 30

    def __exit__(self, *exc):
        from tavsr import ops
        ops.CONV_TAPSKIP, ops.CONV_TAPSKIP_MAXPOS = self.old


@functools.lru_cache(maxsize=None)
def _case(N, H, W, Cin, Cout, stride=1, k=3, pad=1):
    """inputs (fp32) and the fp64 CPU reference of one shape: computed once, shared, never modified"""
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + Cout + stride + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    zr = torch.nn.functional.conv2d(xr, wr, stride=stride, padding=pad)
    dz = torch.randn(zr.shape, generator=g)
    zr.backward(dz.double())
    return x, w, b, dz, zr.detach(), xr.grad, wr.grad


def _rows(t):         # [N, C, H, W] -> channels-last rows [N*H*W, C] on the GPU
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()


def _img(rows, N, H, W):
    return rows.cpu().view(N, H, W, -1).permute(0, 3, 1, 2)


# (n_img, H, W, Cin, Cout)
SHAPES = [(64, 3, 3, 64, 128),        # tile-uniform positions, 64x128 tile, 4 / 6 / 9-tap tiles
          (64, 3, 3, 64, 64),         # the same through the 64x64 tile
          (96, 3, 3, 32, 128),        # n_img % 64 != 0: tiles straddle two positions, M = 864 leaves a ragged last tile
          (5, 6, 6, 64, 64),          # n_img < 64: a tile spans many positions; M % 32 != 0: no weight gradient
          (128, 1, 1, 32, 64),        # one valid tap
          (128, 1, 2, 32, 128),       # two valid taps
          (32, 7, 5, 64, 128),        # odd, non-square map
          (256, 3, 3, 64, 128),       # weight gradient: K split with slices of whole images
          (160, 3, 3, 64, 128),       # weight gradient: the planner's natural K chunk is not a whole number of images
          (40, 6, 6, 64, 64)]         # weight gradient: slices of 24 and 16 images, K-steps that straddle two and three positions


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_tapskip_vs_conv2d_fp64_and_switch_off(N, H, W, Cin, Cout):
    from tavsr import ops
    from tavsr._lib import TavsrError
    from tavsr.functional_av import _w2d, _w2d_grad
    x, w, _, dz, zr, dxr, dwr = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    out = {}
    for on in (True, False):
        with _switch(on):
            z = ops.conv3x3_fwd(xl, w2d, H, W)
            dx = ops.conv3x3_dx(dzl, wflip, H, W)
            ez, ex = rel_err(_img(z, N, H, W), zr), rel_err(_img(dx, N, H, W), dxr)
            print(f"switch {on}: fwd {ez:.2e} dx {ex:.2e}")
            assert ez < TOL and ex < TOL, (on, ez, ex)
            if (N * H * W) % 32 == 0 and Cin % 64 == 0:
                ew = rel_err(_w2d_grad(ops.conv3x3_dw(dzl, xl, H, W), w.shape).cpu(), dwr)
                print(f"switch {on}: dw {ew:.2e}")
                assert ew < TOL, (on, ew)
            else:       # as before the switch existed: whole 32-pixel K-steps and 64-channel N tiles only
                with pytest.raises(TavsrError, match="tavsr_gemm failed"):
                    ops.conv3x3_dw(dzl, xl, H, W)
            out[on] = (z, dx)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(64, 3, 3, 64, 128), (96, 3, 3, 32, 128), (5, 6, 6, 64, 64)])
def test_tapskip_epilogues_residual_bias_relu(N, H, W, Cin, Cout):
    """every row-addressed operand of the permuted epilogue: the data gradient's residual, the forward's bias + ReLU"""
    from tavsr import ops
    from tavsr.functional_av import _w2d
    x, w, b, dz, zr, dxr, _ = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    res = torch.randn(N * H * W, Cin, generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    for on in (True, False):
        with _switch(on):
            dx = ops.conv3x3_dx(dzl, wflip, H, W, res=res)
            y = ops.conv3x3_fwd(xl, w2d, H, W, bias=b.cuda(), act="relu")
        assert rel_err(_img(dx, N, H, W), dxr + _img(res, N, H, W).double()) < TOL
        assert rel_err(_img(y, N, H, W), torch.relu(zr + b.double().view(1, -1, 1, 1))) < TOL
        out[on] = (dx, y)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def test_bias_gradient_still_sums_every_pixel():
    from tavsr import ops
    N, H, W, Cin, Cout = 64, 3, 3, 64, 128
    x, w, _, dz, _, _, dwr = _case(N, H, W, Cin, Cout)
    from tavsr.functional_av import _w2d_grad
    xl, dzl = _rows(x), _rows(dz)
    for on in (True, False):
        with _switch(on):
            dw, gb = ops.conv3x3_dw(dzl, xl, H, W, bias_grad=True)
        assert rel_err(gb.cpu(), dzl.cpu().double().sum(0)) < 1e-5
        assert rel_err(_w2d_grad(dw, w.shape).cpu(), dwr) < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,k,pad0", [(32, 6, 6, 64, 128, 2, 3, False), (32, 6, 6, 64, 128, 2, 1, False),
                                                          (32, 7, 9, 64, 64, 2, 3, True), (32, 5, 5, 64, 64, 1, 3, True)])
def test_other_convolutions_are_not_reached(N, H, W, Cin, Cout, stride, k, pad0):
    """stride 2, the 1x1 tap and the unpadded window: bit-identical with the switch on and off, and still right"""
    from tavsr import ops
    from tavsr.functional_av import _w2d, _w2d_grad
    x, w, _, dz, zr, _, dwr = _case(N, H, W, Cin, Cout, stride, k, 0 if (pad0 or k == 1) else 1)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    Ho, Wo = zr.shape[2:]
    out = {}
    for on in (True, False):
        with _switch(on):
            z = ops.conv3x3_fwd(xl, w2d, H, W, stride, k * k, pad0)
            dw = ops.conv3x3_dw(dzl, xl, H, W, stride, k * k, pad0)
        assert rel_err(_img(z, N, Ho, Wo), zr) < TOL and rel_err(_w2d_grad(dw, w.shape).cpu(), dwr) < TOL
        out[on] = (z, dw)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


@pytest.mark.parametrize("stride,k,pad0", [(2, 3, False), (2, 1, False), (2, 3, True), (1, 3, True)])
def test_flag_is_ignored_by_the_library_where_it_does_not_apply(stride, k, pad0):
    """descriptors with conv_posmajor SET on stride 2, the 1x1 tap and the unpadded window (ops never builds them: raw ops.gemm
    calls): the library ignores the field - forward and weight gradient bit-identical to the field at 0, and right"""
    from tavsr import ops
    from tavsr.functional_av import _w2d, _w2d_grad
    N, H, W, Cin, Cout = 32, 7, 9, 64, 64
    x, w, _, dz, zr, _, dwr = _case(N, H, W, Cin, Cout, stride, k, 0 if (pad0 or k == 1) else 1)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    Ho, Wo = zr.shape[2:]
    Mo, taps = N * Ho * Wo, 90 if pad0 else k * k
    assert Mo % 32 == 0
    out = {}
    for flag in (1, 0):
        z = torch.empty(Mo, Cout, device="cuda")
        dw = torch.empty(Cout, k * k * Cin, device="cuda")
        ops.gemm(Mo, Cout, k * k * Cin, xl, Cin, w2d, k * k * Cin, z, Cout, conv=(1, H, W, Cin, stride, taps, flag))
        ops.gemm(Cout, k * k * Cin, Mo, dzl, Cout, xl, Cin, dw, k * k * Cin, a_kmajor=True, b_kmajor=True,
                 conv=(2, H, W, Cin, stride, taps, flag))
        assert rel_err(_img(z, N, Ho, Wo), zr) < TOL and rel_err(_w2d_grad(dw, w.shape).cpu(), dwr) < TOL
        out[flag] = (z, dw)
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])


def test_visual_frontend_switch_on_vs_off():
    """the lip front-end (2 clips x 8 frames of 88 x 88), forward + backward: the features and every gradient are bit-identical
    except the stride-1 trunk convolution weights, which may differ by a changed summation order only"""
    from oracle.model import fill_parameters_, synth
    from tavsr.frontend.conv3d_resnet18 import Conv3dResNet18
    m = Conv3dResNet18()
    fill_parameters_(m, seed=61)
    m = m.cuda().train()
    x = synth((2, 8, 88, 88), seed=62).cuda()
    r = synth((2, 8, 512), seed=63).cuda()
    stride1 = {f"trunk.layer{l}.{b}.conv{c}.weight" for l in (1, 2, 3, 4) for b in (0, 1) for c in (1, 2)}
    stride1 -= {f"trunk.layer{l}.0.conv1.weight" for l in (2, 3, 4)}
    assert len(stride1) == 13
    got = {}
    for on in (True, False):
        m.zero_grad(set_to_none=True)
        with _switch(on):
            y, _ = m(x, torch.tensor([8, 8]).cuda())
            (y * r).sum().backward()
        got[on] = (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    assert torch.equal(got[True][0], got[False][0])
    for n, g in got[True][1].items():
        if n in stride1:
            assert rel_err(g, got[False][1][n]) < TOL, n
        else:
            assert torch.equal(g, got[False][1][n]), n
