"""Forward and data gradient of the trunk's convolutions on bf16 MFMA over three-way split fp32 operands (ops.CONV_X6,
tavsr_gemm_desc.conv_posmajor bit 4, csrc/gemm_glds.h "split operands").  Every case runs with the switch on and off against torch
conv2d in fp64 on the CPU: the split-operand result is held to the convolution bar (rel_err < 2e-5) AND to
max(1e-6, 4 x the fp32 launch's rel_err on the same inputs) - six bf16 products are to be as good as the fp32 MFMA, not merely good
enough.  The 1e-6 floor is 8 ulp of fp32: below it the two roundings cannot be told apart by a norm-wise error."""
import functools

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5


class _x6:
    """ops.CONV_X6 for the body"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from tavsr import ops
        self.old = ops.CONV_X6
        ops.CONV_X6 = self.on

    def __exit__(self, *exc):
        from tavsr import ops
        ops.CONV_X6 = self.old


class _tapskip:
    """ops.CONV_TAPSKIP for the body; on = every map size"""

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
def _case(N, H, W, Cin, Cout, stride=1, k=3):
    """inputs (fp32) and the fp64 CPU reference of one shape: computed once, shared, never modified"""
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + Cout + stride + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double()
    zr = torch.nn.functional.conv2d(xr, wr, stride=stride, padding=k // 2)
    dz = torch.randn(zr.shape, generator=g)
    zr.backward(dz.double())
    return x, w, b, dz, zr.detach(), xr.grad


def _rows(t):         # [N, C, H, W] -> channels-last rows [N*H*W, C] on the GPU
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()


def _img(rows, N, H, W):
    return rows.cpu().view(N, H, W, -1).permute(0, 3, 1, 2)


def _held(e_on, e_off, what):
    print(f"{what}: x6 {e_on:.3e}  fp32 {e_off:.3e}  ratio {e_on / max(e_off, 1e-30):.2f}")
    assert e_on < TOL and e_off < TOL, (what, e_on, e_off)
    assert e_on <= max(1e-6, 4 * e_off), (what, e_on, e_off)


def _fwd_dx(x, w, dz, H, W, stride=1, k=3):
    """{switch: (z, dx or None)} of one convolution; the data gradient where ops has one (3x3, stride 1)"""
    from tavsr import ops
    from tavsr.functional_av import _w2d
    N, Cin, Cout = x.shape[0], x.shape[1], w.shape[0]
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    out = {}
    for on in (True, False):
        with _x6(on):
            z = ops.conv3x3_fwd(xl, w2d, H, W, stride, k * k)
            dx = ops.conv3x3_dx(dzl, ops.conv_wflip(w2d, Cout, Cin), H, W) if (stride == 1 and k == 3) else None
        out[on] = (z, dx)
    return out


# (n_img, H, W, Cin, Cout, stride, k)
SHAPES = [(64, 3, 3, 64, 128, 1, 3),       # both tiles, tile-uniform positions
          (64, 3, 3, 64, 64, 1, 3),
          (96, 3, 3, 32, 128, 1, 3),       # one K-step per tap, ragged last tile
          (5, 6, 6, 64, 64, 1, 3),         # a tile spans many positions
          (128, 1, 1, 32, 64, 1, 3),       # one live tap, fewer K-steps than ring stages
          (32, 7, 5, 64, 128, 1, 3),       # odd, non-square map
          (3, 22, 22, 64, 64, 1, 3),       # above CONV_TAPSKIP_MAXPOS: the ConvRowsA source
          (4, 11, 11, 64, 128, 2, 3),      # the stride-2 forward
          (32, 6, 6, 256, 128, 2, 1),      # the 1x1 downsample (taps = 1) from 256 channels on
          (2048, 3, 3, 32, 128, 1, 3),     # enough rows for the launch to go without a K split, as the trunk's do: 64x128, 64x64 tiles
          (2048, 3, 3, 32, 64, 1, 3),
          (7296, 3, 3, 32, 128, 1, 3),     # 513 tiles of 128 rows: the 128x128 and 128x64 tiles
          (7296, 3, 3, 32, 64, 1, 3)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,k", SHAPES)
def test_x6_vs_conv2d_fp64_and_fp32_launch(N, H, W, Cin, Cout, stride, k):
    x, w, _, dz, zr, dxr = _case(N, H, W, Cin, Cout, stride, k)
    Ho, Wo = zr.shape[2:]
    out = _fwd_dx(x, w, dz, H, W, stride, k)
    _held(rel_err(_img(out[True][0], N, Ho, Wo), zr), rel_err(_img(out[False][0], N, Ho, Wo), zr), "fwd")
    if out[True][1] is not None:
        _held(rel_err(_img(out[True][1], N, H, W), dxr), rel_err(_img(out[False][1], N, H, W), dxr), "dx")
    assert not torch.equal(out[True][0], out[False][0])        # the switch reached the launch


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(64, 3, 3, 64, 128), (96, 3, 3, 32, 128), (5, 6, 6, 64, 64)])
def test_x6_epilogues_residual_bias_relu(N, H, W, Cin, Cout):
    from tavsr import ops
    from tavsr.functional_av import _w2d
    x, w, b, dz, zr, dxr = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    res = torch.randn(N * H * W, Cin, generator=torch.Generator().manual_seed(5)).cuda()
    err = {}
    for on in (True, False):
        with _x6(on):
            dx = ops.conv3x3_dx(dzl, wflip, H, W, res=res)
            y = ops.conv3x3_fwd(xl, w2d, H, W, bias=b.cuda(), act="relu")
        err[on] = (rel_err(_img(dx, N, H, W), dxr + _img(res, N, H, W).double()),
                   rel_err(_img(y, N, H, W), torch.relu(zr + b.double().view(1, -1, 1, 1))))
    _held(err[True][0], err[False][0], "dx + res")
    _held(err[True][1], err[False][1], "fwd + bias + relu")


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(64, 3, 3, 64, 128), (96, 3, 3, 32, 128), (5, 6, 6, 64, 64), (32, 7, 5, 64, 128)])
def test_x6_tapskip_on_equals_off(N, H, W, Cin, Cout):
    """the skipped K-steps are exact zeros under the split too: bit-identical"""
    from tavsr import ops
    from tavsr.functional_av import _w2d
    x, w, _, dz, _, _ = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    out = {}
    with _x6(True):
        for on in (True, False):
            with _tapskip(on):
                out[on] = (ops.conv3x3_fwd(xl, w2d, H, W), ops.conv3x3_dx(dzl, wflip, H, W))
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def _ref(x, w):
    return torch.nn.functional.conv2d(x.double(), w.double(), padding=1)


@pytest.mark.parametrize("kind", ["offset", "tiny", "huge", "zero_taps"])
def test_x6_inputs_that_stress_the_split(kind):
    N, H, W, Cin, Cout = 5, 6, 6, 64, 64
    x, w, _, dz, _, _ = _case(N, H, W, Cin, Cout)
    g = torch.Generator().manual_seed(17)
    if kind == "offset":          # every image row (pixel) sits at +-(100 .. 200) spreads from zero
        off = (100.0 + 100.0 * torch.rand(N, 1, H, W, generator=g)) * (1 - 2 * torch.randint(0, 2, (N, 1, H, W), generator=g))
        x = x + off
        w = w + 1.0
    elif kind == "tiny":
        x = x * 2.0 ** -100
    elif kind == "huge":
        x = x * 2.0 ** 100
    else:
        w = w.clone()
        w[:, :, 0, :] = 0.0
        w[:, :, :, 2] = 0.0
    zr = _ref(x, w)
    out = _fwd_dx(x, w, dz, H, W)
    _held(rel_err(_img(out[True][0], N, H, W), zr), rel_err(_img(out[False][0], N, H, W), zr), kind)


def test_x6_one_nan_poisons_its_window_only():
    from tavsr import ops
    from tavsr.functional_av import _w2d
    N, H, W, Cin, Cout = 5, 6, 6, 64, 64
    x, w, _, _, _, _ = _case(N, H, W, Cin, Cout)
    x = x.clone()
    x[1, 3, 2, 4] = float("nan")
    with _x6(True):
        z = _img(ops.conv3x3_fwd(_rows(x), _w2d(w.cuda()), H, W), N, H, W)
    hit = torch.zeros(N, H, W, dtype=torch.bool)
    hit[1, 1:4, 3:6] = True
    bad = torch.isnan(z)
    assert bool((bad == hit.view(N, 1, H, W)).all()) and bool(torch.isfinite(z[~bad]).all())


def test_x6_caller_planes_equal_planes_made_inside():
    from tavsr import ops
    from tavsr.functional_av import _w2d
    N, H, W, Cin, Cout = 64, 3, 3, 64, 128
    x, w, _, dz, _, _ = _case(N, H, W, Cin, Cout)
    xl, dzl, w2d = _rows(x), _rows(dz), _w2d(w.cuda())
    wflip = ops.conv_wflip(w2d, Cout, Cin)
    with _x6(True):
        z, dx = ops.conv3x3_fwd(xl, w2d, H, W), ops.conv3x3_dx(dzl, wflip, H, W)
        zp = ops.conv3x3_fwd(xl, w2d, H, W, planes=ops.conv_wsplit(w2d))
        dxp = ops.conv3x3_dx(dzl, wflip, H, W, planes=ops.conv_wsplit(wflip))
    assert torch.equal(z, zp) and torch.equal(dx, dxp)
    # the buffer: the weights themselves, then three bf16 parts that add up to them (k permuted inside 16-blocks)
    buf = ops.conv_wsplit(w2d)
    n, k = w2d.shape
    assert torch.equal(buf[: n * k].view(n, k), w2d)
    parts = buf[n * k:].view(torch.bfloat16).view(3, n, k // 16, 2, 2, 4).double().sum(0)        # [n][block][lk][half][j]
    assert torch.equal(parts.transpose(2, 3).reshape(n, k), w2d.double())


def test_x6_leaves_the_weight_gradient_alone():
    from tavsr import ops
    N, H, W, Cin, Cout = 64, 3, 3, 64, 128
    x, _, _, dz, _, _ = _case(N, H, W, Cin, Cout)
    xl, dzl = _rows(x), _rows(dz)
    got = {}
    for on in (True, False):
        with _x6(on):
            got[on] = ops.conv3x3_dw(dzl, xl, H, W)
    assert torch.equal(got[True], got[False])


def test_x6_visual_frontend_on_vs_off():
    """the lip front-end (2 clips x 4 frames of 88 x 88), forward + backward: the features and every parameter gradient within the
    convolution bar of the fp32 launches' """
    from oracle.model import fill_parameters_, synth
    from tavsr.frontend.conv3d_resnet18 import Conv3dResNet18
    m = Conv3dResNet18()
    fill_parameters_(m, seed=61)
    m = m.cuda().train()
    x = synth((2, 4, 88, 88), seed=62).cuda()
    r = synth((2, 4, 512), seed=63).cuda()
    got = {}
    for on in (True, False):
        m.zero_grad(set_to_none=True)
        with _x6(on):
            y, _ = m(x, torch.tensor([4, 4]).cuda())
            (y * r).sum().backward()
        got[on] = (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    e = rel_err(got[True][0], got[False][0])
    print(f"features: {e:.3e}")
    worst = max((rel_err(g, got[False][1][n]), n) for n, g in got[True][1].items())
    print(f"worst gradient: {worst[0]:.3e} {worst[1]}")
    assert e < TOL
    for n, g in got[True][1].items():
        assert rel_err(g, got[False][1][n]) < TOL, (n, rel_err(g, got[False][1][n]))
