"""Weight gradient of the trunk's convolutions on bf16 MFMA over three-way split fp32 operands (ops.CONV_X6_DW,
tavsr_gemm_desc.conv_posmajor bit 5, csrc/gemm_glds.h "split operands" / csrc/gemm_conv.hip conv_x6_dw): both operands are activations and
both are split in the kernel.  Every case runs with the switch on and off against torch conv2d's weight gradient in fp64 on the CPU:
the split-operand result is held to the convolution bar (rel_err < 2e-5) AND to max(1e-6, 4 x the fp32 launch's rel_err on the same
inputs), as tests/test_gpu_conv_x6.py holds the forward.  The bias gradient of the same launch stays fp32: bit-identical on and off."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5


class _x6dw:
    """ops.CONV_X6_DW for the body"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from tavsr import ops
        self.old = ops.CONV_X6_DW
        ops.CONV_X6_DW = self.on

    def __exit__(self, *exc):
        from tavsr import ops
        ops.CONV_X6_DW = self.old


@functools.lru_cache(maxsize=None)
def _host():
    """the planner's test entry points (not in include/tavsr.h, as in tests/test_gpu_conv_waves.py)"""
    lib = ctypes.CDLL(f"{ROOT}/tailored-avsr_amd/tavsr/lib/libtavsr_hip.so")
    lib.tavsr_conv_dw_plan.restype, lib.tavsr_conv_dw_plan.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.c_void_p]
    lib.tavsr_conv_dw_tile.restype, lib.tavsr_conv_dw_tile.argtypes = ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.c_void_p]
    return lib


def _plan(H, W, cin, cout, images, flag, force=0):
    """(slices, n_big) of a stride-1 3x3 weight gradient's K split"""
    out = np.zeros(3, np.int32)
    ns = _host().tavsr_conv_dw_plan(H, W, cin, cout, images, flag, force, out.ctypes.data)
    return ns, int(out[1])


def _tile(H, W, cin, cout, images, stride, k, flag):
    """(block rows, block columns, waves, split operands) of the launch conv3x3_dw makes for this descriptor"""
    out = np.zeros(4, np.int32)
    assert _host().tavsr_conv_dw_tile(H, W, cin, cout, images, stride, k * k, flag, out.ctypes.data) == 1
    return tuple(int(v) for v in out)


@functools.lru_cache(maxsize=None)
def _case(N, H, W, Cin, Cout, stride=1, k=3):
    """inputs (fp32) and the fp64 CPU weight gradient of one shape: computed once, shared, never modified"""
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + Cout + stride + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dz = torch.randn(N, Cout, Ho, Wo, generator=g)
    return x, dz, _ref(x, dz, Cout, stride, k)


def _ref(x, dz, Cout, stride=1, k=3):
    wr = torch.zeros(Cout, x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double(), wr, stride=stride, padding=k // 2).backward(dz.double())
    return wr.grad


def _rows(t):         # [N, C, H, W] -> channels-last rows [N*H*W, C] on the GPU
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()


def _flag(H, W, stride=1, k=3, cin=64):
    """conv_posmajor as ops.conv3x3_dw builds it under the current switches"""
    from tavsr import ops
    return ops._tapskip_any(H, W, stride, k * k, False, dw=True) | (32 if ops.x6_dw_takes(cin, 0, k * k) else 0)


def _dw(x, dz, stride=1, k=3, **kw):
    """{switch: the weight gradient in torch's layout [Cout, Cin, k, k] (bias_grad: with the bias gradient)}"""
    from tavsr import ops
    from tavsr.functional_av import _w2d_grad
    H, W = x.shape[2:]
    shape = (dz.shape[1], x.shape[1], k, k)
    xl, dzl = _rows(x), _rows(dz)
    out = {}
    for on in (True, False):
        with _x6dw(on):
            r = ops.conv3x3_dw(dzl, xl, H, W, stride, k * k, **kw)
        out[on] = (_w2d_grad(r[0], shape), r[1]) if kw.get("bias_grad") else _w2d_grad(r, shape)
    return out


def _held(e_on, e_off, what):
    print(f"{what}: x6 {e_on:.3e}  fp32 {e_off:.3e}  ratio {e_on / max(e_off, 1e-30):.2f}")
    assert e_on < TOL and e_off < TOL, (what, e_on, e_off)
    assert e_on <= max(1e-6, 4 * e_off), (what, e_on, e_off)


# (images, H, W, Cin, Cout, stride, k, switches for the body, position-major walk expected)
SHAPES = [(64, 3, 3, 64, 128, 1, 3, {}, True),          # position-major walk, whole steps per position, the 128-row tile
          (64, 3, 3, 64, 64, 1, 3, {}, True),           # the 64-row tile
          (8, 6, 6, 64, 64, 1, 3, {}, True),            # steps straddling positions
          (8, 22, 22, 64, 64, 1, 3, {}, False),         # above CONV_TAPSKIP_MAXPOS_DW: the plain PatchB source (layer 1's form), a K split
          (32, 11, 11, 64, 128, 1, 3, {}, False),       # layer 2's map at the default gate ...
          (32, 11, 11, 64, 128, 1, 3, {"CONV_TAPSKIP_MAXPOS_DW": 121}, True),       # ... and inside it
          (8, 11, 11, 64, 128, 2, 3, {"CONV_TAPSKIP_STRIDE2_DW": False}, False),    # the stride-2 opener, plain and walked
          (8, 11, 11, 64, 128, 2, 3, {"CONV_TAPSKIP_STRIDE2_DW": True}, True),
          (32, 6, 6, 64, 128, 2, 1, {}, False),         # the 1x1 downsample
          (32, 6, 6, 256, 64, 2, 1, {}, False),         # ... from 256 channels, the 64-row tile
          (2048, 3, 3, 64, 128, 1, 3, {}, True)]        # the trunk's regime: a multiple of 8 slices, every slice on one XCD


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,k,switches,walked", SHAPES)
def test_x6_dw_vs_conv2d_fp64_and_fp32_launch(N, H, W, Cin, Cout, stride, k, switches, walked, monkeypatch):
    from tavsr import ops
    for name, v in {"CONV_TAPSKIP": True, "CONV_TILEORDER": True, "CONV_DW_UNEVEN": True, "CONV_TAPSKIP_MAXPOS_DW": 36,
                    "CONV_TAPSKIP_STRIDE2_DW": False, "CONV_X6_DW": True, **switches}.items():
        monkeypatch.setattr(ops, name, v)
    flag = _flag(H, W, stride, k, Cin)
    assert bool(flag & 1) == walked and flag & 32
    # the tile this case is here for, and that the launch runs on split operands
    tile = _tile(H, W, Cin, Cout, N, stride, k, flag)
    assert tile[:2] == ((128, 64) if Cout % 128 == 0 else (64, 64)) and tile[3] == 1, tile
    assert _tile(H, W, Cin, Cout, N, stride, k, flag & ~32)[3] == 0
    if N == 2048:
        ns, _ = _plan(H, W, Cin, Cout, N, flag)
        assert ns >= 8 and ns % 8 == 0
    if H == 22:
        assert _plan(H, W, Cin, Cout, N, flag)[0] > 1
    x, dz, dwr = _case(N, H, W, Cin, Cout, stride, k)
    out = _dw(x, dz, stride, k)
    _held(rel_err(out[True].cpu(), dwr), rel_err(out[False].cpu(), dwr), "dw")
    assert not torch.equal(out[True], out[False])        # the switch reached the launch


@pytest.mark.parametrize("Cout", [128, 64])
def test_x6_dw_two_slice_lengths_and_the_plain_tile_order(Cout, monkeypatch):
    """13 units of 288 pixels in 8 forced slices (5 long); the plain tile order hands out the same tiles with the same K order"""
    from tavsr import ops
    N, H, W, Cin = 104, 6, 6, 64
    for name, v in (("CONV_TAPSKIP", True), ("CONV_TILEORDER", True), ("CONV_DW_UNEVEN", True), ("CONV_TAPSKIP_MAXPOS_DW", 36)):
        monkeypatch.setattr(ops, name, v)
    ns, n_big = _plan(H, W, Cin, Cout, N, 1 | 32, 8)
    assert ns == 8 and n_big == 5
    x, dz, dwr = _case(N, H, W, Cin, Cout)
    out = _dw(x, dz, force=(-1, 8))
    _held(rel_err(out[True].cpu(), dwr), rel_err(out[False].cpu(), dwr), "dw, two slice lengths")
    assert not torch.equal(out[True], out[False])
    monkeypatch.setattr(ops, "CONV_TILEORDER", False)
    assert torch.equal(_dw(x, dz, force=(-1, 8))[True], out[True])


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(64, 3, 3, 64, 128), (8, 6, 6, 64, 64), (8, 22, 22, 64, 64)])
def test_x6_dw_bias_gradient_stays_fp32_bit_for_bit(N, H, W, Cin, Cout):
    x, dz, dwr = _case(N, H, W, Cin, Cout)
    out = _dw(x, dz, bias_grad=True)
    assert torch.equal(out[True][1], out[False][1])
    e = rel_err(out[True][1].cpu(), dz.double().sum((0, 2, 3)))
    print(f"bias gradient: {e:.2e}")
    assert e < 1e-5
    _held(rel_err(out[True][0].cpu(), dwr), rel_err(out[False][0].cpu(), dwr), "dw beside the bias gradient")
    assert torch.equal(out[True][0], _dw(x, dz)[True])             # the same weight gradient with and without the row sums


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(64, 3, 3, 64, 128), (8, 22, 22, 64, 64)])
def test_x6_dw_second_call_gives_the_same_bits(N, H, W, Cin, Cout):
    x, dz, _ = _case(N, H, W, Cin, Cout)
    assert torch.equal(_dw(x, dz)[True], _dw(x, dz)[True])


@pytest.mark.parametrize("kind", ["offset", "scaled", "zero_channels"])
def test_x6_dw_inputs_that_stress_the_split(kind):
    N, H, W, Cin, Cout = 8, 6, 6, 64, 64
    x, dz, _ = _case(N, H, W, Cin, Cout)
    g = torch.Generator().manual_seed(17)
    if kind == "offset":          # every image row (pixel) sits at +-(100 .. 200) spreads from zero: post-BatchNorm activations
        x = x + (100.0 + 100.0 * torch.rand(N, 1, H, W, generator=g)) * (1 - 2 * torch.randint(0, 2, (N, 1, H, W), generator=g))
    elif kind == "scaled":
        x, dz = x * 2.0 ** 100, dz * 2.0 ** -100
    else:                         # three taps' worth of the 9 Cin columns: a third of the input channels are zero
        x = x.clone()
        x[:, ::3] = 0.0
    dwr = _ref(x, dz, Cout)
    out = _dw(x, dz)
    _held(rel_err(out[True].cpu(), dwr), rel_err(out[False].cpu(), dwr), kind)
    if kind == "zero_channels":
        assert bool((out[True][:, ::3] == 0).all())


def test_x6_dw_one_nan_in_dz_poisons_its_output_channel_only():
    N, H, W, Cin, Cout = 8, 6, 6, 64, 64
    x, dz, _ = _case(N, H, W, Cin, Cout)
    dz = dz.clone()
    dz[3, 5, 2, 4] = float("nan")              # an interior pixel: all nine taps multiply it
    bad = torch.isnan(_dw(x, dz)[True].cpu())
    hit = torch.zeros(Cout, Cin, 3, 3, dtype=torch.bool)
    hit[5] = True
    assert int(hit.sum()) == 9 * Cin and bool((bad == hit).all())


@pytest.mark.parametrize("y,xx", [(2, 4), (0, 0), (5, 3)])
def test_x6_dw_one_nan_in_the_image_poisons_the_taps_that_see_it(y, xx):
    N, H, W, Cin, Cout = 8, 6, 6, 64, 64
    x, dz, _ = _case(N, H, W, Cin, Cout)
    x = x.clone()
    x[2, 7, y, xx] = float("nan")
    dw = _dw(x, dz)[True].cpu()
    hit = torch.zeros(Cout, Cin, 3, 3, dtype=torch.bool)
    for ty in range(3):          # tap (ty, tx) reads pixel (y, xx) for output pixel (y - ty + 1, xx - tx + 1), where that is in the map
        for tx in range(3):
            hit[:, 7, ty, tx] = 0 <= y - ty + 1 < H and 0 <= xx - tx + 1 < W
    bad = torch.isnan(dw)
    assert int(hit.sum()) in (9 * Cout, 6 * Cout, 4 * Cout)
    assert bool((bad == hit).all()) and bool(torch.isfinite(dw[~bad]).all())


def test_x6_dw_visual_frontend_on_vs_off():
    """the lip front-end (2 clips x 4 frames of 88 x 88), forward + backward: a weight gradient feeds nothing, so the features are the same
    bits, and every parameter gradient is within the convolution bar of the fp32 launches' """
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
        with _x6dw(on):
            y, _ = m(x, torch.tensor([4, 4]).cuda())
            (y * r).sum().backward()
        got[on] = (y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    assert torch.equal(got[True][0], got[False][0])
    worst = max((rel_err(g, got[False][1][n]), n) for n, g in got[True][1].items())
    print(f"worst gradient: {worst[0]:.3e} {worst[1]}")
    differ = [n for n, g in got[True][1].items() if not torch.equal(g, got[False][1][n])]
    assert differ and all(n.endswith("weight") and ("conv" in n or "downsample.0" in n) for n in differ), differ
    for n, g in got[True][1].items():
        assert rel_err(g, got[False][1][n]) < TOL, (n, rel_err(g, got[False][1][n]))
