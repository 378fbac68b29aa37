"""The arithmetic of the split-operand weight gradient (csrc/gemm_glds.h "split operands", the CONV 2 form), restated on the CPU in the
regime that launch runs in: BOTH operands are activations split three ways in the kernel, K is the pixel axis and thousands of k go
into one accumulator, the image operand is non-negative (post-ReLU) or sits at an offset while dz is signed.  The model of
tests/test_conv_x6_host.py, extended; and the Python mirror of the launch's gate (ops.x6_dw_takes)."""
import pytest
import torch


def split3(x):
    """x = h + m + l, every part bf16(what the parts before it left), rounded to nearest even"""
    h = x.to(torch.bfloat16).float()
    m = (x - h).to(torch.bfloat16).float()
    l = (x - h - m).to(torch.bfloat16).float()
    return h, m, l


def _six_products(a, b):
    """C = A B^T as the kernel sums it: per 16-k block the products hl, lh, mm, hm, mh, hh, each a 16-term dot product summed exactly and
    rounded once into the ONE fp32 accumulator, small to large"""
    pa, pb = split3(a), split3(b)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 16):
        for ia, ib in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
            acc = (acc.double() + pa[ia][:, k0:k0 + 16].double() @ pb[ib][:, k0:k0 + 16].double().T).float()
    return acc


def _pairwise2_chain(a, b):
    """the fp32 launch's model, v_mfma_f32_32x32x2_f32: two k per instruction, their two products summed exactly and rounded once into the
    fp32 accumulator"""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in range(0, a.shape[1], 2):
        acc = (acc.double() + a[:, k:k + 2].double() @ b[:, k:k + 2].double().T).float()
    return acc


def _operands(kind, k=4096, rows=48, seed=5):
    """(dz rows, image rows) over k pixels"""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(rows, k, generator=g)
    x = torch.randn(rows, k, generator=g)
    if kind == "relu":
        x = torch.relu(x)
    elif kind == "offset":          # post-BatchNorm rows: a mean of either sign well above the spread
        x = x + 150.0 * (1 - 2 * torch.randint(0, 2, (rows, 1), generator=g))
    return dz, x


def _err(c, ref):
    return float((c.double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("kind", ["relu", "offset", "signed"])
def test_six_products_of_two_split_operands_at_k_4096_are_no_worse_than_the_fp32_chain(kind):
    dz, x = _operands(kind)
    ref = dz.double() @ x.double().T
    e6, e32 = _err(_six_products(dz, x), ref), _err(_pairwise2_chain(dz, x), ref)
    print(f"{kind}: six products {e6:.3e}, pairwise-2 fp32 chain {e32:.3e}, ratio {e6 / e32:.2f}")
    # 6 roundings of the accumulator per 16 k against 8: sqrt(6 / 8) = 0.87 of the chain's error in the mean, whatever K is; the
    # dropped products ml, lm, ll are <= 3 x 2^-23 of |a b| each and do not accumulate in the norm
    assert e6 <= e32, (kind, e6, e32)
    assert e6 < 2e-5


def test_the_split_of_both_operands_is_exact_and_zeros_split_to_zeros():
    dz, x = _operands("relu", k=1024)
    for t in (dz, x, x * 2.0 ** 100, dz * 2.0 ** -100):
        # exact where the low part is no bf16 denormal, |t| >= 2^-126 * 2^24 (tests/test_conv_x6_host.py): below that the split loses bits
        # under 2^-133, far beneath anything a product of the scaled pair can show
        t = t[(t == 0) | (t.abs() >= 2.0 ** -102)]
        h, m, l = split3(t)
        assert torch.equal(h.double() + m.double() + l.double(), t.double())
    z = torch.tensor([0.0, -0.0])
    for part in split3(z):
        assert torch.equal(part, torch.zeros(2))
    assert bool((x == 0).any())                       # the post-ReLU operand has exact zeros ...
    h, m, l = split3(x)
    assert bool(((x != 0) | ((h == 0) & (m == 0) & (l == 0))).all())        # ... and they stay zeros in every plane


def test_one_nan_poisons_its_row_of_the_product_only():
    dz, x = _operands("relu", k=64, rows=8)
    dz[3, 17] = float("nan")
    bad = torch.isnan(_six_products(dz, x))
    assert bool(bad[3].all()) and int(bad.sum()) == 8


# (Cin, Cout, taps, output pixels at the benchmark's 3200 frames) of the trunk's weight gradients (profiles/r08_gemm_shapes_av.txt)
TRUNK = [(64, 64, 9, 1548800), (64, 128, 9, 387200), (128, 128, 9, 387200), (128, 256, 9, 115200), (256, 256, 9, 115200),
         (256, 512, 9, 28800), (512, 512, 9, 28800), (64, 128, 1, 387200), (128, 256, 1, 115200), (256, 512, 1, 28800)]


def test_gate_mirror_takes_the_trunk_and_refuses_the_rest(monkeypatch):
    from tavsr import ops
    monkeypatch.setattr(ops, "CONV_X6_DW", True)
    for cin, cout, taps, pixels in TRUNK:
        assert ops.x6_dw_takes(cin, cout, taps, pixels=pixels), (cin, cout, taps)
    assert not ops.x6_dw_takes(256, 256, 9, pad0=True, pixels=1 << 15)          # Conv2dSubsampling's unpadded window
    assert not ops.x6_dw_takes(64, 64, 9, mode=5, pixels=1 << 15)               # the Conv3d stem, gathered ...
    assert not ops.x6_dw_takes(64, 64, 9, mode=7, pixels=1 << 15)               # ... and over padded clips
    assert not ops.x6_dw_takes(64, 64, 9, pixels=8 * 11 * 11)                   # 968 pixels: no whole K-steps (the im2col route)
    assert not ops.x6_dw_takes(32, 64, 9, pixels=1 << 15)                       # a column tile would straddle taps
    monkeypatch.setattr(ops, "CONV_X6_DW", False)
    assert not any(ops.x6_dw_takes(cin, cout, taps, pixels=pixels) for cin, cout, taps, pixels in TRUNK)


def test_the_switch_is_its_own_and_reaches_the_descriptor_bit(monkeypatch):
    """ops.CONV_X6 does not move the weight gradient's bit (tests/test_gpu_conv_x6.py demands identical weight-gradient bits across it)"""
    from tavsr import ops
    seen = []
    monkeypatch.setattr(ops.vision, "gemm", lambda *a, **kw: seen.append(kw["conv"][6]))
    monkeypatch.setattr(ops.vision, "empty", lambda *shape, like=None: None)

    class _T:
        def __init__(self, *shape):
            self.shape = shape

    for x6, dw, want in ((True, True, 32), (False, True, 32), (True, False, 0), (False, False, 0)):
        monkeypatch.setattr(ops, "CONV_X6", x6)
        monkeypatch.setattr(ops, "CONV_X6_DW", dw)
        ops.conv3x3_dw(_T(576, 128), _T(576, 64), 3, 3)
        assert seen[-1] & 32 == want and seen[-1] & 16 == 0
        ops.conv3x3_dw(_T(576, 128), _T(576, 64), 8, 8, stride=2, pad0=True)    # the unpadded window never carries the bit
        assert seen[-1] & 32 == 0
