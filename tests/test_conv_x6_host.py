"""The arithmetic of the split-operand convolution kernels (csrc/gemm_glds.h "split operands"), restated on the CPU: the three-way
bf16 split of an fp32 value and the six-product accumulation the kernel runs per 16-k block.  This is the model the GPU results
of tests/test_gpu_conv_x6.py are read against."""
import pytest
import torch


def _bf16(x, mode):
    if mode == "rne":
        return x.to(torch.bfloat16).float()
    return (x.view(torch.int32) & -65536).view(torch.float32)          # truncation: the upper 16 bits


def split3(x, mode):
    h = _bf16(x, mode)
    m = _bf16(x - h, mode)
    l = _bf16(x - h - m, mode)
    return h, m, l


def _inputs(n, k, seed, offset):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g) + offset, torch.randn(n, k, generator=g) + offset


@pytest.mark.parametrize("mode", ["rne", "trunc"])
def test_three_way_split_is_exact(mode):
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g) + 3.0,
                   torch.randn(1 << 14, generator=g) * 2.0 ** 100, torch.randn(1 << 14, generator=g) * 2.0 ** -100,
                   torch.tensor([0.0, -0.0, 1.0, -1.0, 0.1, 3.0e38 if mode == "trunc" else 3.0e37, 1.2e-30])])
    # exact where the low part is no bf16 denormal: |x| >= 2^-126 * 2^24 (below that the split loses bits under 2^-133, which no product
    # of the trunk sees; the GPU test scales a whole operand by 2^-100 all the same)
    x = x[(x == 0) | (x.abs() >= 2.0 ** -102)]
    h, m, l = split3(x, mode)
    # the residuals are exact in fp32 (Sterbenz-like: each part takes the leading 8 bits of what is left) and the parts are bf16 values
    for part in (h, m, l):
        assert torch.equal(part, _bf16(part, "trunc"))
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert torch.equal((x - h) - m - l, torch.zeros_like(x))
    # sizes: |m| <= 2^-8 |x| and |l| <= 2^-16 |x| to nearest, one bit more when truncating - the dropped ml, lm, ll are <= 2^-23 |a b|
    s = 1 if mode == "trunc" else 0
    assert bool((m.abs() <= x.abs() * 2.0 ** (-8 + s)).all()) and bool((l.abs() <= x.abs() * 2.0 ** (-16 + s)).all())


def test_nan_and_inf_through_the_split():
    x = torch.tensor([float("nan"), float("inf"), -float("inf")])
    h, m, l = split3(x, "rne")
    assert bool(torch.isnan(h[0])) and bool(torch.isnan(m[0]))
    assert bool(torch.isinf(h[1:]).all()) and bool(torch.isnan(m[1:]).all())        # inf - inf: an infinite input gives NaN


def _six_products(a, b, mode):
    """C = A B^T as the kernel sums it: per 16-k block the products hl, lh, mm, hm, mh, hh, each a 16-term dot product summed exactly
    (fp64 holds the 16-bit products and their sum) and rounded once into the fp32 accumulator, small to large"""
    pa, pb = split3(a, mode), split3(b, mode)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 16):
        for ia, ib in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
            blk = pa[ia][:, k0:k0 + 16].double() @ pb[ib][:, k0:k0 + 16].double().T
            acc = (acc.double() + blk).float()
    return acc


def _fmaf_chain(a, b):
    """the fp32 MFMA's model: one fused multiply-add per k into the fp32 accumulator"""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = (acc.double() + a[:, k:k + 1].double() * b[:, k].double()).float()
    return acc


@pytest.mark.parametrize("offset", [0.0, 3.0])
def test_six_products_are_fp32_level_at_k_576(offset):
    a, b = _inputs(32, 576, 11 + int(offset), offset)
    ref = a.double() @ b.double().T
    scale = a.double().abs() @ b.double().abs().T
    e32 = float(((_fmaf_chain(a, b).double() - ref).abs() / scale).max())
    err = {mode: float(((_six_products(a, b, mode).double() - ref).abs() / scale).max()) for mode in ("rne", "trunc")}
    print(f"offset {offset}: fmaf chain {e32:.2e}, six products rne {err['rne']:.2e} trunc {err['trunc']:.2e}")
    # the gate: no worse than 4 x the fp32 chain on the same inputs, and inside the worst case of its own roundings - K / 16 blocks x 6
    # roundings of the accumulator, 2^-24 of at most sum |a| |b| each - plus the dropped products' 3 x 2^-23
    bound = (a.shape[1] // 16) * 6 * 2.0 ** -24 + 3 * 2.0 ** -23
    for mode in ("rne", "trunc"):
        assert err[mode] <= 4 * e32 and err[mode] < bound, (mode, err[mode], e32)


def test_three_products_of_a_two_way_split_are_not():
    """why six: x = h + m with hh, hm, mh leaves mm ~ 2^-16 |a b| behind (to nearest), well above the fp32 chain"""
    a, b = _inputs(32, 576, 14, 3.0)
    ref = a.double() @ b.double().T
    scale = a.double().abs() @ b.double().abs().T
    ha, hb = _bf16(a, "rne"), _bf16(b, "rne")
    ma, mb = _bf16(a - ha, "rne"), _bf16(b - hb, "rne")
    c = ha.double() @ hb.double().T + ha.double() @ mb.double().T + ma.double() @ hb.double().T        # even summed exactly
    e3 = float(((c - ref).abs() / scale).max())
    pa, pb = split3(a, "rne"), split3(b, "rne")
    c6 = sum(pa[i].double() @ pb[j].double().T for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)))
    e6 = float(((c6 - ref).abs() / scale).max())
    print(f"summed exactly: three products {e3:.2e}, six {e6:.2e}")
    assert e3 > 2.0 ** -22 and e6 < 2.0 ** -23, (e3, e6)       # above / inside an fp32 rounding or two of the result
