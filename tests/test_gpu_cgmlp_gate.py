"""GPU: the cgMLP gate behind tavsr_dwconv_gate_fwd / _bwd - the gate form of the depthwise-convolution tile core
(csrc/dwconv_time.hip) at every kernel size class, the pair of csrc/cgmlp.hip fixed at K = 31, the partial-slab reduction behind
them, the ``accumulate`` and ``zr`` routes, the refusals, and CgmlpBranch on its unfused route - against tests/cgmlp_gate_ref.py in
float64.

Tolerance (the convention of tests/test_gpu_ebf.py / test_gpu_conformer.py): the same chain is evaluated by the reference in fp32
on the CPU; its error against float64 (e32) is what fp32 costs this computation, and the GPU may be four times as far from float64,
never asked for less than the project's kernel floors: 1e-5 on values (out, conv), 1e-4 on gradients (dr, dgn, dw, dbias).  Values
are compared as max |a - b| / max |b|, gradients as relative L2.  Every case prints both errors and their ratio before it asserts.
Weights are scaled by K ** -0.5, so the convolution's output keeps the scale of its input at every K.

The sweep: K on both sides of 31, K = 1 (no halo; waves 1 to 3 of the backward own no tap), K = 43 / 45 (sizes like any other: the gate uses
no dynamic LDS), K = 63 (all 16 tap accumulators of the gate form, its 32-step tile filling the 96 LDS rows); C = 64 (a whole tile), 67 (a 3-lane tail), 200 (three tiles and 8 lanes); T around
the gate form's tile (32), the K = 31 kernels' backward tile (64) and forward tile (128), each with its halo, around the gate form's
backward chunk (256: at 257 an utterance gets a second partial slab of one step), and T <= pad, where the window is wider than the
utterance.

The measured gpu error / e32 ratios are recorded in profiles/cgmlp_gate_edges.txt.
"""
import pytest
import torch

import cgmlp_gate_ref as R
from helpers import max_rel, rel_err

pytestmark = pytest.mark.gpu

NAN = float("nan")
SWEEP_K = (1, 3, 7, 15, 29, 31, 33, 43, 45, 63)
SWEEP_C = (64, 67, 200)
NAMES = ("out", "conv", "dr", "dgn", "dw", "dbias")
FLOORS = (1e-5, 1e-5, 1e-4, 1e-4, 1e-4, 1e-4)
IS_VALUE = (True, True, False, False, False, False)


def sweep_T(K):
    pad = (K - 1) // 2
    return sorted({t for t in (1, 2, pad, pad + 1, 31, 32, 33, 32 + pad + 1, 63, 64, 65, 64 + pad, 127, 128, 129, 128 + pad + 1, 200,
                               255, 256, 257) if t > 0})


def _bounded(name, gpu, f32, f64, floor, value=False):
    """|gpu - f64| <= max(floor, 4 |f32 - f64|)"""
    err = max_rel if value else rel_err
    gpu, f64 = gpu.detach().cpu(), f64.detach()
    assert bool(torch.isfinite(gpu).all()), name
    if float(f64.abs().max()) < 1e-6:
        assert float(gpu.abs().max()) < 1e-5, name
        return 0.0
    e_gpu, e_f32 = err(gpu, f64), err(f32.detach(), f64)
    print(f"    {name:<44} gpu {e_gpu:.3e}   fp32-on-cpu {e_f32:.3e}   ratio {e_gpu / max(e_f32, 1e-30):.2f}")
    assert e_gpu <= max(floor, 4.0 * e_f32), (name, e_gpu, e_f32)
    return e_gpu / max(e_f32, 1e-30)


def _nan_blocks(*numels):
    """leave NaN in the allocator's cached blocks of these sizes (what TAVSR_POISON=nan does for the whole suite): an output
    element that a kernel does not write then reads NaN"""
    blocks = [torch.full((n,), NAN, device="cuda") for n in numels for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


def _case(B, T, C, K):
    """inputs on the CPU and the float64 / fp32 references (out, conv, dr, dgn, dw, dbias)"""
    g = torch.Generator().manual_seed(100000 * B + 1000 * C + 10 * K + T)
    r, gn, du = (torch.randn(B, T, C, generator=g) for _ in range(3))
    w, b = torch.randn(C, K, generator=g) * K ** -0.5, torch.randn(C, generator=g)
    return (r, gn, du, w, b), R.gate_with_grads(r, gn, w, b, du, torch.float64), R.gate_with_grads(r, gn, w, b, du, torch.float32)


def _wide(t, M, C):
    """a [M, 2C + 8] buffer of NaN with ``t`` (or nothing) in its first C columns, and the view of those columns: how the layer
    holds r (the left half of channel_proj1's output) and dr (the left half of its gradient)"""
    buf = torch.full((M, 2 * C + 8), NAN, device="cuda")
    if t is not None:
        buf[:, :C] = t.reshape(M, C).cuda()
    return buf, buf[:, :C]


def _run_gpu(inputs, B, T):
    """forward, then the backward twice (dw / dbias bit-equal), outputs beyond the C columns untouched -> the six results with
    out / conv / dr / dgn as [B*T, C] rows"""
    from tavsr import ops
    r, gn, du, w, b = inputs
    C, K = w.shape
    M = B * T
    (rbuf, rg), (drbuf, drg) = _wide(r, M, C), _wide(None, M, C)
    gng, dug, wg, bg = gn.reshape(M, C).cuda(), du.reshape(M, C).cuda(), w.cuda(), b.cuda()
    nws = max(1, ops.lib().tavsr_dwconv_gate_bwd_ws(B, T, C, K))
    _nan_blocks(M * C, C * K, C, nws)
    out, conv = ops.dwconv_gate_fwd(gng, rg, wg, bg, B, T)
    dgn, dw, db = ops.dwconv_gate_bwd(dug, gng, rg, conv, wg, drg, B, T)
    dr = drg.clone()
    _nan_blocks(M * C, C * K, C, nws)
    drg.fill_(NAN)
    dgn2, dw2, db2 = ops.dwconv_gate_bwd(dug, gng, rg, conv, wg, drg, B, T)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), (B, T, C, K, "dw / dbias differ between two runs")
    assert torch.equal(dgn, dgn2) and torch.equal(dr, drg), (B, T, C, K, "dr / dgn differ between two runs")
    assert bool(torch.isnan(rbuf[:, C:]).all()) and bool(torch.isnan(drbuf[:, C:]).all()), (B, T, C, K, "wrote beyond the C columns")
    return out, conv, dr, dgn, dw, db


def _check(tag, got, r32, r64, names=NAMES):
    worst = 0.0
    for n, fl, val, g_, a, c in zip(NAMES, FLOORS, IS_VALUE, got, r32, r64):
        if n in names:
            worst = max(worst, _bounded(f"{tag} {n}", g_.reshape(c.shape), a, c, fl, value=val))
    return worst


# ------------------------------------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("K", SWEEP_K)
@pytest.mark.parametrize("C", SWEEP_C)
def test_dwconv_gate_kernels_vs_float64(C, K):
    """forward and backward at every T of sweep_T(K), B = 3; r and dr are column views of wider NaN-filled buffers (row strides
    2C + 8), the allocator's blocks of the output and workspace sizes hold NaN, nothing is written beyond the C columns, the
    backward's results are bit-equal across two runs, and the middle utterance run alone (B = 1) gives bit for bit its rows of
    the B = 3 run: nothing crosses an utterance boundary through the halo"""
    B = 3
    worst = 0.0
    for T in sweep_T(K):
        inputs, r64, r32 = _case(B, T, C, K)
        got = _run_gpu(inputs, B, T)
        print(f"  C {C} K {K} T {T}")
        worst = max(worst, _check(f"T {T}", got, r32, r64))
        r, gn, du, w, b = inputs
        alone = _run_gpu((r[1:2], gn[1:2], du[1:2], w, b), 1, T)
        for n, whole, one in zip(NAMES[:4], got[:4], alone[:4]):
            assert torch.equal(whole[T:2 * T], one), (T, n, "the middle utterance alone differs from its rows in the batch")
    print(f"  C {C} K {K}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("C", SWEEP_C)
def test_every_other_supported_kernel_size(C):
    """include/tavsr.h: every odd K from 1 to 63 - the 22 sizes the sweep leaves out, at T = 70 (two backward tiles, the second
    of 6 steps: shorter than the halo from K = 15 on), same checks"""
    B, T = 3, 70
    worst = 0.0
    for K in (k for k in range(1, 64, 2) if k not in SWEEP_K):
        inputs, r64, r32 = _case(B, T, C, K)
        print(f"  C {C} K {K} T {T}")
        worst = max(worst, _check(f"K {K}", _run_gpu(inputs, B, T), r32, r64))
    print(f"  C {C}, the other K: worst ratio {worst:.2f}")


# ------------------------------------------------------------------------------------------------ 2. accumulate, slabs, zr
def _raw_bwd(entry, du, gn, r, conv, w, dr, dw, db, accumulate, B, T, *tail):
    """tavsr_dwconv_gate_bwd[_act] through the binding itself, dw / dbias the caller's -> dgn"""
    from tavsr._lib import check, lib, ptr, stream
    C, K = w.shape
    dgn = torch.full((B * T, C), NAN, device="cuda")
    ws = torch.full((max(1, lib().tavsr_dwconv_gate_bwd_ws(B, T, C, K)),), NAN, device="cuda")
    check(getattr(lib(), entry)(ptr(du), ptr(gn), ptr(r), r.stride(0), ptr(conv), ptr(w), ptr(dr), dr.stride(0), ptr(dgn), ptr(dw),
                                ptr(db), accumulate, ptr(ws), B, T, C, K, *tail, stream()), entry)
    return dgn


@pytest.mark.parametrize("K", [7, 31])
def test_backward_accumulates_into_dw_and_dbias(K):
    """accumulate = 1 (what the C-side layer passes): dw / dbias += the gradient, bit-equal to prefill + the accumulate = 0
    result (one fp32 addition per element either way); a ragged channel tile, two time tiles"""
    from tavsr import ops
    B, T, C = 3, 65, 67
    M = B * T
    (r, gn, du, w, b), r64, r32 = _case(B, T, C, K)
    (_, rg), (_, drg) = _wide(r, M, C), _wide(None, M, C)
    gng, dug, wg, bg = gn.reshape(M, C).cuda(), du.reshape(M, C).cuda(), w.cuda(), b.cuda()
    _, conv = ops.dwconv_gate_fwd(gng, rg, wg, bg, B, T)
    dw0, db0 = torch.full((C, K), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    _raw_bwd("tavsr_dwconv_gate_bwd", dug, gng, rg, conv, wg, drg, dw0, db0, 0, B, T)
    _bounded("dw", dw0, r32[4], r64[4], 1e-4)
    _bounded("dbias", db0, r32[5], r64[5], 1e-4)
    torch.manual_seed(K)
    pw, pb = torch.randn(C, K, device="cuda"), torch.randn(C, device="cuda")
    dw1, db1 = pw.clone(), pb.clone()
    _raw_bwd("tavsr_dwconv_gate_bwd", dug, gng, rg, conv, wg, drg, dw1, db1, 1, B, T)
    assert torch.equal(dw1, pw + dw0) and torch.equal(db1, pb + db0)


SLAB_T = {1: 2, 17: 2, 65: 2, 9: 257}


@pytest.mark.parametrize("B", SLAB_T)
def test_partial_slab_reduction_block_counts(B):
    """one partial slab per utterance and 256-step chunk, summed by sum_partials_kernel, whose 16 waves take the slabs 16 apart, four
    at a time from 49 slabs on: T = 2 with B = 1 (15 idle waves), 17 (wave 0 takes two, the tail loop), 65 (wave 0 runs the unrolled
    loop once, then the tail loop); B = 9 at T = 257, two chunks per utterance: 18 slabs, the second of each utterance of one step
    (the tail loop again).  dw / dbias against float64, bit-equal across two runs"""
    T, C, K = SLAB_T[B], 64, 3
    inputs, r64, r32 = _case(B, T, C, K)
    got = _run_gpu(inputs, B, T)
    _check(f"B {B}", got, r32, r64, names=("dw", "dbias"))


@pytest.mark.parametrize("T", [1, 65])
def test_zr_route_at_a_ragged_channel_tile(T):
    """tavsr_dwconv_gate_bwd_act (K = 31: dr written as the gradient w.r.t. zr, r = gelu(zr)) at C = 67: dr bit-equal to the plain
    backward followed by ops.act_bwd_ (the identity tests/test_gpu_ops.py::test_dwconv_gate asserts at C = 1024), dgn / dw /
    dbias bit-equal to the plain backward's"""
    from tavsr import ops
    from tavsr._lib import ACT
    B, C, K = 3, 67, 31
    M = B * T
    (r, gn, du, w, b), _, _ = _case(B, T, C, K)
    (_, rg), (drbuf, drg) = _wide(r, M, C), _wide(None, M, C)
    gng, dug, wg, bg = gn.reshape(M, C).cuda(), du.reshape(M, C).cuda(), w.cuda(), b.cuda()
    torch.manual_seed(T)
    z = torch.randn(M, C, device="cuda")
    zbuf, zg = _wide(z.cpu(), M, C)
    _, conv = ops.dwconv_gate_fwd(gng, rg, wg, bg, B, T)
    want_dr = torch.full((M, C), NAN, device="cuda")
    dgn, dw, db = ops.dwconv_gate_bwd(dug, gng, rg, conv, wg, want_dr, B, T)
    ops.act_bwd_(want_dr, z, "gelu")
    dw2, db2 = torch.full((C, K), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    dgn2 = _raw_bwd("tavsr_dwconv_gate_bwd_act", dug, gng, rg, conv, wg, drg, dw2, db2, 0, B, T, zg.data_ptr(), zg.stride(0), ACT["gelu"])
    assert bool(torch.isfinite(want_dr).all())
    assert torch.equal(drg, want_dr)
    assert torch.equal(dgn2, dgn) and torch.equal(dw2, dw) and torch.equal(db2, db)
    assert bool(torch.isnan(drbuf[:, C:]).all()) and bool(torch.isnan(zbuf[:, C:]).all())


# ------------------------------------------------------------------------------------------------ 3. refusals
def _refused(rc, outputs):
    from tavsr._lib import TavsrError, check
    with pytest.raises(TavsrError, match="rc=-3"):
        check(rc, "refusal")
    assert all(bool(torch.isnan(t).all()) for t in outputs)      # nothing was launched


def test_refusals_launch_nothing():
    """supported: every odd K from 1 to 63 (include/tavsr.h).  K = 0, an even K and K = 65 are refused by the forward and the
    backward; the fused forward takes K = 31 and whole 64-channel tiles only, the zr backward K = 31 only - TAVSR_EUNSUPPORTED
    (-3) each, with NaN-filled outputs left as they were"""
    from tavsr import ops
    from tavsr._lib import ACT, lib, ptr, stream
    B, T, C = 2, 3, 128
    M = B * T
    nan = lambda *s: torch.full(s, NAN, device="cuda")
    x, g = torch.randn(M, C, device="cuda"), torch.randn(M, 2 * C, device="cuda")
    w, bias = torch.randn(C, 65, device="cuda"), torch.randn(C, device="cuda")      # (room for every K tried)
    for K in (0, 2, 65):
        out, conv = nan(M, C), nan(M, C)
        _refused(lib().tavsr_dwconv_gate_fwd(ptr(x), ptr(g), 2 * C, ptr(w), ptr(bias), ptr(out), ptr(conv), B, T, C, K, stream()), (out, conv))
        outs = dr, dgn, dw, db, ws = nan(M, C), nan(M, C), nan(C, 65), nan(C), nan(3 * C * 66)
        _refused(lib().tavsr_dwconv_gate_bwd(ptr(x), ptr(x), ptr(g), 2 * C, ptr(x), ptr(w), ptr(dr), C, ptr(dgn), ptr(dw), ptr(db), 0, ptr(ws),
                                             B, T, C, K, stream()), outs)
        assert not ops.csgu_usable(g, w[:, :K])
    outs = dr, dgn, dw, db, ws = nan(M, C), nan(M, C), nan(C, 7), nan(C), nan(3 * C * 8)
    _refused(lib().tavsr_dwconv_gate_bwd_act(ptr(x), ptr(x), ptr(g), 2 * C, ptr(x), ptr(w), ptr(dr), C, ptr(dgn), ptr(dw), ptr(db), 0, ptr(ws),
                                             B, T, C, 7, ptr(g), 2 * C, ACT["gelu"], stream()), outs)
    for Cn, K in ((C, 7), (96, 31)):
        gg = torch.randn(M, 2 * Cn, device="cuda")
        assert not ops.csgu_usable(gg, w[:Cn, :K])
        outs = out, gn, conv, mean, rstd = nan(M, Cn), nan(M, Cn), nan(M, Cn), nan(M), nan(M)
        _refused(lib().tavsr_csgu_fwd(ptr(gg), 2 * Cn, ptr(bias), ptr(bias), 1e-12, ptr(w), ptr(bias), ptr(out), ptr(gn), ptr(conv), ptr(mean),
                                      ptr(rstd), 0.0, None, 0, B, T, Cn, K, None, stream()), outs)
    assert ops.csgu_usable(g, w[:, :31]) == bool(ops.CSGU_FUSED)      # (the shape the fused forward does take)


# ------------------------------------------------------------------------------------------------ 4. the branch, unfused
BRANCH_LENS = (20, 13, 1)


@pytest.mark.parametrize("K", [3, 45])
def test_cgmlp_branch_on_its_unfused_route(K, monkeypatch):
    """CgmlpBranch.fwd / bwd (tavsr/layer_blocks.py) at cgmlp_linear_units = 192: C = 96 is no multiple of the channel tile, so
    csgu_usable is false and the branch runs LayerNorm + tavsr_dwconv_gate_fwd, and the backward without zr (the gate form of the
    tile core at both K).  D = 64, utterances of (20, 13, 1) frames padded to T = 20 with the loss on the valid frames; output (valid frames),
    input gradient and every parameter gradient against oracle.leaves.ConvolutionalGatingMLP in float64"""
    from oracle import leaves as L
    from oracle.model import fill_parameters_, synth
    from tavsr import ops
    from tavsr.layer_blocks import CgmlpBranch
    B, T, D, units = len(BRANCH_LENS), max(BRANCH_LENS), 64, 192
    ref = L.ConvolutionalGatingMLP(D, units, K, 0.0, False, "identity").eval()
    fill_parameters_(ref, seed=300 + K)
    x, dy = synth((B, T, D), seed=71), synth((B, T, D), seed=72)
    valid = torch.arange(T)[None, :] < torch.tensor(BRANCH_LENS)[:, None]
    dy = dy * valid[:, :, None]
    sd = {n: v.float() for n, v in ref.state_dict().items()}
    res = {}
    for dt in (torch.float64, torch.float32):
        m = ref.to(dt)
        m.zero_grad()
        xx = x.to(dt).clone().requires_grad_()
        y = m(xx, None)
        (y * dy.to(dt)).sum().backward()
        res[dt] = (y.detach(), xx.grad.clone(), {n: q.grad.clone() for n, q in m.named_parameters()})
    (y64, dx64, g64), (y32, dx32, g32) = res[torch.float64], res[torch.float32]

    p = {"cgmlp." + n: v.cuda() for n, v in sd.items()}
    n_rows = x.reshape(B * T, D).cuda()
    assert not ops.csgu_usable(torch.empty(B * T, units, device="cuda"), p["cgmlp.csgu.conv.weight"])
    calls = []
    fwd, bwd = ops.dwconv_gate_fwd, ops.dwconv_gate_bwd
    monkeypatch.setattr(ops, "dwconv_gate_fwd", lambda *a, **k: (calls.append("fwd"), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "dwconv_gate_bwd", lambda *a, **k: (calls.append(("bwd", k.get("zr") is None)), bwd(*a, **k))[1])
    u, saved = CgmlpBranch.fwd(n_rows, p, B, T, 0.0, True)
    yg = ops.linear(u, p["cgmlp.channel_proj2.weight"], p["cgmlp.channel_proj2.bias"])
    G, grp = {}, ops.WgradGroup()
    dn = CgmlpBranch.bwd(dy.reshape(B * T, D).cuda(), saved, p, B, T, grp, G)
    grp.flush()
    assert calls == ["fwd", ("bwd", True)], calls      # the gate kernels, without the K = 31 zr route
    v = valid.reshape(-1)
    ratios = [_bounded("y (valid frames)", yg.cpu()[v], y32.reshape(B * T, D)[v], y64.reshape(B * T, D)[v], 1e-5, value=True),
              _bounded("dx", dn, dx32.reshape(B * T, D), dx64.reshape(B * T, D), 1e-4)]
    assert set(G) == {"cgmlp." + n for n in g64}
    for n in sorted(g64):
        ratios.append(_bounded(n, G["cgmlp." + n].reshape(g64[n].shape), g32[n], g64[n], 1e-4))
    print(f"  CgmlpBranch K {K}: worst ratio {max(ratios):.2f}")
