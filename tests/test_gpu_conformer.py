"""GPU: Conformer on the HIP path - the GLU + depthwise convolution kernel (csrc/dwconv_time.hip), the convolution module in
train and eval mode, the layer, the encoder, train-mode dropout with graph capture, and the recipe model end to end - against
tests/conformer_ref.py in float64.

Tolerance (the convention of tests/test_gpu_ebf.py): the same chain is evaluated by conformer_ref in fp32 on the CPU; its error
against float64 (e32) is what fp32 costs this computation, and the GPU may be four times as far from float64, never asked for less
than the project's floors - the kernel alone: 1e-5 on values, 1e-4 on gradients; module, layer and encoder: 1e-4 on activations,
1e-3 on gradients (with helpers.relu_gated_tol for the embedding's convolutions).  Values are compared as max |a - b| / max |b|,
gradients as relative L2.  Every case prints both errors and their ratio before it asserts.

``depthwise_conv.bias`` has a bound of its own: in train mode BatchNorm removes a per-channel shift, so its gradient is
analytically zero (|float64| ~ 1e-13, the fp32 CPU chain gives rounding noise of ~1e-5) and a relative error means nothing.  It is
bounded absolutely by max(4 * max |fp32-on-CPU value|, 1e-4 * max |d norm.weight in float64|).

Measured on an MI355X on the commit that added the test (gpu error / e32, the worst over a case's outputs and, for the kernel, over
the eight T; the errors themselves are 5e-8 ... 7e-6, so every bound that decided was a floor or 4 e32 with room):
  kernel   C 128: K 1 1.24, K 3 1.21, K 15 3.57, K 31 3.05   C 192: 1.15, 1.53, 3.91, 3.04   C 520: 1.26, 1.35, 2.29, 2.93
           (K >= 15: z, 2e-7 ... 3.5e-7 against 5e-8 ... 1e-7 - the hardware sigmoid and the order of the tap sum - under the 1e-5 floor)
  module   train D 64 K 3 1.41, D 64 K 31 1.13, D 96 K 3 1.25, D 96 K 31 1.12; depthwise_conv.bias max |gpu| 1e-5 ... 2.3e-5 against
           max |fp32-on-cpu| 8e-6 ... 1.1e-5 and bounds of 8.5e-4 ... 9.8e-4
  layer    D 64 K 3 by (macaron, conv): (F, F) 1.31, (T, F) 1.04, (F, T) 1.32, (T, T) 1.52;  D 96 K 31 1.33
  encoder  plain 1.44, intermediate CTC with conditioning 1.70;  recipe model 1.40
  dropout  frozen-mask central difference against the gradient norm: 8.9e-5 (K 3), 1.1e-4 (K 31) of the 3e-2 bound
"""
import argparse
import functools

import numpy as np
import pytest
import torch
import yaml

import conformer_ref as R
from helpers import max_rel, rel_err, relu_gated_tol
from test_conformer_host import CONFORMER_YAML

pytestmark = pytest.mark.gpu

DW_BIAS = "depthwise_conv.bias"


def _bounded(name, gpu, f32, f64, floor, value=False):
    """|gpu - f64| <= max(floor, 4 |f32 - f64|); a gradient that is analytically zero (linear_k.bias: softmax shift invariance)
    is rounding noise on every side and is bounded absolutely, as helpers.grad_ok does"""
    err = max_rel if value else rel_err
    gpu, f64 = gpu.detach().cpu(), f64.detach()
    assert bool(torch.isfinite(gpu).all()), name
    if float(f64.abs().max()) < 1e-6:
        assert float(gpu.abs().max()) < 1e-5, name
        return 0.0
    e_gpu, e_f32 = err(gpu, f64), err(f32.detach(), f64)
    print(f"    {name:<52} gpu {e_gpu:.3e}   fp32-on-cpu {e_f32:.3e}   ratio {e_gpu / max(e_f32, 1e-30):.2f}")
    assert e_gpu <= max(floor, 4.0 * e_f32), (name, e_gpu, e_f32)
    return e_gpu / max(e_f32, 1e-30)


def _dw_bias_bounded(name, gpu, f32, bn_weight_grad64):
    """the analytically-zero gradient of the depthwise convolution's bias in train mode: absolute bound (module docstring)"""
    gpu = gpu.detach().cpu()
    assert bool(torch.isfinite(gpu).all()), name
    a_gpu, a_f32 = float(gpu.abs().max()), float(f32.abs().max())
    bound = max(4.0 * a_f32, 1e-4 * float(bn_weight_grad64.abs().max()))
    print(f"    {name:<52} max|gpu| {a_gpu:.3e}   max|fp32-on-cpu| {a_f32:.3e}   bound {bound:.3e}")
    assert a_gpu <= bound, (name, a_gpu, bound)


def _grads_bounded(got, g32, g64, floor=1e-3, tol=lambda n, t: t):
    """every parameter gradient of a module against the references; -> ratios"""
    ratios = []
    for n in sorted(g64):
        assert got[n].grad is not None, n
        if n.endswith(DW_BIAS):
            _dw_bias_bounded(n, got[n].grad, g32[n], g64[n[:-len(DW_BIAS)] + "norm.weight"])
        else:
            ratios.append(_bounded(n, got[n].grad, g32[n], g64[n], tol(n, floor)))
    return ratios


def _nan_blocks(*numels):
    """leave NaN in the allocator's cached blocks of these sizes (what TAVSR_POISON=nan does for the whole suite): an output
    element that a kernel does not write then reads NaN"""
    blocks = [torch.full((n,), float("nan"), device="cuda") for n in numels for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
KERNEL_T = (1, 2, 15, 16, 17, 33, 100, 257)      # 257: one step beyond the backward's time chunk of 256 (two partial slabs)


@functools.lru_cache(maxsize=None)
def _kernel_case(C, K, T, B=3):
    g = torch.Generator().manual_seed(1000 * C + 10 * K + T)
    h, dz = torch.randn(B, T, 2 * C, generator=g), torch.randn(B, T, C, generator=g)
    w, b = torch.randn(C, K, generator=g) / K ** 0.5, torch.randn(C, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        hh, ww, bb = (t.to(dt).clone().requires_grad_() for t in (h, w, b))
        z = R.glu_dwconv(hh, ww, bb)
        out[dt] = (z.detach(), *torch.autograd.grad(z, (hh, ww, bb), dz.to(dt)))
    return h, dz, w, b, out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("K", [1, 3, 15, 31])
@pytest.mark.parametrize("C", [128, 192, 520])
def test_glu_dwconv_kernel_vs_float64(C, K):
    """forward and backward at every T of KERNEL_T (T = 15 / 16: half a window of K = 31 and one more, the kernel wider than the
    sequence - with B = 3 a halo that read the neighbouring utterance's rows would show; T = 100: two time tiles; T = 257: two
    backward chunks; C = 520: a ragged last wave), rows strided wider than the data, outputs pre-filled with NaN and nothing
    written beyond the data columns; dw / dbias bit-equal across two runs"""
    from tavsr import ops
    B = 3
    worst = 0.0
    for T in KERNEL_T:
        h, dz, w, b, r64, r32 = _kernel_case(C, K, T)
        assert ops.glu_dwconv_ok(B, T, C, K)
        M = B * T

        def strided(t, n):
            buf = torch.full((M, n + 8), float("nan"), device="cuda")
            if t is not None:
                buf[:, :n] = t.reshape(M, n).cuda()
            return buf, buf[:, :n]

        (_, hg), (_, dzg), (zbuf, zg), (dhbuf, dhg) = strided(h, 2 * C), strided(dz, C), strided(None, C), strided(None, 2 * C)
        wg, bg = w.cuda(), b.cuda()
        _nan_blocks(C * K, C, max(1, ops.lib().tavsr_glu_dwconv_bwd_ws(B, T, C, K)))
        ops.glu_dwconv_fwd(hg, wg, bg, B, T, out=zg)
        dh, dw, db = ops.glu_dwconv_bwd(dzg, hg, wg, B, T, dh=dhg)
        _, dw2, db2 = ops.glu_dwconv_bwd(dzg, hg, wg, B, T)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), (T, "dw / dbias differ between two runs")
        assert bool(torch.isnan(zbuf[:, C:]).all()) and bool(torch.isnan(dhbuf[:, 2 * C:]).all())      # nothing beyond the data
        print(f"  C {C} K {K} T {T}")
        got = (zg.reshape(B, T, C), dh.reshape(B, T, 2 * C), dw, db)
        for n, g_, a, c, fl, val in zip(("z", "dh", "dw", "dbias"), got, r32, r64, (1e-5, 1e-4, 1e-4, 1e-4), (True, False, False, False)):
            worst = max(worst, _bounded(n, g_, a, c, fl, value=val))
    print(f"  C {C} K {K}: worst ratio {worst:.2f}")


def test_glu_dwconv_refusals_launch_nothing():
    from tavsr import ops
    from tavsr._lib import TavsrError
    h, dz = torch.randn(6, 256, device="cuda"), torch.randn(6, 128, device="cuda")
    for K in (2, 33):
        assert not ops.glu_dwconv_ok(2, 3, 128, K)
        z = torch.full((6, 128), float("nan"), device="cuda")
        with pytest.raises(TavsrError, match="rc=-3"):
            ops.glu_dwconv_fwd(h, torch.randn(128, K, device="cuda"), torch.randn(128, device="cuda"), 2, 3, out=z)
        dh = torch.full((6, 256), float("nan"), device="cuda")
        with pytest.raises(TavsrError, match="rc=-3"):
            ops.glu_dwconv_bwd(dz, h, torch.randn(128, K, device="cuda"), 2, 3, dh=dh)
        assert bool(torch.isnan(z).all()) and bool(torch.isnan(dh).all())      # nothing was launched


# ------------------------------------------------------------------------------------------------ 2. the convolution module
MOD_B, MOD_T = 3, 20


@functools.lru_cache(maxsize=None)
def _module_reference(D, K):
    """two train-mode steps of the reference module on (x1, x2) with loss = <y, r>, then an eval-mode forward of x1 ->
    (state_dict before, inputs, {dtype: (y1, dx1, grads1, running_mean, running_var, nbt, y_eval)})"""
    from oracle import leaves as L
    from oracle.model import fill_parameters_, synth
    ref = R.ConvolutionModuleRef(D, K, L.get_activation("swish"))
    fill_parameters_(ref, seed=200 + K)
    sd = {n: v.clone() for n, v in ref.state_dict().items()}
    x1, x2, r = synth((MOD_B, MOD_T, D), seed=61), synth((MOD_B, MOD_T, D), seed=62), synth((MOD_B, MOD_T, D), seed=63)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = R.ConvolutionModuleRef(D, K, L.get_activation("swish"))
        m.load_state_dict(sd)
        m = m.to(dt).train()
        xx = x1.to(dt).clone().requires_grad_()
        y = m(xx)
        (y * r.to(dt)).sum().backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters()}
        with torch.no_grad():
            m(x2.to(dt))
            ye = m.eval()(x1.to(dt))
        out[dt] = (y.detach(), xx.grad.clone(), grads, m.norm.running_mean.clone(), m.norm.running_var.clone(),
                   int(m.norm.num_batches_tracked), ye)
    return sd, (x1, x2, r), out


@pytest.mark.parametrize("K", [3, 31])
@pytest.mark.parametrize("D", [64, 96])
def test_conv_module_train_mode(D, K):
    """train mode, B = 3, T = 20 (M = 60 rows of batch statistics): the output, dx and every parameter gradient; after a second
    train-mode forward (under no_grad: torch updates the statistics there too) running_mean / running_var and
    num_batches_tracked == 2"""
    from tavsr.encoder.conformer import ConvolutionModule
    sd, (x1, x2, r), out = _module_reference(D, K)
    mod = ConvolutionModule(D, K, "swish")
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().train()
    xg = x1.cuda().requires_grad_()
    y = mod(xg)
    (y * r.cuda()).sum().backward()
    (y64, dx64, g64, rm64, rv64, nbt64, _), (y32, dx32, g32, rm32, rv32, _, _) = out[torch.float64], out[torch.float32]
    ratios = [_bounded("y", y, y32, y64, 1e-4, value=True), _bounded("dx", xg.grad, dx32, dx64, 1e-3)]
    got = dict(mod.named_parameters())
    assert set(got) == set(g64)
    ratios += _grads_bounded(got, g32, g64)
    with torch.no_grad():
        mod(x2.cuda())
    assert int(mod.norm.num_batches_tracked) == nbt64 == 2
    ratios.append(_bounded("running_mean", mod.norm.running_mean, rm32, rm64, 1e-4, value=True))
    ratios.append(_bounded("running_var", mod.norm.running_var, rv32, rv64, 1e-4, value=True))
    print(f"  conv module train D {D} K {K}: worst ratio {max(ratios):.2f}")


def test_conv_module_eval_mode_uses_running_statistics_and_refuses_backward():
    """eval mode: the output comes from the running statistics (which two train-mode steps moved) and the buffers stay as they
    are; a backward through eval mode (autograd recording) raises, as the lip front-end's eval-mode BatchNorm does"""
    from tavsr.encoder.conformer import ConvolutionModule
    D, K = 64, 3
    sd, (x1, x2, _), out = _module_reference(D, K)
    mod = ConvolutionModule(D, K, "swish")
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().train()
    with torch.no_grad():
        mod(x1.cuda())
        mod(x2.cuda())
        mod.eval()
        before = {n: b.clone() for n, b in mod.named_buffers()}
        ye = mod(x1.cuda())
    assert all(torch.equal(b, before[n]) for n, b in mod.named_buffers())
    _bounded("y (eval)", ye, out[torch.float32][6], out[torch.float64][6], 1e-4, value=True)
    # ... and not from the batch's own statistics: the train-mode output of the same input is another one
    assert max_rel(ye.cpu(), out[torch.float64][0]) > 1e-3
    with pytest.raises(NotImplementedError, match="eval-mode BatchNorm"):
        mod(x1.cuda().requires_grad_()).sum().backward()


# ------------------------------------------------------------------------------------------------ 3. the layer
LAYER_LENS = (20, 13, 1)


def _layer_modules(D, H, K, macaron, conv, ref, p=0.0):
    if ref:
        from oracle import leaves as M
        act = M.get_activation("swish")
        cm = R.ConvolutionModuleRef(D, K, M.get_activation("swish")) if conv else None
        cls = R.ConformerLayerRef
    else:
        from tavsr import layers as M
        from tavsr.encoder.conformer import ConvolutionModule
        from tavsr.encoder.conformer import EncoderLayer as cls
        act = "swish"
        cm = ConvolutionModule(D, K, "swish") if conv else None
    ffn = lambda: M.PositionwiseFeedForward(D, 128, p, act)
    return cls(D, M.RelPositionMultiHeadedAttention(H, D, p), ffn(), ffn() if macaron else None, cm, p)


def _valid(t, lens=LAYER_LENS):
    return torch.cat([t[b, :n] for b, n in enumerate(lens)])


@functools.lru_cache(maxsize=None)
def _layer_reference(D, H, K, macaron, conv):
    """(state_dict, inputs, {dtype: (y, dx, {parameter: gradient})}) of one reference layer in train mode at dropout 0 (BatchNorm
    on batch statistics over all B*T rows, padded ones included): loss = <y, r> over the valid frames"""
    from oracle import leaves as L
    from oracle.model import fill_parameters_, synth
    B, T = len(LAYER_LENS), max(LAYER_LENS)
    ref = _layer_modules(D, H, K, macaron, conv, ref=True)
    fill_parameters_(ref, seed=100 + K)
    sd = {n: v.clone() for n, v in ref.state_dict().items()}
    x, r = synth((B, T, D), seed=41), synth((B, T, D), seed=42)
    mask = (torch.arange(T)[None, :] < torch.tensor(LAYER_LENS)[:, None])[:, None, :]
    r = r * mask.transpose(1, 2)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = _layer_modules(D, H, K, macaron, conv, ref=True)
        m.load_state_dict(sd)
        m = m.to(dt).train()
        xx = x.to(dt).clone().requires_grad_()
        pos = L.RelPositionalEncoding(D, 0.0)(xx.detach())[1]
        y = m((xx, pos), mask)[0][0]
        (y * r.to(dt)).sum().backward()
        out[dt] = (y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    return sd, (x, r, mask), out


def _run_layer_parity(D, H, K, macaron, conv):
    from tavsr.layers import RelPositionalEncoding
    sd, (x, r, mask), out = _layer_reference(D, H, K, macaron, conv)
    layer = _layer_modules(D, H, K, macaron, conv, ref=False)
    layer.load_state_dict(sd, strict=True)
    layer = layer.cuda().train()
    xg = x.detach().cuda().requires_grad_()
    pos = RelPositionalEncoding(D, 0.0)(xg.detach())[1]
    y = layer((xg, pos), mask.cuda())[0][0]
    (y * r.cuda()).sum().backward()
    (y64, dx64, g64), (y32, dx32, g32) = out[torch.float64], out[torch.float32]
    ratios = [_bounded("y (valid frames)", _valid(y), _valid(y32), _valid(y64), 1e-4, value=True),
              _bounded("dx (valid frames)", _valid(xg.grad), _valid(dx32), _valid(dx64), 1e-3)]
    got = dict(layer.named_parameters())
    assert set(got) == set(g64)
    ratios += _grads_bounded(got, g32, g64)
    if conv:
        assert int(layer.conv_module.norm.num_batches_tracked) == 1
    print(f"  layer D {D} H {H} K {K} macaron {macaron} conv {conv}: worst ratio {max(ratios):.2f}")


@pytest.mark.parametrize("macaron,conv", [(False, False), (True, False), (False, True), (True, True)])
def test_layer_parity_block_combinations(macaron, conv):
    """train mode at dropout 0, B = 3, T = 20, lengths (20, 13, 1), D 64, K 3: the valid frames of the output and of the input
    gradient, and every parameter gradient, for the four (macaron_style, use_cnn_module) pairs.  The convolution reads padded
    frames and BatchNorm's statistics include them: the valid frames agree only if the padded rows hold what espnet computes."""
    _run_layer_parity(64, 2, 3, macaron, conv)


def test_layer_parity_kernel_31():
    """D 96 (three heads of 32: the unfused attention core), K 31 wider than every utterance, both optional blocks on"""
    _run_layer_parity(96, 3, 31, True, True)


# ------------------------------------------------------------------------------------------------ 4. the encoder
ENC_KW = dict(input_size=80, output_size=64, attention_heads=2, linear_units=128, num_blocks=2, dropout_rate=0.0,
              positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer="conv2d", macaron_style=True, rel_pos_type="latest",
              use_cnn_module=True, cnn_module_kernel=7)
ENC_ILENS, ENC_V = (83, 55, 31), 12


def _enc_holder(kw, interctc, ref):
    from oracle.model import CTCOracle
    from tavsr.ctc.ctc import CTC
    from tavsr.encoder.conformer import ConformerEncoder
    holder = torch.nn.Module()
    holder.encoder, holder.ctc = (R.ConformerEncoderRef(**kw), CTCOracle(ENC_V, 64)) if ref else (ConformerEncoder(**kw), CTC(ENC_V, 64))
    if interctc:
        holder.encoder.conditioning_layer = torch.nn.Linear(ENC_V, 64)
    return holder


@functools.lru_cache(maxsize=None)
def _encoder_reference(interctc):
    from oracle.model import fill_parameters_, synth
    kw = dict(ENC_KW, **(dict(interctc_layer_idx=[1], interctc_use_conditioning=True) if interctc else {}))
    holder = _enc_holder(kw, interctc, ref=True)
    fill_parameters_(holder, seed=77)
    sd = {n: v.clone() for n, v in holder.state_dict().items()}
    B, T = len(ENC_ILENS), max(ENC_ILENS)
    x = synth((B, T, 80), seed=51)
    ilens = torch.tensor(ENC_ILENS)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = _enc_holder(kw, interctc, ref=True)
        m.load_state_dict(sd)
        m = m.to(dt).train()
        ys, olens, _ = m.encoder(x.to(dt), ilens, ctc=m.ctc)
        ys, inter = ys if interctc else (ys, [])
        r = synth(tuple(ys.shape), seed=52).to(dt)
        r2 = synth(tuple(ys.shape), seed=53).to(dt)
        loss = sum((_valid(o, olens.tolist()) * _valid(q, olens.tolist())).sum() for o, q in zip([ys] + [o for _, o in inter], (r, r2)))
        loss.backward()
        out[dt] = (ys.detach(), [o.detach() for _, o in inter], olens, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    return kw, sd, x, ilens, out


@pytest.mark.parametrize("interctc", [False, True], ids=["plain", "interctc-conditioning"])
def test_encoder_parity(interctc):
    """2 blocks behind Conv2dSubsampling on ragged 80-dim input, train mode at dropout 0; with interctc_layer_idx=[1] and
    conditioning the tap after layer 1 and the conditioning's gradients (conditioning_layer, ctc_lo) are compared too.  The CPU
    reference module's state_dict is loaded into the HIP module key for key (strict)."""
    from oracle.model import synth
    kw, sd, x, ilens, out = _encoder_reference(interctc)
    holder = _enc_holder(kw, interctc, ref=False)
    assert set(holder.state_dict()) == set(sd)
    holder.load_state_dict(sd, strict=True)
    holder = holder.cuda().train()
    ys, olens, _ = holder.encoder(x.cuda(), ilens.cuda(), ctc=holder.ctc)
    ys, inter = ys if interctc else (ys, [])
    (y64, i64, ol64, g64), (y32, i32, _, g32) = out[torch.float64], out[torch.float32]
    assert olens.tolist() == ol64.tolist() and len(inter) == len(i64)
    ol = ol64.tolist()
    r, r2 = synth(tuple(ys.shape), seed=52).cuda(), synth(tuple(ys.shape), seed=53).cuda()
    loss = sum((_valid(o, ol) * _valid(q, ol)).sum() for o, q in zip([ys] + [o for _, o in inter], (r, r2)))
    loss.backward()
    ratios = [_bounded("encoder out (valid frames)", _valid(ys, ol), _valid(y32, ol), _valid(y64, ol), 1e-4, value=True)]
    for (idx, o), a, c in zip(inter, i32, i64):
        assert idx == 1
        ratios.append(_bounded("tap after layer 1", _valid(o, ol), _valid(a, ol), _valid(c, ol), 1e-4, value=True))
    got = {n: p for n, p in holder.named_parameters()}
    assert set(n for n, p in got.items() if p.grad is not None) == set(g64)
    ratios += _grads_bounded(got, g32, g64, tol=relu_gated_tol)
    print(f"  encoder interctc {interctc}: worst ratio {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------ 5. dropout, graph capture
def _dropout_encoder(K, p=0.1, seeded=True):
    from oracle.model import fill_parameters_, synth
    from tavsr import ops
    from tavsr.encoder.conformer import ConformerEncoder
    from tavsr.layers import RelPositionalEncoding
    B, T, D = 3, 40, 256
    enc = ConformerEncoder(input_size=D, output_size=D, attention_heads=4, num_blocks=2, input_layer=None, dropout_rate=p,
                           positional_dropout_rate=0.0, attention_dropout_rate=p, linear_units=1024, macaron_style=True,
                           rel_pos_type="latest", cnn_module_kernel=K)
    fill_parameters_(enc, seed=17)
    enc = enc.cuda().train()
    xs, pos = RelPositionalEncoding(D, 0.0)(synth((B, T, D), seed=8).cuda())
    lens = torch.tensor([40, 27, 20], device="cuda")
    mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    r = synth((B, T, D), seed=10).cuda().double()

    def loss_at():
        if seeded:
            ops.manual_seed(2024)      # the same masks at every call
        else:
            ops.rng_step_begin()       # a kernel advances the generator: new masks at every call and at every graph replay
        h, m = (xs, pos), mask
        for layer in enc.encoders:
            h, m = layer(h, m)
        return (h[0].double() * r).sum()
    return enc, loss_at


@pytest.mark.parametrize("K", [3, 31])
def test_layers_backward_under_frozen_masks(K):
    """dropout 0.1 in training: tests/test_gpu_ebf.py's check (central difference of the loss along the gradient direction with the
    masks frozen by re-seeding, 0.2 % step, 3e-2 bound) on two Conformer layers: the backward applies the masks the forward drew
    (the four blocks' outer ones, the feed-forward blocks' inner ones, the attention's)"""
    enc, loss_at = _dropout_encoder(K)
    enc.zero_grad()
    loss_at().backward()
    params = [p for p in enc.parameters() if p.grad is not None]
    assert len(params) == len(list(enc.encoders.parameters()))      # (after_norm is not part of the layer loop)
    grads = [p.grad.detach().clone() for p in params]
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    assert np.isfinite(gnorm) and gnorm > 0
    eps = 2e-3 / gnorm * float(torch.sqrt(sum((p.double() ** 2).sum() for p in params)))
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.add_(g, alpha=eps / gnorm)
        lp = float(loss_at())
        for p, g in zip(params, grads):
            p.add_(g, alpha=-2 * eps / gnorm)
        lm = float(loss_at())
    fd = (lp - lm) / (2 * eps)
    print(f"frozen-mask Conformer layers K {K}: fd {fd:.6g} gnorm {gnorm:.6g} rel {abs(fd - gnorm) / gnorm:.3e}")
    assert abs(fd - gnorm) / gnorm < 3e-2, (fd, gnorm)


def _capture(enc, loss_at):
    params = list(enc.encoders.parameters())

    def step():
        for p in params:
            p.grad = None
        loss = loss_at()
        loss.backward()
        return loss

    eager_loss = step().detach().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = loss_at()
        static_loss.backward()
    return graph, static_loss, eager_loss


def test_captured_dropout_step_draws_new_masks_and_counts_its_batches():
    """a train step (generator advance, forward, backward) captured under torch.cuda.graph and replayed twice: the masks differ
    between the replays (the losses do), every gradient is finite, and num_batches_tracked advances once per replay"""
    from tavsr import ops
    ops.manual_seed(99)
    enc, loss_at = _dropout_encoder(31, seeded=False)
    try:
        graph, static_loss, _ = _capture(enc, loss_at)
        nbt = lambda: [int(l.conv_module.norm.num_batches_tracked) for l in enc.encoders]
        n0, losses = nbt(), []
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            losses.append(float(static_loss))
            assert nbt() == [n + replay + 1 for n in n0], (replay, n0, nbt())
            assert all(bool(torch.isfinite(p.grad).all()) for p in enc.encoders.parameters())
        assert np.isfinite(losses).all() and losses[0] != losses[1], losses
        del graph
    finally:
        ops.manual_seed(0)      # (drops the pass-local seed the capture left behind)


def test_captured_step_without_dropout_replays_the_eager_bits():
    """at dropout 0 the captured loss equals the eager one bit for bit (BatchNorm's batch statistics are reduced in a fixed order)"""
    enc, loss_at = _dropout_encoder(31, p=0.0)
    graph, static_loss, eager_loss = _capture(enc, loss_at)
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.detach(), eager_loss), replay
    del graph


# ------------------------------------------------------------------------------------------------ 6. end to end
def _recipe_conf():
    conf = yaml.safe_load(open(CONFORMER_YAML))
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"].update(num_blocks=2, output_size=64, attention_heads=2, linear_units=128, dropout_rate=0.0,
                                positional_dropout_rate=0.0, attention_dropout_rate=0.0)
    conf["decoder_conf"].update(num_blocks=1, attention_heads=2, linear_units=128, dropout_rate=0.0, positional_dropout_rate=0.0,
                                self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0)
    conf["ctc_conf"]["dropout_rate"] = 0.0
    return conf


def _recipe_oracle(conf):
    from oracle import leaves as L
    from oracle.model import ASRModelOracle, CTCOracle
    from tavsr.utils.tokens import CHAR_ENGLISH
    ec = {k: v for k, v in conf["encoder_conf"].items()
          if k not in ("normalize_before", "pos_enc_layer_type", "positionwise_layer_type", "selfattention_layer_type")}
    V = len(CHAR_ENGLISH)
    encoder = R.ConformerEncoderRef(input_size=80, **ec)
    decoder = L.TransformerDecoder(vocab_size=V, encoder_output_size=64, **conf["decoder_conf"])
    return ASRModelOracle(vocab_size=V, token_list=list(CHAR_ENGLISH), frontend=None, specaug=None,
                          normalize=L.UtteranceMVN(**conf["normalize_conf"]), encoder=encoder, decoder=decoder,
                          ctc=CTCOracle(odim=V, encoder_output_size=64, **conf["ctc_conf"]), **conf["model_conf"])


@functools.lru_cache(maxsize=None)
def _recipe_reference():
    import copy

    from oracle.model import fill_parameters_, synth
    conf = _recipe_conf()
    base = _recipe_oracle(copy.deepcopy(conf))
    fill_parameters_(base, seed=5)
    sd = {n: v.clone() for n, v in base.state_dict().items()}
    speech, slens = synth((2, 100, 80), seed=8), torch.tensor([100, 76])
    text, tlens = synth((2, 6), seed=9, kind="int", lo=1, hi=40), torch.tensor([6, 4])
    text[1, 4:] = -1
    out = {}
    for dt in (torch.float64, torch.float32):
        m = _recipe_oracle(copy.deepcopy(conf))
        m.load_state_dict(sd)
        m = m.to(dt).train()
        loss = m(speech.to(dt), slens, text, tlens)[0]
        loss.backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        m.load_state_dict({k: v.to(dt) for k, v in sd.items()})      # the running statistics as they were, for the eval pass
        with torch.no_grad():
            enc, olens = m.eval().encode(speech.to(dt), slens)
        out[dt] = (loss.detach(), grads, enc, olens)
    return conf, sd, (speech, slens, text, tlens), out


def test_recipe_model_train_eval_and_decode():
    """the recipe shrunk to 2 encoder blocks / 1 decoder block at D 64: train mode - loss and every gradient against the
    restatement; eval mode - the encoder output (BatchNorm on the running statistics); Speech2Text(model, beam_size=2) returns
    text"""
    import copy

    from tavsr.inference import Speech2Text
    from tavsr.tasks.asr import ASRTask
    conf, sd, (speech, slens, text, tlens), out = _recipe_reference()
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    assert set(model.state_dict()) == set(sd)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    (l64, g64, e64, ol64), (l32, g32, e32, _) = out[torch.float64], out[torch.float32]
    loss = model(speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda())[0]
    loss.backward()
    ratios = [_bounded("loss", loss.reshape(1), l32.reshape(1), l64.reshape(1), 1e-4, value=True)]
    got = dict(model.named_parameters())
    assert set(n for n, p in got.items() if p.grad is not None) == set(g64)
    ratios += _grads_bounded(got, g32, g64, tol=relu_gated_tol)
    model.load_state_dict(sd, strict=True)
    model.eval()
    with torch.no_grad():
        enc, olens = model.encode(speech.cuda(), slens.cuda())
    ol = ol64.tolist()
    assert olens.tolist() == ol
    ratios.append(_bounded("encoder out, eval (valid frames)", _valid(enc, ol), _valid(e32, ol), _valid(e64, ol), 1e-4, value=True))
    print(f"  recipe model: worst ratio {max(ratios):.2f}")
    res = Speech2Text(model, beam_size=2)(speech.cuda(), slens.cuda())
    assert len(res) == 2
    for nbest in res:
        text_out, token, token_int = nbest[0][:3]
        assert isinstance(text_out, str) and len(token) == len(token_int)
