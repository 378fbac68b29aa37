"""GPU: E-Branchformer on the HIP path - the merge convolution kernel (csrc/dwconv_time.hip), the layer, the encoder, train-mode
dropout with graph capture, and the recipe model end to end - against tests/ebf_ref.py in float64.

Tolerance (the convention of tests/test_gpu_rnnt.py / test_gpu_vocab.py): the same chain is evaluated by ebf_ref in fp32 on the
CPU; its error against float64 (e32) is what fp32 costs this computation, and the GPU may be four times as far from float64,
never asked for less than the project's floors - the kernel alone: 1e-5 on values, 1e-4 on gradients (test_gpu_vocab.py); layer
and encoder: 1e-4 on activations, 1e-3 on gradients (ACT_TOL / GRAD_TOL of tests/test_gpu_parity.py, with its relu_gated_tol for
the embedding's convolutions).  Values are compared as max |a - b| / max |b|, gradients as relative L2.  Every case prints both
errors and their ratio before it asserts.

Measured on an MI355X on the commit that added the test (gpu error / e32, the worst over a case's outputs and, for the kernel, over
the eight T; the errors themselves are 2e-8 ... 1e-6, so every bound that decided was a floor or 4 e32 with room; K = 15 and
T = 257 measured when they were added, the other figures did not move):
  kernel   C 128: K 1 1.26, K 3 1.42, K 15 2.58, K 31 3.58   C 192: 1.23, 1.49, 2.39, 3.49   C 520: 1.10, 1.32, 2.53, 2.69
           (K = 15, 31: u and dx, whose 15- / 31-term sums the CPU convolution adds in another order; dw / dbias stay below 2.4)
  layer    D 64 k 3 1.35, D 64 k 31 1.29, D 96 k 3 1.29, D 96 k 31 1.25;  D 64 k 3 by (use_ffn, macaron): (F, F) 1.60, (T, F) 1.38,
           (F, T) 1.43, (T, T) 1.35
  encoder  plain 1.62, intermediate CTC with conditioning 1.43
  dropout  frozen-mask central difference against the gradient norm: 7.1e-6 (k 3), 4.8e-5 (k 31) of the 3e-2 bound
"""
import argparse
import functools

import numpy as np
import pytest
import torch
import yaml

import ebf_ref as R
from helpers import max_rel, rel_err, relu_gated_tol
from test_ebf_host import EBF_YAML

pytestmark = pytest.mark.gpu

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
    print(f"    {name:<44} gpu {e_gpu:.3e}   fp32-on-cpu {e_f32:.3e}   ratio {e_gpu / max(e_f32, 1e-30):.2f}")
    assert e_gpu <= max(floor, 4.0 * e_f32), (name, e_gpu, e_f32)
    return e_gpu / max(e_f32, 1e-30)


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
    x, du = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    w, b = torch.randn(C, K, generator=g) / K ** 0.5, torch.randn(C, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        xx, ww, bb = (t.to(dt).clone().requires_grad_() for t in (x, w, b))
        u = R.dwconv_add(xx, ww, bb)
        out[dt] = (u.detach(), *torch.autograd.grad(u, (xx, ww, bb), du.to(dt)))
    return x, du, w, b, out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("K", [1, 3, 15, 31])
@pytest.mark.parametrize("C", [128, 192, 520])
def test_dwconv_add_kernel_vs_float64(C, K):
    """forward and backward at every T of KERNEL_T (T = 15 / 16: half a window of K = 31 and one more, the kernel wider than the
    sequence; T = 100: two time tiles; T = 257: two backward chunks; C = 520: a ragged last wave), B = 3, rows strided wider than C, outputs pre-filled with
    NaN; dw / dbias bit-equal across two runs"""
    from tavsr import ops
    B, ld = 3, C + 8
    worst = 0.0
    for T in KERNEL_T:
        x, du, w, b, r64, r32 = _kernel_case(C, K, T)
        assert ops.dwconv_add_ok(B, T, C, K)
        M = B * T

        def strided(t):
            buf = torch.full((M, ld), float("nan"), device="cuda")
            if t is not None:
                buf[:, :C] = t.reshape(M, C).cuda()
            return buf, buf[:, :C]

        (_, xg), (_, dug), (ubuf, ug), (dxbuf, dxg) = strided(x), strided(du), strided(None), strided(None)
        wg, bg = w.cuda(), b.cuda()
        _nan_blocks(C * K, C, max(1, ops.lib().tavsr_dwconv_add_bwd_ws(B, T, C, K)))
        ops.dwconv_add_fwd(xg, wg, bg, B, T, out=ug)
        dx, dw, db = ops.dwconv_add_bwd(dug, xg, wg, B, T, dx=dxg)
        _, dw2, db2 = ops.dwconv_add_bwd(dug, xg, wg, B, T)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), (T, "dw / dbias differ between two runs")
        assert bool(torch.isnan(ubuf[:, C:]).all()) and bool(torch.isnan(dxbuf[:, C:]).all())      # nothing beyond the C columns
        print(f"  C {C} K {K} T {T}")
        got = (ug.reshape(B, T, C), dx.reshape(B, T, C), dw, db)
        for n, g_, a, c, fl, val in zip(("u", "dx", "dw", "dbias"), got, r32, r64, (1e-5, 1e-4, 1e-4, 1e-4), (True, False, False, False)):
            worst = max(worst, _bounded(n, g_, a, c, fl, value=val))
    print(f"  C {C} K {K}: worst ratio {worst:.2f}")


def test_dwconv_add_refusals_launch_nothing():
    from tavsr import ops
    from tavsr._lib import TavsrError
    x = torch.randn(6, 128, device="cuda")
    for K in (2, 33):
        assert not ops.dwconv_add_ok(2, 3, 128, K)
        with pytest.raises(TavsrError, match="rc=-3"):
            ops.dwconv_add_fwd(x, torch.randn(128, K, device="cuda"), torch.randn(128, device="cuda"), 2, 3)
        with pytest.raises(TavsrError, match="rc=-3"):
            ops.dwconv_add_bwd(x, x, torch.randn(128, K, device="cuda"), 2, 3)


# ------------------------------------------------------------------------------------------------ 2. the layer
LAYER_LENS = (20, 13, 1)


def _layer_modules(D, H, k, use_ffn, macaron, ref):
    if ref:
        from oracle import leaves as M
        act = M.get_activation("swish")
        cls = R.EBranchformerLayerRef
    else:
        from tavsr import layers as M
        from tavsr.encoder.e_branchformer import EBranchformerEncoderLayer as cls
        act = "swish"
    ffn = lambda: M.PositionwiseFeedForward(D, 128, 0.0, act)
    return cls(D, M.RelPositionMultiHeadedAttention(H, D, 0.0), M.ConvolutionalGatingMLP(D, 128, 7, 0.0, False, "identity"),
               ffn() if use_ffn else None, ffn() if macaron else None, 0.0, k)


def _valid(t, lens=LAYER_LENS):
    return torch.cat([t[b, :n] for b, n in enumerate(lens)])


@functools.lru_cache(maxsize=None)
def _layer_reference(D, H, k, use_ffn, macaron):
    """(state_dict, inputs, {dtype: (y, dx, {parameter: gradient})}) of one reference layer in eval mode: loss = <y, r> over the
    valid frames"""
    from oracle import leaves as L
    from oracle.model import fill_parameters_, synth
    B, T = len(LAYER_LENS), max(LAYER_LENS)
    ref = _layer_modules(D, H, k, use_ffn, macaron, ref=True).eval()
    fill_parameters_(ref, seed=100 + k)
    x, r = synth((B, T, D), seed=41), synth((B, T, D), seed=42)
    mask = (torch.arange(T)[None, :] < torch.tensor(LAYER_LENS)[:, None])[:, None, :]
    r = r * mask.transpose(1, 2)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = ref.to(dt)
        m.zero_grad()
        xx = x.to(dt).clone().requires_grad_()
        pos = L.RelPositionalEncoding(D, 0.0)(xx.detach())[1]
        y = m((xx, pos), mask)[0][0]
        (y * r.to(dt)).sum().backward()
        out[dt] = (y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    sd = {n: v.float() for n, v in ref.state_dict().items()}
    return sd, (x, r, mask), out


def _run_layer_parity(D, H, k, use_ffn, macaron):
    from tavsr.layers import RelPositionalEncoding
    sd, (x, r, mask), out = _layer_reference(D, H, k, use_ffn, macaron)
    layer = _layer_modules(D, H, k, use_ffn, macaron, ref=False)
    layer.load_state_dict(sd)
    layer = layer.cuda().eval()
    xg = x.detach().cuda().requires_grad_()
    pos = RelPositionalEncoding(D, 0.0)(xg.detach())[1]
    y = layer((xg, pos), mask.cuda())[0][0]
    (y * r.cuda()).sum().backward()
    (y64, dx64, g64), (y32, dx32, g32) = out[torch.float64], out[torch.float32]
    ratios = [_bounded("y (valid frames)", _valid(y), _valid(y32), _valid(y64), 1e-4, value=True),
              _bounded("dx (valid frames)", _valid(xg.grad), _valid(dx32), _valid(dx64), 1e-3)]
    got = dict(layer.named_parameters())
    assert set(got) == set(g64)
    for n in sorted(g64):
        assert got[n].grad is not None, n
        ratios.append(_bounded(n, got[n].grad, g32[n], g64[n], 1e-3))
    print(f"  layer D {D} H {H} k {k} ffn {use_ffn} macaron {macaron}: worst ratio {max(ratios):.2f}")


@pytest.mark.parametrize("k", [3, 31])
@pytest.mark.parametrize("D,H", [(64, 2), (96, 3)])
def test_layer_parity_forward_and_all_gradients(D, H, k):
    """eval mode, B = 3, T = 20, lengths (20, 13, 1): the valid frames of the output and of the input gradient, and every parameter
    gradient.  The last (k-1)/2 valid frames of the short utterances read padded frames of the concatenated branch outputs (with
    k = 31 every frame does): they agree only if the padded rows hold what espnet computes there."""
    _run_layer_parity(D, H, k, True, True)


@pytest.mark.parametrize("use_ffn,macaron", [(False, False), (True, False), (False, True), (True, True)])
def test_layer_parity_feed_forward_combinations(use_ffn, macaron):
    """the four feed_forward / feed_forward_macaron combinations of the layer (ff_scale 0.5 with the macaron block, else 1.0;
    without the closing block norm_final is a LayerNorm of its own).  The encoder refuses macaron_ffn without use_ffn; the layer,
    like espnet's, takes the two modules independently."""
    _run_layer_parity(64, 2, 3, use_ffn, macaron)


# ------------------------------------------------------------------------------------------------ 3. the encoder
ENC_KW = dict(input_size=80, output_size=64, attention_heads=2, cgmlp_linear_units=128, cgmlp_conv_kernel=7, num_blocks=2,
              dropout_rate=0.0, positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer="conv2d", use_ffn=True,
              macaron_ffn=True, linear_units=128, merge_conv_kernel=3)
ENC_ILENS, ENC_V = (83, 55, 31), 12


@functools.lru_cache(maxsize=None)
def _encoder_reference(interctc):
    from oracle.model import CTCOracle, fill_parameters_, synth
    kw = dict(ENC_KW, **(dict(interctc_layer_idx=[1], interctc_use_conditioning=True) if interctc else {}))
    holder = torch.nn.Module()
    holder.encoder, holder.ctc = R.EBranchformerEncoderRef(**kw), CTCOracle(ENC_V, 64)
    if interctc:
        holder.encoder.conditioning_layer = torch.nn.Linear(ENC_V, 64)
    fill_parameters_(holder, seed=77)
    holder.eval()
    B, T = len(ENC_ILENS), max(ENC_ILENS)
    x = synth((B, T, 80), seed=51)
    ilens = torch.tensor(ENC_ILENS)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = holder.to(dt)
        m.zero_grad()
        ys, olens, _ = m.encoder(x.to(dt), ilens, ctc=m.ctc)
        ys, inter = ys if interctc else (ys, [])
        r = synth(tuple(ys.shape), seed=52).to(dt)
        r2 = synth(tuple(ys.shape), seed=53).to(dt)
        loss = sum((_valid(o, olens.tolist()) * _valid(q, olens.tolist())).sum() for o, q in zip([ys] + [o for _, o in inter], (r, r2)))
        loss.backward()
        out[dt] = (ys.detach(), [o.detach() for _, o in inter], olens, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    return kw, {n: v.float() for n, v in holder.state_dict().items()}, x, ilens, out


@pytest.mark.parametrize("interctc", [False, True], ids=["plain", "interctc-conditioning"])
def test_encoder_parity(interctc):
    """2 blocks behind Conv2dSubsampling on ragged 80-dim input; with interctc_layer_idx=[1] and conditioning the tap after layer
    1 and the conditioning's gradients (conditioning_layer, ctc_lo) are compared too.  The CPU reference module's state_dict is
    loaded into the HIP module key for key (strict)."""
    from oracle.model import synth
    from tavsr.ctc.ctc import CTC
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    kw, sd, x, ilens, out = _encoder_reference(interctc)
    holder = torch.nn.Module()
    holder.encoder, holder.ctc = EBranchformerEncoder(**kw), CTC(ENC_V, 64)
    if interctc:
        holder.encoder.conditioning_layer = torch.nn.Linear(ENC_V, 64)
    assert set(holder.state_dict()) == set(sd)
    holder.load_state_dict(sd, strict=True)
    holder = holder.cuda().eval()
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
    for n in sorted(g64):
        ratios.append(_bounded(n, got[n].grad, g32[n], g64[n], relu_gated_tol(n, 1e-3)))
    print(f"  encoder interctc {interctc}: worst ratio {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------ 3b. the C-side layer route
@pytest.mark.parametrize("kind", ["branchformer", "e_branchformer"])
def test_eager_training_step_route_through_the_c_side_layer(kind, monkeypatch):
    """an eager (un-captured) training step of the recipe's Branchformer layer (learned_ave, D = 256) still runs forward AND backward
    as the C-side calls, once per layer: the E-Branchformer parameters must not leave ``None`` entries in its parameter list.  The
    E-Branchformer layer itself never takes the C-side route (the sequencer is not extended)."""
    from tavsr import functional as F_
    from tavsr import ops
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    from tavsr.layers import RelPositionalEncoding
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = F_._layer_c_forward, F_._layer_c_backward
    monkeypatch.setattr(F_, "_layer_c_forward", lambda *a: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a))[1])
    monkeypatch.setattr(F_, "_layer_c_backward", lambda *a: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a))[1])
    torch.manual_seed(0)
    B, T, D = 3, 40, 256
    kw = dict(input_size=D, num_blocks=2, input_layer=None, dropout_rate=0.1, positional_dropout_rate=0.0, attention_dropout_rate=0.1,
              ffn_activation_type="swish")
    enc = (MyBranchformerEncoder(merge_method="learned_ave", **kw) if kind == "branchformer"
           else EBranchformerEncoder(use_ffn=True, macaron_ffn=True, merge_conv_kernel=31, **kw)).cuda().train()
    xs, pos = RelPositionalEncoding(D, 0.0)(torch.randn(B, T, D, device="cuda"))
    xs = xs.detach().requires_grad_()
    lens = torch.tensor([40, 27, 20], device="cuda")
    h, mask = (xs, pos), (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    ops.manual_seed(11)
    for layer in enc.encoders:
        h, mask = layer(h, mask)
    h[0].sum().backward()
    assert bool(torch.isfinite(xs.grad).all())
    want = 2 if (kind == "branchformer" and ops.LAYER_C) else 0      # (TAVSR_LAYER_C=0 switches the route off for every layer)
    assert calls == {"fwd": want, "bwd": want}, calls


# ------------------------------------------------------------------------------------------------ 4. dropout, graph capture
def _dropout_encoder(k):
    from oracle.model import fill_parameters_, synth
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    from tavsr.layers import RelPositionalEncoding
    B, T, D = 3, 40, 256
    enc = EBranchformerEncoder(input_size=D, output_size=D, attention_heads=4, num_blocks=2, input_layer=None, dropout_rate=0.1,
                               positional_dropout_rate=0.0, attention_dropout_rate=0.1, cgmlp_linear_units=1024, linear_units=1024,
                               use_ffn=True, macaron_ffn=True, merge_conv_kernel=k)
    fill_parameters_(enc, seed=17)
    enc = enc.cuda().train()
    xs, pos = RelPositionalEncoding(D, 0.0)(synth((B, T, D), seed=8).cuda())
    lens = torch.tensor([40, 27, 20], device="cuda")
    mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    r = synth((B, T, D), seed=10).cuda().double()

    def loss_at():
        from tavsr import ops
        ops.manual_seed(2024)
        h, m = (xs, pos), mask
        for layer in enc.encoders:
            h, m = layer(h, m)
        return (h[0].double() * r).sum()
    return enc, loss_at


@pytest.mark.parametrize("k", [3, 31])
def test_layers_backward_under_frozen_masks(k):
    """dropout 0.1 in training: tests/test_gpu_dropout.py's check of the Branchformer layer (central difference of the loss along
    the gradient direction with the masks frozen by re-seeding, 0.2 % step, 3e-2 bound) on two E-Branchformer layers: the
    backward applies the masks the forward drew (the concat buffer's, the merge projection's, the blocks')"""
    enc, loss_at = _dropout_encoder(k)
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
    print(f"frozen-mask E-Branchformer layers k {k}: fd {fd:.6g} gnorm {gnorm:.6g} rel {abs(fd - gnorm) / gnorm:.3e}")
    assert abs(fd - gnorm) / gnorm < 3e-2, (fd, gnorm)


def test_captured_dropout_step_replays_the_eager_bits():
    """the same seeded step (seed, forward, backward) captured under torch.cuda.graph: every replay gives the loss and the
    gradients of the eager launches, bit for bit"""
    enc, loss_at = _dropout_encoder(31)
    params = list(enc.encoders.parameters())

    def step():
        for p in params:
            p.grad = None
        loss = loss_at()
        loss.backward()
        return loss

    eager_loss = step().detach().clone()
    eager = [p.grad.detach().clone() for p in params]
    assert any(float((g == 0).float().mean()) < 1.0 for g in eager)
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
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.detach(), eager_loss), replay
        bad = [n for (n, p), g in zip(enc.encoders.named_parameters(), eager) if not torch.equal(p.grad, g)]
        assert not bad, (replay, bad[:8])
    del graph


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_recipe_model_trains_and_decodes():
    """the recipe at 2 encoder blocks / 1 decoder block on 80-dim features: finite loss and gradients for every parameter, and
    Speech2Text(model, beam_size=2) returns text"""
    from oracle.model import fill_parameters_, synth
    from tavsr.inference import Speech2Text
    from tavsr.tasks.asr import ASRTask
    conf = yaml.safe_load(open(EBF_YAML))
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"]["num_blocks"] = 2
    conf["decoder_conf"]["num_blocks"] = 1
    model = ASRTask.build_model(argparse.Namespace(**conf))
    fill_parameters_(model, seed=5)
    model = model.cuda().train()
    speech, slens = synth((2, 100, 80), seed=8).cuda(), torch.tensor([100, 76]).cuda()
    text, tlens = synth((2, 6), seed=9, kind="int", lo=1, hi=40), torch.tensor([6, 4]).cuda()
    text[1, 4:] = -1
    loss = model(speech, slens, text.cuda(), tlens)[0]
    loss.backward()
    assert bool(torch.isfinite(loss))
    missing = [n for n, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing[:8]
    assert float(model.encoder.encoders[0].depthwise_conv_fusion.weight.grad.abs().max()) > 0
    res = Speech2Text(model.eval(), beam_size=2)(speech, slens)
    assert len(res) == 2
    for nbest in res:
        text_out, token, token_int = nbest[0][:3]
        assert isinstance(text_out, str) and len(token) == len(token_int)
