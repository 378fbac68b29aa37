"""GPU: the Branchformer attention branch beyond rel_selfattn / rel_pos - Fastformer's additive attention (csrc/fastattn.hip),
plain multi-head attention and the absolute positional encodings - kernel, layer, encoder, train-mode dropout with graph capture
and the recipe model end to end, against tests/fastattn_ref.py in float64.

Tolerance (the convention of tests/test_gpu_ebf.py): the same chain is evaluated by the restatement in fp32 on the CPU; its error
against float64 (e32) is what fp32 costs this computation, and the GPU may be four times as far from float64, never asked for less
than the project's floors - the kernel alone: 1e-5 on values, 1e-4 on gradients; layer and encoder: 1e-4 on activations, 1e-3 on
gradients (relu_gated_tol for the embedding's convolutions).  Values are compared as max |a - b| / max |b|, gradients as relative
L2; gradients that are analytically zero (query_att.bias, key_att.bias, linear_k.bias, the two score weights at T = 1) are bounded
absolutely at 1e-5.  Every case prints both errors and their ratio before it asserts.

Measured on an MI355X on the commit that added the test (gpu error / e32, the worst over a case's outputs and, for the kernels, over
the eight T; the kernels' own errors stay below 4e-6, so every bound that decided was a floor or 4 e32 with room; per-T rows in
profiles/fastattn_edges.txt):
  kernels  D 64 H 4 2.04, D 256 H 4 1.83, D 64 H 8 2.07, D 96 H 4 2.83, D 256 H 1 2.25
  layer    fast_selfattn abs_pos learned_ave 1.37, fast_selfattn abs_pos concat 1.54, fast_selfattn scaled_abs_pos learned_ave 1.33, fast_selfattn scaled_abs_pos concat 1.35
           selfattn abs_pos learned_ave 1.30, selfattn abs_pos concat 1.33, selfattn scaled_abs_pos learned_ave 3.06, selfattn scaled_abs_pos concat 2.42
  encoder  fast plain 1.44, fast interctc 2.66, selfattn-dk64 plain 2.43, selfattn-dk64 interctc 5.94, selfattn-dk16 plain 6.05, selfattn-dk16 interctc 1.41
           (the ratios above 4 are merge-weight gradients - weight_proj1.bias 4.2e-6 against an e32 of 7.1e-7, pooling_proj1.weight
           6.4e-5 against 1.1e-5; in the model weight_proj1.bias 1.1e-5 against 2.3e-6 - all under the 1e-3 floor)
  model    4.69
  dropout  frozen-mask central difference against the gradient norm: fast_selfattn 9.493e-05, selfattn 8.541e-05 of the 3e-2 bound
"""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import fastattn_ref as R
from helpers import ROOT, max_rel, rel_err, relu_gated_tol

pytestmark = pytest.mark.gpu

FAST_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "branchformer_fast", "asr_branchformer_fast_transformer_ctc_english.yaml")


def _bounded(name, gpu, f32, f64, floor, value=False):
    """|gpu - f64| <= max(floor, 4 |f32 - f64|); an analytically zero gradient is bounded absolutely (tests/test_gpu_ebf.py)"""
    err = max_rel if value else rel_err
    gpu, f64 = gpu.detach().cpu(), f64.detach()
    assert bool(torch.isfinite(gpu).all()), name
    if float(f64.abs().max()) < 1e-6:
        assert float(gpu.abs().max()) < 1e-5, (name, float(gpu.abs().max()))
        return 0.0
    e_gpu, e_f32 = err(gpu, f64), err(f32.detach(), f64)
    print(f"    {name:<44} gpu {e_gpu:.3e}   fp32-on-cpu {e_f32:.3e}   ratio {e_gpu / max(e_f32, 1e-30):.2f}")
    assert e_gpu <= max(floor, 4.0 * e_f32), (name, e_gpu, e_f32)
    return e_gpu / max(e_f32, 1e-30)


def _nan_blocks(*numels):
    """leave NaN in the allocator's cached blocks of these sizes: an output element that a kernel does not write then reads NaN"""
    blocks = [torch.full((max(1, n),), float("nan"), device="cuda") for n in numels for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


def _fill(module, seed):
    """oracle's fill_parameters_ on every parameter but the 0-dim ones, which it does not take (ScaledPositionalEncoding.alpha:
    set to 0.7, away from its initial 1.0)"""
    from oracle.model import fill_parameters_
    scalars = [(m, n, p) for m in module.modules() for n, p in list(m._parameters.items()) if p is not None and p.dim() == 0]
    for m, n, _ in scalars:
        del m._parameters[n]
    try:
        fill_parameters_(module, seed=seed)
    finally:
        for m, n, p in scalars:
            m._parameters[n] = p
    for _, _, p in scalars:
        p.data.fill_(0.7)


def _lens(T):
    return (T, max(1, T // 2), 1)


def _valid(t, lens):
    return torch.cat([t[b, :n] for b, n in enumerate(lens)])


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
# 65: one frame beyond the 64-frame block of the row-parallel launches (kFaRows; two partial slabs per utterance); 130: three blocks;
# 257: one beyond the 256 threads that stride over time in the pooling launch; 500: the long end of the recipe's range
KERNEL_T = (1, 2, 63, 64, 65, 130, 257, 500)
KERNEL_DH = [(64, 4), (256, 4), (64, 8), (96, 4), (256, 1)]      # dh 16, 64, 8, 24 (a channel tail: 24 of 64 lanes), 256
NAMES = ("wv", "alpha", "beta", "pq", "pk", "dq", "dk", "query_att.weight", "query_att.bias", "key_att.weight", "key_att.bias")
IS_VALUE = (True, True, True, True, True, False, False, False, False, False, False)


@functools.lru_cache(maxsize=None)
def _kernel_case(D, H, T, B=3):
    """inputs and, per dtype, (wv, alpha, beta, pq, pk, dq, dk, d query_att.weight, .bias, d key_att.weight, .bias) of
    loss = <wv, dwv> + <q, dres> with every row of dwv / dres random (the padded ones too: the reference's wv exists there)"""
    g = torch.Generator().manual_seed(100000 * D + 1000 * H + T)
    q, k, dwv, dres = (torch.randn(B, T, D, generator=g) for _ in range(4))
    wq, wk = (torch.randn(H, D, generator=g) * 0.3 for _ in range(2))
    bq, bk = (torch.randn(H, generator=g) for _ in range(2))
    lens = torch.tensor(_lens(T))
    out = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt).clone().requires_grad_() for t in (q, k, wq, bq, wk, bk)]
        wv, alpha, beta, pq, pk = R.fast_core(*leaves, lens, H)
        grads = torch.autograd.grad((wv * dwv.to(dt)).sum() + (leaves[0] * dres.to(dt)).sum(), leaves)
        out[dt] = tuple(t.detach() for t in (wv, alpha, beta, pq, pk)) + grads
    return (q, k, dwv, dres, wq, bq, wk, bk, lens), out[torch.float64], out[torch.float32]


def _run_core(q, k, dwv, dres, wq, bq, wk, bk, lens, H):
    from tavsr import ops
    B, T, D = q.shape
    M = B * T
    qk = torch.cat([q, k], dim=-1).reshape(M, 2 * D).cuda()
    dwv_g, dres_g = dwv.reshape(M, D).cuda(), dres.reshape(M, D).cuda()
    wq, bq, wk, bk, lens = (t.cuda() for t in (wq, bq, wk, bk, lens))
    _nan_blocks(B * H * T, B * D, M * D, M * 2 * D, H * D + H, ops.lib().tavsr_fastattn_bwd_ws(B, T, D, H))
    wv, kept = ops.fastattn_fwd(qk, wq, bq, wk, bk, lens, B, T, D, H)
    alpha, pq_pre, pq, _, beta, pk_pre, pk, _ = kept
    assert pq is pq_pre and pk is pk_pre      # (no dropout)
    dqk, gwq, gbq, gwk, gbk = ops.fastattn_bwd(dwv_g, dres_g, qk, kept, wq, wk, lens, B, T, D, H)
    dqk = dqk.reshape(B, T, 2 * D)
    return (wv.reshape(B, T, D), alpha, beta, pq, pk, dqk[..., :D], dqk[..., D:], gwq, gbq, gwk, gbk)


@pytest.mark.parametrize("D,H", KERNEL_DH)
def test_fastattn_kernels_vs_float64(D, H):
    """forward and backward at every T of KERNEL_T, B = 3 with lengths (T, max(1, T // 2), 1); each case once more after leaving NaN
    in the allocator's cached blocks (an output element left unwritten would read it), the two backward runs bit-equal"""
    from tavsr import ops
    assert ops.fastattn_ok(D, H) and ops.lib().tavsr_fastattn_ok(D, H) == 1
    worst = 0.0
    for T in KERNEL_T:
        ins, r64, r32 = _kernel_case(D, H, T)
        got = _run_core(*ins, H)
        again = _run_core(*ins, H)
        for n, a, b in zip(NAMES, got, again):
            assert torch.equal(a, b), (T, n, "differs between two runs")
        print(f"  D {D} H {H} T {T}")
        for n, g_, a, c, val in zip(NAMES, got, r32, r64, IS_VALUE):
            worst = max(worst, _bounded(n, g_, a, c, 1e-5 if val else 1e-4, value=val))
    print(f"  D {D} H {H}: worst ratio {worst:.2f}")


def test_fastattn_refusals_launch_nothing():
    from tavsr import ops
    from tavsr._lib import TavsrError
    for D, H in ((72, 12), (516, 1), (60, 5), (66, 4), (60, 6)):      # too many heads, too wide, (60, 5) is fine, H does not divide D, dh = 10
        ok = 1 <= H <= 8 and D <= 512 and D % H == 0 and (D // H) % 4 == 0
        assert ops.fastattn_ok(D, H) == ok and ops.lib().tavsr_fastattn_ok(D, H) == int(ok)
        if ok:
            continue
        qk = torch.randn(6, 2 * D, device="cuda")
        with pytest.raises(TavsrError, match="rc=-3"):
            ops.fastattn_pool(qk, 0, None, torch.randn(H, D, device="cuda"), torch.randn(H, device="cuda"),
                              torch.tensor([3, 2], device="cuda"), 2, 3, D, H)


# ------------------------------------------------------------------------------------------------ 2. mask exactness
@pytest.mark.parametrize("D,H", [(64, 4), (256, 4)])
def test_padded_frames_are_never_read(D, H):
    """NaN in the padded frames of q and k while ``lens`` marks them out: pq, pk, the weights, every valid row of wv, dq and dk and
    the four score gradients are finite and equal the run with zeros there, bit for bit.  The upstream gradients are zero at the
    padded frames (a loss over the valid frames): d pk = sum_t dwv * q is the one sum the reference takes over every row."""
    T = 130
    (q, k, dwv, dres, wq, bq, wk, bk, lens), _, _ = _kernel_case(D, H, T)
    pad = (torch.arange(T)[None, :] >= lens[:, None])[:, :, None]
    dwv, dres = dwv.masked_fill(pad, 0.0), dres.masked_fill(pad, 0.0)
    runs = []
    for fill in (0.0, float("nan")):
        runs.append(_run_core(q.masked_fill(pad, fill), k.masked_fill(pad, fill), dwv, dres, wq, bq, wk, bk, lens, H))
    ll = lens.tolist()
    for n, a, b in zip(NAMES, *runs):
        if n in ("wv", "dq", "dk"):
            a, b = _valid(a, ll), _valid(b, ll)
        assert bool(torch.isfinite(b).all()), n
        assert torch.equal(a, b), n
    for n, a in zip(NAMES, runs[1]):
        if n in ("alpha", "beta"):
            assert all(float(a[b_, :, n_:].abs().max()) == 0.0 for b_, n_ in enumerate(ll) if n_ < T), n      # exactly 0 at the padding
        if n == "dk":
            assert all(float(a[b_, n_:].abs().max()) == 0.0 for b_, n_ in enumerate(ll) if n_ < T)


# ------------------------------------------------------------------------------------------------ 3. the layer
LAYER_LENS, LAYER_D, LAYER_H = (37, 20, 1), 64, 4


def _layer_holder(kind, pos, merge, ref):
    """``embed`` = Sequential(positional encoding), ``layer`` = one Branchformer layer: embed.0.alpha is ScaledPositionalEncoding's"""
    D, H = LAYER_D, LAYER_H
    if ref:
        from oracle import leaves as M
        from oracle.model import BranchformerLayerOracle as cls
        act, fast = M.get_activation("swish"), R.FastSelfAttentionRef
    else:
        from tavsr import layers as M
        from tavsr.encoder.branchformer.encoder_layer import MyBranchformerEncoderLayer as cls
        act, fast = "swish", M.FastSelfAttention
    pe = {"abs_pos": M.PositionalEncoding, "scaled_abs_pos": M.ScaledPositionalEncoding}[pos](D, 0.0)
    attn = fast(D, H, 0.0) if kind == "fast_selfattn" else M.MultiHeadedAttention(H, D, 0.0)
    ffn = lambda: M.PositionwiseFeedForward(D, 128, 0.0, act)
    holder = torch.nn.Module()
    holder.embed = torch.nn.Sequential(pe)
    holder.layer = cls(D, attn, M.ConvolutionalGatingMLP(D, 128, 7, 0.0, False, "identity"), ffn(), ffn(), 0.0, merge)
    return holder


@functools.lru_cache(maxsize=None)
def _layer_reference(kind, pos, merge):
    from oracle.model import synth
    B, T, D = len(LAYER_LENS), max(LAYER_LENS), LAYER_D
    ref = _layer_holder(kind, pos, merge, ref=True).eval()
    _fill(ref, 300 + len(kind) + len(pos) + len(merge))
    x, r = synth((B, T, D), seed=41), synth((B, T, D), seed=42)
    mask = (torch.arange(T)[None, :] < torch.tensor(LAYER_LENS)[:, None])[:, None, :]
    r = r * mask.transpose(1, 2)
    out = {}
    for dt in (torch.float64, torch.float32):
        m = ref.to(dt)
        m.zero_grad()
        xx = x.to(dt).clone().requires_grad_()
        y = m.layer(m.embed(xx), mask)[0]
        (y * r.to(dt)).sum().backward()
        out[dt] = (y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    return {n: v.float() for n, v in ref.state_dict().items()}, (x, r, mask), out


@pytest.mark.parametrize("merge", ["learned_ave", "concat"])
@pytest.mark.parametrize("pos", ["abs_pos", "scaled_abs_pos"])
@pytest.mark.parametrize("kind", ["fast_selfattn", "selfattn"])
def test_layer_parity_forward_and_all_gradients(kind, pos, merge):
    """dropout 0, D = 64, H = 4, T = 37, lengths (37, 20, 1), the positional encoding in front of the layer: the valid frames of
    the output and of the input gradient and every parameter gradient (``embed.0.alpha`` with scaled_abs_pos); the restatement's
    state_dict loads strictly"""
    sd, (x, r, mask), out = _layer_reference(kind, pos, merge)
    holder = _layer_holder(kind, pos, merge, ref=False)
    assert set(holder.state_dict()) == set(sd)
    holder.load_state_dict(sd, strict=True)
    holder = holder.cuda().eval()
    xg = x.detach().cuda().requires_grad_()
    y = holder.layer(holder.embed(xg), mask.cuda())[0]
    assert torch.is_tensor(y)      # the tensor form: no (x, pos_emb)
    (y * r.cuda()).sum().backward()
    (y64, dx64, g64), (y32, dx32, g32) = out[torch.float64], out[torch.float32]
    ll = LAYER_LENS
    ratios = [_bounded("y (valid frames)", _valid(y, ll), _valid(y32, ll), _valid(y64, ll), 1e-4, value=True),
              _bounded("dx (valid frames)", _valid(xg.grad, ll), _valid(dx32, ll), _valid(dx64, ll), 1e-3)]
    got = dict(holder.named_parameters())
    assert set(got) == set(g64) and ("embed.0.alpha" in got) == (pos == "scaled_abs_pos")
    for n in sorted(g64):
        assert got[n].grad is not None, n
        ratios.append(_bounded(n, got[n].grad, g32[n], g64[n], 1e-3))
    print(f"  layer {kind} {pos} {merge}: worst ratio {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------ 4. the encoder
ENC_ILENS, ENC_V = (83, 55, 31), 12
# (attention, positional encoding, output_size, heads): the additive attention; plain attention on the fused core (dk = 64) and on
# the GEMM + softmax route (dk = 16)
ENC_KINDS = {"fast": ("fast_selfattn", "abs_pos", 64, 4), "selfattn-dk64": ("selfattn", "scaled_abs_pos", 128, 2),
             "selfattn-dk16": ("selfattn", "abs_pos", 64, 4)}


def _enc_kw(which, interctc):
    kind, pos, D, H = ENC_KINDS[which]
    kw = dict(input_size=80, output_size=D, attention_heads=H, cgmlp_linear_units=128, cgmlp_conv_kernel=7, num_blocks=2,
              dropout_rate=0.0, positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer="conv2d", linear_units=128,
              ffn_activation_type="swish", attention_layer_type=kind, pos_enc_layer_type=pos)
    if interctc:
        kw.update(interctc_layer_idx=[1], interctc_use_conditioning=True)
    return kw


@functools.lru_cache(maxsize=None)
def _encoder_reference(which, interctc):
    from oracle.model import CTCOracle, synth
    kw = _enc_kw(which, interctc)
    D = kw["output_size"]
    holder = torch.nn.Module()
    holder.encoder, holder.ctc = R.BranchformerEncoderRef(**kw), CTCOracle(ENC_V, D)
    if interctc:
        holder.encoder.conditioning_layer = torch.nn.Linear(ENC_V, D)
    _fill(holder, 77)
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
        ol = olens.tolist()
        r, r2 = synth(tuple(ys.shape), seed=52).to(dt), synth(tuple(ys.shape), seed=53).to(dt)
        loss = sum((_valid(o, ol) * _valid(q, ol)).sum() for o, q in zip([ys] + [o for _, o in inter], (r, r2)))
        loss.backward()
        out[dt] = (ys.detach(), [o.detach() for _, o in inter], olens, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    return kw, {n: v.float() for n, v in holder.state_dict().items()}, x, ilens, out


@pytest.mark.parametrize("interctc", [False, True], ids=["plain", "interctc-conditioning"])
@pytest.mark.parametrize("which", list(ENC_KINDS))
def test_encoder_parity(which, interctc):
    """2 blocks behind Conv2dSubsampling on ragged 80-dim input; with interctc_layer_idx=[1] and conditioning the tap after layer 1
    and the conditioning's gradients too.  The restatement's state_dict is loaded key for key (strict)."""
    from oracle.model import synth
    from tavsr.ctc.ctc import CTC
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    kw, sd, x, ilens, out = _encoder_reference(which, interctc)
    D = kw["output_size"]
    holder = torch.nn.Module()
    holder.encoder, holder.ctc = MyBranchformerEncoder(**kw), CTC(ENC_V, D)
    if interctc:
        holder.encoder.conditioning_layer = torch.nn.Linear(ENC_V, D)
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
    print(f"  encoder {which} interctc {interctc}: worst ratio {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------ 5. dropout, graph capture
def _dropout_encoder(kind, p=0.1, seeded=True):
    from oracle.model import synth
    from tavsr import ops
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    B, T, D = 3, 40, 256
    enc = MyBranchformerEncoder(input_size=D, output_size=D, attention_heads=4, num_blocks=2, input_layer=None, dropout_rate=p,
                                positional_dropout_rate=0.0, attention_dropout_rate=p, cgmlp_linear_units=1024, linear_units=1024,
                                attention_layer_type=kind, pos_enc_layer_type="abs_pos")
    _fill(enc, 17)
    enc = enc.cuda()
    xs = synth((B, T, D), seed=8).cuda()
    lens = torch.tensor([40, 27, 20], device="cuda")
    mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    r = synth((B, T, D), seed=10).cuda().double()

    def loss_at():
        if seeded:
            ops.manual_seed(2024)      # the same masks at every call
        else:
            ops.rng_step_begin()       # a kernel advances the generator: new masks at every call and at every graph replay
        h, m = xs, mask
        for layer in enc.encoders:
            h, m = layer(h, m)
        return (h.double() * r).sum()
    return enc, loss_at


@pytest.mark.parametrize("kind", ["fast_selfattn", "selfattn"])
def test_layers_backward_under_frozen_masks(kind):
    """dropout 0.1 in training: central difference of the loss along the gradient direction with the masks frozen by re-seeding
    (0.2 % step, the 3e-2 bound of tests/test_gpu_ebf.py) on two layers: the backward applies the masks the forward drew (pq, pk
    and the transform output among them)"""
    enc, loss_at = _dropout_encoder(kind)
    enc.train()
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
    print(f"frozen-mask {kind} layers: fd {fd:.6g} gnorm {gnorm:.6g} rel {abs(fd - gnorm) / gnorm:.3e}")
    assert abs(fd - gnorm) / gnorm < 3e-2, (fd, gnorm)


def test_eval_equals_zero_dropout():
    """eval mode of a p = 0.1 encoder gives the bits of the p = 0 encoder"""
    outs = []
    for p in (0.1, 0.0):
        enc, loss_at = _dropout_encoder("fast_selfattn", p=p)
        enc.eval()
        with torch.no_grad():
            outs.append(loss_at())
    assert torch.equal(*outs)


def test_captured_dropout_step_draws_fresh_masks_at_every_replay():
    """forward + backward at p = 0.1 captured under torch.cuda.graph with the generator advanced by a kernel inside the graph:
    nothing is read on the host (the lengths stay on the device), and two replays give different losses and gradients, both finite"""
    enc, loss_at = _dropout_encoder("fast_selfattn", seeded=False)
    enc.train()
    params = list(enc.encoders.parameters())

    def step():
        for p in params:
            p.grad = None
        loss = loss_at()
        loss.backward()
        return loss

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
    seen = []
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(static_loss))
        g = dict(enc.encoders.named_parameters())["0.attn.query_att.weight"].grad
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        seen.append((static_loss.detach().clone(), g.detach().clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
    del graph


# ------------------------------------------------------------------------------------------------ 6. the recipe model
def _recipe_conf():
    conf = yaml.safe_load(open(FAST_YAML))
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"]["num_blocks"] = 2
    conf["decoder_conf"]["num_blocks"] = 1
    for sub, keys in (("encoder_conf", ("dropout_rate", "positional_dropout_rate", "attention_dropout_rate")),
                      ("decoder_conf", ("dropout_rate", "positional_dropout_rate", "self_attention_dropout_rate", "src_attention_dropout_rate")),
                      ("ctc_conf", ("dropout_rate",))):
        for k in keys:
            conf[sub][k] = 0.0
    return conf


def test_recipe_model_trains_and_decodes_like_the_restatement():
    """the new recipe at 2 encoder blocks / 1 decoder block on 80-dim features: one forward + backward step - the loss and every
    gradient against the restatement (oracle's model around tests/fastattn_ref.py's encoder) - and Speech2Text on two ragged
    utterances returns the tokens the same search finds on the restatement's encoder output"""
    import copy

    from oracle.model import build_asr_oracle, synth
    from tavsr.inference import Speech2Text
    from tavsr.tasks.asr import ASRTask
    from tavsr.utils.tokens import CHAR_ENGLISH
    conf = _recipe_conf()
    oconf = copy.deepcopy(conf)
    oconf["encoder_conf"].update(attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos")
    oracle = build_asr_oracle(oconf, CHAR_ENGLISH)
    oracle.encoder = R.BranchformerEncoderRef(input_size=80, **copy.deepcopy(conf["encoder_conf"]))
    oracle = oracle.train()
    _fill(oracle, 5)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    assert type(model.encoder.encoders[0].attn).__name__ == "FastSelfAttention"
    model.load_state_dict(oracle.state_dict(), strict=True)
    model = model.cuda().train()
    speech, slens = synth((2, 100, 80), seed=8), torch.tensor([100, 76])
    text, tlens = synth((2, 6), seed=9, kind="int", lo=1, hi=40), torch.tensor([6, 4])
    text[1, 4:] = -1
    res = {}
    for dt in (torch.float64, torch.float32):
        m = oracle.to(dt)
        m.zero_grad()
        lo = m(speech.to(dt), slens, text, tlens)[0]
        lo.backward()
        res[dt] = (lo.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    loss = model(speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda())[0]
    loss.backward()
    assert bool(torch.isfinite(loss))
    (l64, g64), (l32, g32) = res[torch.float64], res[torch.float32]
    ratios = [_bounded("loss", loss.reshape(1), l32.reshape(1), l64.reshape(1), 1e-4, value=True)]
    got = dict(model.named_parameters())
    assert set(n for n, p in got.items() if p.grad is not None) == set(g64)
    for n in sorted(g64):
        ratios.append(_bounded(n, got[n].grad, g32[n], g64[n], relu_gated_tol(n, 1e-3)))
    print(f"  recipe model: worst ratio {max(ratios):.2f}")
    # decoding: the module's encoder against the restatement's encoder output under the same search
    s2t = Speech2Text(model.eval(), beam_size=3, ctc_weight=0.3, lm_weight=0.0)
    ours = s2t(speech.cuda(), slens.cuda())
    o32 = oracle.to(torch.float32).eval()
    with torch.no_grad():
        enc_ref, enc_lens = o32.encode(speech, slens)
    theirs = s2t._results(enc_ref.cuda(), enc_lens.cuda())
    assert len(ours) == 2
    for a, b in zip(ours, theirs):
        assert a[0][2] == b[0][2] and isinstance(a[0][0], str)


# ------------------------------------------------------------------------------------------------ 7. the default is unchanged
def test_default_options_are_the_relative_position_path_bit_for_bit(monkeypatch):
    """an encoder built without the new keywords and one with attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos"
    spelled out give the same bits for y and every gradient, and an eager training step still takes the C-side layer route"""
    from oracle.model import synth
    from tavsr import functional as F_
    from tavsr import ops
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    calls = {"fwd": 0}
    fwd = F_._layer_c_forward
    monkeypatch.setattr(F_, "_layer_c_forward", lambda *a: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a))[1])
    kw = dict(input_size=80, output_size=256, attention_heads=4, num_blocks=2, input_layer="conv2d", dropout_rate=0.0,
              positional_dropout_rate=0.0, attention_dropout_rate=0.0, cgmlp_linear_units=1024, linear_units=1024,
              ffn_activation_type="swish")
    x, ilens = synth((3, 83, 80), seed=51).cuda(), torch.tensor(ENC_ILENS).cuda()
    outs = []
    for extra in ({}, dict(attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos")):
        enc = MyBranchformerEncoder(**kw, **extra)
        _fill(enc, 3)
        enc = enc.cuda().train()
        calls["fwd"] = 0
        y, olens, _ = enc(x, ilens)
        (y * synth(tuple(y.shape), seed=52).cuda()).sum().backward()
        assert calls["fwd"] == (2 if ops.LAYER_C else 0)
        outs.append((y.detach(), {n: p.grad.clone() for n, p in enc.named_parameters()}))
    assert torch.equal(outs[0][0], outs[1][0]) and set(outs[0][1]) == set(outs[1][1])
    for n in outs[0][1]:
        assert torch.equal(outs[0][1][n], outs[1][1][n]), n
