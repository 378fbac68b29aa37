"""GPU: the transducer kernels (csrc/rnnt.hip) and everything built on them against the float64 restatements of
tests/rnnt_ref.py - the lattice, joint + loss in chunks, the LSTM recurrence, a whole transducer model's training step, and the
greedy search.

Tolerance rule of the joint + loss and LSTM tests (``_bounded``): the same chain is evaluated in fp32 with torch on the CPU; its
relative L2 error against float64 is what fp32 costs this computation, and the GPU result may be four times that far from
float64 (another summation order, not another algorithm)."""
import argparse
import os
import re

import pytest
import torch

import rnnt_ref as R
from helpers import ROOT, TOKENS_EN, grad_ok, rel_err
from test_rnnt_host import rnnt_conf

pytestmark = pytest.mark.gpu


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    print(f"    max-rel {err:.3e} (bar {tol:.0e})")
    assert err < tol, err


def _bounded(name, gpu, f32, f64, factor=4.0):
    """|gpu - f64| <= factor * |f32 - f64| (relative L2): prints both figures before it asserts"""
    e_gpu, e_f32 = rel_err(gpu.cpu(), f64), rel_err(f32, f64)
    print(f"    {name:<18} gpu {e_gpu:.3e}   fp32-on-cpu {e_f32:.3e}   ratio {e_gpu / max(e_f32, 1e-30):.2f}")
    assert e_gpu <= factor * e_f32, (name, e_gpu, e_f32)


# ------------------------------------------------------------------------------------------------ 1. lattice
def _lattice_case(t_lens, u_lens, V=8, seed=0):
    torch.manual_seed(seed)
    B, T, U1 = len(t_lens), max(t_lens), max(u_lens) + 1
    logits = torch.randn(B, T, U1, V, dtype=torch.float64) * 2
    labels = torch.randint(1, V, (B, max(U1 - 1, 1)))
    lpb, lpl = torch.zeros(B, T, U1), torch.zeros(B, T, U1)
    for b in range(B):
        a, c = R.node_logprobs(logits[b], labels[b].tolist())
        lpb[b], lpl[b] = a.float(), c.float()
    ref = [torch.zeros(B, dtype=torch.float64)] + [torch.zeros(B, T, U1, dtype=torch.float64) for _ in range(3)]
    for b in range(B):
        Tb, Ub = t_lens[b], u_lens[b]
        nll, occ, pb, pl = R.lattice_coefficients(lpb[b].double(), lpl[b].double(), Tb, Ub)
        ref[0][b] = nll
        ref[1][b, :Tb, : Ub + 1], ref[2][b, :Tb, : Ub + 1], ref[3][b, :Tb, : Ub + 1] = occ, pb, pl
    return lpb.cuda(), lpl.cuda(), torch.tensor(t_lens).cuda(), torch.tensor(u_lens).cuda(), ref


@pytest.mark.parametrize("t_lens,u_lens", [([1], [0]), ([1], [3]), ([5], [0]), ([1, 7, 37], [0, 12, 5]), ([3], [64]), ([3, 2], [129, 70])],
                         ids=["T1U0", "T1U3", "T5U0", "ragged", "U1=65", "U1=130"])
def test_lattice_vs_float64(t_lens, u_lens):
    """nll at 1e-5 and the three coefficient sets at 1e-4 (the bars of test_ctc_loss_vs_torch), dead nodes exactly 0"""
    from tavsr import ops
    lpb, lpl, tl, ul, ref = _lattice_case(t_lens, u_lens, seed=len(t_lens) + max(u_lens))
    got = ops.rnnt_lattice(lpb, lpl, tl, ul)
    _close(got[0], ref[0], 1e-5)
    for g, r in zip(got[1:], ref[1:]):
        _close(g, r, 1e-4)
        assert float(g.cpu()[r == 0].abs().max() if bool((r == 0).any()) else 0.0) == 0.0


def test_lattice_workspace_route_is_bit_identical_to_the_lds_route():
    from tavsr import ops
    lpb, lpl, tl, ul, ref = _lattice_case([1, 7, 37], [0, 12, 5], seed=7)
    assert ops.rnnt_lattice_lds_ok(37, 13) and not ops.rnnt_lattice_lds_ok(4096, 64)
    lds = ops.rnnt_lattice(lpb, lpl, tl, ul, route="lds")
    ws = ops.rnnt_lattice(lpb, lpl, tl, ul, route="ws")
    for a, b in zip(lds, ws):
        assert torch.equal(a, b)
    _close(ws[0], ref[0], 1e-5)


# ------------------------------------------------------------------------------------------------ 2. joint + loss
JL_T, JL_U, JL_J, JL_DE, JL_DD = 9, 5, 64, 64, 96
JL_TLEN, JL_ULEN = [9, 6, 4], [5, 0, 3]
JL_NAMES = ("enc", "dec", "lin_enc.weight", "lin_enc.bias", "lin_dec.weight", "lin_out.weight", "lin_out.bias")


def _joint_case(V):
    torch.manual_seed(100 + V)
    B = len(JL_TLEN)
    enc, dec = torch.randn(B, JL_T, JL_DE), torch.randn(B, JL_U + 1, JL_DD)
    P = [torch.randn(JL_J, JL_DE) / 8, torch.randn(JL_J) / 4, torch.randn(JL_J, JL_DD) / 10, torch.randn(V, JL_J) / 4, torch.randn(V) / 2]
    target = torch.randint(1, V, (B, JL_U), dtype=torch.int32)
    return enc, dec, P, target


def _joint_reference(enc, dec, P, target, dtype):
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in [enc, dec] + P]
    loss = R.joint_loss(leaves[0], leaves[1], JL_TLEN, JL_ULEN, target, leaves[2:])
    loss.backward()
    return [loss.detach()] + [t.grad for t in leaves]


def _joint_gpu(enc, dec, P, target, chunk):
    from tavsr.functional_rnnt import RNNTLossFn
    leaves = [t.detach().clone().cuda().requires_grad_(True) for t in [enc, dec] + P]
    tl, ul = torch.tensor(JL_TLEN).cuda(), torch.tensor(JL_ULEN).cuda()
    loss = RNNTLossFn.apply(leaves[0], leaves[1], tl, ul, target.cuda(), dict(blank=0, chunk=chunk), *leaves[2:])
    loss.backward()
    torch.cuda.synchronize()
    return [loss.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("V", [41, 65, 5000])
def test_joint_and_loss_in_chunks_vs_float64(V):
    """B = 3 ragged, T = 9, U = 5, J = 64; 162 lattice rows in chunks of 50: three whole chunks and one of 12.
    Measured relative L2 errors against float64, GPU | fp32 on the CPU (bound: 4 x the second; ``pytest -s`` prints them):
      V = 41:   loss 1.1e-8 | 1.1e-8, enc 3.3e-7 | 4.5e-7, dec 2.4e-7 | 4.1e-7, lin_enc.weight 3.3e-7 | 4.3e-7, lin_enc.bias 1.2e-7 | 1.2e-7,
                lin_dec.weight 1.9e-7 | 3.8e-7, lin_out.weight 2.0e-7 | 4.3e-7, lin_out.bias 9.2e-8 | 4.9e-8
      V = 65:   loss 1.4e-8 | 1.4e-8, enc 3.4e-7 | 6.4e-7, dec 2.9e-7 | 4.4e-7, lin_enc.weight 3.1e-7 | 5.6e-7, lin_enc.bias 1.1e-7 | 1.4e-7,
                lin_dec.weight 2.6e-7 | 4.2e-7, lin_out.weight 2.4e-7 | 4.5e-7, lin_out.bias 4.5e-8 | 4.8e-8
      V = 5000: loss 3.4e-8 | 3.4e-8, enc 1.5e-6 | 6.9e-7, dec 8.2e-7 | 4.4e-7, lin_enc.weight 1.5e-6 | 6.6e-7, lin_enc.bias 5.6e-7 | 2.0e-7,
                lin_dec.weight 8.6e-7 | 4.2e-7, lin_out.weight 1.8e-7 | 3.4e-7, lin_out.bias 9.9e-8 | 3.2e-8 (the largest ratio: 3.1)"""
    from tavsr import ops
    enc, dec, P, target = _joint_case(V)
    rows = len(JL_TLEN) * JL_T * (JL_U + 1)
    chunk = 50
    assert rows // chunk >= 3 and rows % chunk != 0 and ops.lib().tavsr_rnnt_ws(3, JL_T, JL_U + 1, JL_J, V, chunk, 1) > 0
    f64 = _joint_reference(enc, dec, P, target, torch.float64)
    f32 = _joint_reference(enc, dec, P, target, torch.float32)
    got = _joint_gpu(enc, dec, P, target, chunk)
    for name, g, a, r in zip(("loss",) + JL_NAMES, got, f32, f64):
        _bounded(name, g, a, r)
    # the same bits from a second run, and padded rows are never read
    again = _joint_gpu(enc, dec, P, target, chunk)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    enc_p, dec_p = enc.clone(), dec.clone()
    for b, (t, u) in enumerate(zip(JL_TLEN, JL_ULEN)):
        enc_p[b, t:] = float("nan")
        dec_p[b, u + 1:] = float("nan")
    poisoned = _joint_gpu(enc_p, dec_p, P, target, chunk)
    assert all(bool(torch.isfinite(t).all()) for t in poisoned)
    assert all(torch.equal(a, b) for a, b in zip(got, poisoned))
    # one chunk for everything is the same computation (other partial sums: close, not equal)
    whole = _joint_gpu(enc, dec, P, target, None)
    assert rel_err(whole[0].cpu(), f64[0]) <= 4 * rel_err(f32[0], f64[0]) and rel_err(whole[6].cpu(), got[6].cpu()) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. LSTM
def _lstm_ref(x, layers, h0, c0, w, a, c_, dtype):
    """torch.nn.LSTM layers chained on the CPU in ``dtype``; loss = <y, w> + <hN, a> + <cN, c_> of the last layer"""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    mods, states, inp = [], [], x
    for li, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
        m = torch.nn.LSTM(w_ih.shape[1], w_hh.shape[1], 1, batch_first=True).to(dtype)
        with torch.no_grad():
            m.weight_ih_l0.copy_(w_ih); m.weight_hh_l0.copy_(w_hh); m.bias_ih_l0.copy_(b_ih); m.bias_hh_l0.copy_(b_hh)
        h, c = (t[li].detach().clone().to(dtype).requires_grad_(True) for t in (h0, c0))
        inp, (hN, cN) = m(inp, (h[None], c[None]))
        mods.append(m)
        states.append((h, c))
    loss = (inp * w.to(dtype)).sum() + (hN[0] * a.to(dtype)).sum() + (cN[0] * c_.to(dtype)).sum()
    loss.backward()
    out = {"y": inp.detach(), "hN": hN[0].detach(), "cN": cN[0].detach(), "dx": x.grad}
    for li, (m, (h, c)) in enumerate(zip(mods, states)):
        out.update({f"dW_ih{li}": m.weight_ih_l0.grad, f"dW_hh{li}": m.weight_hh_l0.grad, f"db_ih{li}": m.bias_ih_l0.grad,
                    f"db_hh{li}": m.bias_hh_l0.grad, f"dh0_{li}": h.grad, f"dc0_{li}": c.grad})
    return out


def _lstm_gpu(x, layers, h0, c0, w, a, c_):
    from tavsr import ops
    dev = [[t.cuda() for t in l] for l in layers]
    inp, saved = x.cuda(), []
    for li, (w_ih, w_hh, b_ih, b_hh) in enumerate(dev):
        y, hN, cN, sv = ops.lstm_fwd(inp, w_ih, w_hh, b_ih, b_hh, h0[li].cuda().contiguous(), c0[li].cuda().contiguous())
        saved.append(sv)
        inp = y
    out = {"y": y, "hN": hN, "cN": cN}
    dy, dhN, dcN = w.cuda().contiguous(), a.cuda().contiguous(), c_.cuda().contiguous()
    for li in reversed(range(len(dev))):
        w_ih, w_hh = dev[li][0], dev[li][1]
        dy, dw_ih, dw_hh, db, dh0, dc0 = ops.lstm_bwd(dy, saved[li], w_ih, w_hh, c0[li].cuda().contiguous(), None, dhN, dcN)
        dhN = dcN = None
        out.update({f"dW_ih{li}": dw_ih, f"dW_hh{li}": dw_hh, f"db_ih{li}": db, f"db_hh{li}": db, f"dh0_{li}": dh0, f"dc0_{li}": dc0})
    out["dx"] = dy
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,L,I,H,n", [(1, 1, 32, 32, 1), (3, 7, 64, 96, 1), (33, 41, 320, 320, 2)])
def test_lstm_forward_and_backward_vs_torch_float64(B, L, I, H, n):
    """forward, dx, dW_ih, dW_hh, both biases, dh0 and dc0 of every layer against torch.nn.LSTM in float64; 33 rows do not
    divide the rows-per-workgroup plan.  Measured relative L2 errors against float64, GPU | fp32 on the CPU (bound: 4 x the
    second), at (33, 41, 320, 320) x 2 layers: y 2.8e-7 | 2.9e-7, hN 3.1e-7 | 3.1e-7, cN 3.1e-7 | 3.1e-7, dx 4.4e-7 | 4.5e-7,
    dW_ih 4.5e-7 | 4.7e-7, dW_hh 5.0e-7 | 5.0e-7, biases 2.8e-7 | 7.4e-7, dh0 5.0e-7 | 4.8e-7, dc0 2.9e-7 | 3.1e-7 (layer 0);
    the largest ratio over the three shapes is 1.13 (hN at (3, 7, 64, 96))."""
    from tavsr import ops
    assert 33 % ops.lstm_rows_per_wg() != 0
    torch.manual_seed(B * L + H)
    k = 1.0 / H ** 0.5
    layers = [tuple((torch.rand(s) * 2 - 1) * k for s in ((4 * H, I if li == 0 else H), (4 * H, H), (4 * H,), (4 * H,))) for li in range(n)]
    x, h0, c0 = torch.randn(B, L, I), torch.randn(n, B, H) * 0.5, torch.randn(n, B, H) * 0.5
    w, a, c_ = torch.randn(B, L, H), torch.randn(B, H), torch.randn(B, H)
    f64, f32 = _lstm_ref(x, layers, h0, c0, w, a, c_, torch.float64), _lstm_ref(x, layers, h0, c0, w, a, c_, torch.float32)
    got = _lstm_gpu(x, layers, h0, c0, w, a, c_)
    for name in f64:
        _bounded(name, got[name], f32[name], f64[name])


def test_lstm_padded_steps_keep_the_state():
    from tavsr import ops
    torch.manual_seed(4)
    B, L, I, H = 3, 7, 64, 96
    lens = [7, 3, 1]
    m = torch.nn.LSTM(I, H, 1, batch_first=True).double()
    x = torch.randn(B, L, I)
    P = [p.detach().float().cuda() for p in (m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0)]
    y, hN, cN, sv = ops.lstm_fwd(x.cuda(), *P, lens=torch.tensor(lens).cuda())
    dy = torch.randn(B, L, H)
    dx, dw_ih, dw_hh, db, _, _ = ops.lstm_bwd(dy.cuda(), sv, P[0], P[1], lens=torch.tensor(lens).cuda())
    xr = x.double().requires_grad_(True)
    loss = 0.0
    for b, n in enumerate(lens):
        yr, (hr, cr) = m(xr[b: b + 1, :n])
        loss = loss + (yr * dy[b: b + 1, :n].double()).sum()
        _close(y[b, :n], yr[0], 1e-5)
        _close(hN[b], hr[0, 0], 1e-5)
        _close(cN[b], cr[0, 0], 1e-5)
        assert float(y[b, n:].abs().max() if n < L else 0.0) == 0.0
    loss.backward()
    _close(dx, xr.grad, 1e-4)
    _close(dw_hh, m.weight_hh_l0.grad, 1e-4)
    _close(db, m.bias_ih_l0.grad, 1e-4)
    assert float(dx[1, 3:].abs().max()) == 0.0 and float(dx[2, 1:].abs().max()) == 0.0


def test_lstm_step_with_commit_mask_is_bit_equal_to_the_step_of_lstm_fwd():
    from tavsr import ops
    torch.manual_seed(8)
    B, L, I, H = 5, 3, 64, 96
    k = 1.0 / H ** 0.5
    w_ih, w_hh, b_ih, b_hh = (((torch.rand(s) * 2 - 1) * k).cuda() for s in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)))
    x, h0, c0 = torch.randn(B, L, I).cuda(), torch.randn(B, H).cuda(), torch.randn(B, H).cuda()
    y, hN, cN, (x2, hprev, c_all, gates) = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    xg = ops.linear(x2, w_ih).view(B, L, 4 * H)                    # the GEMM lstm_fwd runs: the same launch, the same bits
    wt = ops.lstm_wt(w_hh)
    h, c = h0.clone(), c0.clone()
    for t in range(L):
        ops.lstm_step(xg[:, t], wt, b_ih, b_hh, h, c)
        assert torch.equal(h, y[:, t]) and torch.equal(c, c_all[:, t]), t
    assert torch.equal(h, hN) and torch.equal(c, cN)
    # a commit mask: rows 1 and 3 keep their state, the others take step 0
    commit = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8).cuda()
    h, c = h0.clone(), c0.clone()
    ops.lstm_step(xg[:, 0], wt, b_ih, b_hh, h, c, commit)
    keep = commit.bool()
    assert torch.equal(h[keep], y[:, 0][keep]) and torch.equal(c[keep], c_all[:, 0][keep])
    assert torch.equal(h[~keep], h0[~keep]) and torch.equal(c[~keep], c0[~keep])


def test_decoder_dropout_masks_and_one_token_steps():
    """train-mode dropout (embedding and layer outputs, Philox masks regenerated in the backward) and espnet's one-token calls"""
    from tavsr import ops
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    from tavsr.inference.transducer import Hypothesis
    torch.manual_seed(3)
    dec = TransducerDecoder(41, num_layers=2, hidden_size=96, dropout=0.5, dropout_embed=0.25).cuda()
    labels = torch.randint(1, 41, (4, 9)).cuda()
    labels[:, 0] = 0
    ev = dec.eval()(labels)
    ops.manual_seed(11)
    ops.rng_step_begin(labels.device)
    out = dec.train()(labels)
    zeros = float((out == 0).float().mean())
    assert 0.4 < zeros < 0.6 and bool(torch.isfinite(out).all()) and not torch.equal(out, ev)
    out.backward(torch.ones_like(out))
    grads = [p.grad for p in dec.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert float(dec.embed.weight.grad[0].abs().max()) == 0.0 and float(dec.embed.weight.grad.abs().max()) > 0.0
    # the same seed and step draw the same masks: the forward is reproducible bit for bit
    ops.manual_seed(11)
    ops.rng_step_begin(labels.device)
    assert torch.equal(dec(labels), out)
    # score / batch_score: one token from a given state = the teacher-forced pass up to that token
    dec.eval()
    hyp = Hypothesis(score=0.0, yseq=[0], dec_state=dec.init_state(1))
    cache = {}
    d0, st, lab = dec.score(hyp, cache)
    assert rel_err(d0.cpu(), ev[0, 0].cpu()) < 1e-6 and int(lab) == 0 and "0" in cache
    hyp2 = Hypothesis(score=0.0, yseq=[0, int(labels[0, 1])], dec_state=st)
    d1, st2, _ = dec.batch_score([hyp2, hyp2])
    assert rel_err(d1[1].cpu(), ev[0, 1].cpu()) < 1e-6 and st2[0].shape == (2, 2, 96)
    assert dec.select_state(st2, 1)[1].shape == (2, 1, 96)


# ------------------------------------------------------------------------------------------------ 4. model
def _model(seed=21, **kw):
    from tavsr.tasks.asr import ASRTask
    torch.manual_seed(seed)
    return ASRTask.build_model(argparse.Namespace(**rnnt_conf(**kw)))


def _batch(seed=22):
    from oracle.model import synth
    speech, slens = synth((3, 64, 80), seed=seed), torch.tensor([64, 50, 41])
    text, tlens = synth((3, 6), seed=seed + 1, kind="int", lo=1, hi=40), torch.tensor([6, 3, 1])
    text[1, 3:] = -1
    text[2, 1:] = -1
    return [speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda()]


def test_transducer_model_loss_and_every_gradient_vs_float64_on_its_encoder_output():
    """1-block audio-only model, two LSTM layers, ctc_weight 0.3.  The restatement takes the model's encoder output to the
    CPU in float64 and runs decoder, joint, RNN-T loss and the CTC loss there; its gradient of the encoder output goes back
    through the encoder for the encoder's parameters.  Bars: the model-level ones of test_gpu_parity.py (1e-4 loss, 1e-3 gradients)."""
    model = _model(layers=2, hidden=96).cuda().train()
    batch = _batch()
    params = dict(model.named_parameters())
    loss, stats, weight = model(*batch)
    loss.backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    assert set(got) == set(params), sorted(set(params) - set(got))
    assert stats["cer_transducer"] is None and stats["wer_transducer"] is None and int(weight) == 3
    for p in params.values():
        p.grad = None
    enc_out, enc_lens = model.encode(batch[0], batch[1])
    e64 = enc_out.detach().double().cpu().requires_grad_(True)
    text, tlens = batch[2].cpu(), batch[3].cpu()
    dsd, emb, lay = R.decoder_params(model.decoder)
    jsd, P = R.joint_params(model.joint_network)
    labels = torch.zeros(3, 7, dtype=torch.int64)
    for b in range(3):
        labels[b, 1: 1 + int(tlens[b])] = text[b, : int(tlens[b])]
    l_t = R.joint_loss(e64, R.lstm_stack(emb, lay, labels), enc_lens.cpu(), tlens, text, P)
    w_c, b_c = (t.detach().double().cpu().requires_grad_(True) for t in (model.ctc.ctc_lo.weight, model.ctc.ctc_lo.bias))
    lp = torch.nn.functional.linear(e64, w_c, b_c).log_softmax(2).transpose(0, 1)
    flat = torch.cat([text[b, : int(tlens[b])] for b in range(3)])
    l_c = torch.nn.functional.ctc_loss(lp, flat, enc_lens.cpu(), tlens, blank=0, reduction="sum", zero_infinity=True) / 3
    ref = l_t + 0.3 * l_c
    ref.backward()
    print(f"    loss {float(loss):.6f} ref {float(ref):.6f}  transducer {float(stats['loss_transducer']):.6f} ref {float(l_t):.6f}")
    assert rel_err(loss.detach().cpu(), ref.detach()) < 1e-4
    assert rel_err(stats["loss_transducer"].cpu(), l_t.detach()) < 1e-4 and rel_err(stats["loss_ctc"].cpu(), l_c.detach()) < 1e-4
    enc_out.backward(e64.grad.float().cuda())
    torch.cuda.synchronize()
    want = {n: p.grad for n, p in params.items() if p.grad is not None}                    # the encoder's parameters
    want.update({f"decoder.{k}": v.grad for k, v in dsd.items()})
    want.update({f"joint_network.{k}": v.grad for k, v in jsd.items()})
    want.update({"ctc.ctc_lo.weight": w_c.grad, "ctc.ctc_lo.bias": b_c.grad})
    assert set(want) == set(got)
    bad = [(n, rel_err(got[n].cpu(), want[n].cpu())) for n in sorted(got) if not grad_ok(got[n].cpu(), want[n].cpu(), 1e-3)]
    assert not bad, bad
    assert float(got["decoder.embed.weight"][0].abs().max()) == 0.0        # the padding row gets no gradient


@pytest.fixture
def _streams_restored():
    from tavsr import _lib
    keep = _lib.SINGLE_STREAM
    yield
    _lib.SINGLE_STREAM = keep


def test_captured_training_step_and_single_stream_are_bit_equal_to_eager(_streams_restored):
    from tavsr import _lib
    model = _model(layers=1, hidden=96).cuda().train()
    speech, slens, text, tlens = _batch()
    batch = [speech[:, :64].contiguous(), torch.full((3,), 64).cuda(), text[:, :3].contiguous().clamp_min(1), torch.full((3,), 3).cuda()]
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        loss = model(*batch)[0]
        loss.backward()
        return loss

    eager_loss = step().detach().clone()
    eager = [p.grad.detach().clone() for p in params]
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
        static_loss = model(*batch)[0]
        static_loss.backward()
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.detach(), eager_loss), replay
        bad = [n for (n, p), g in zip(model.named_parameters(), eager) if not torch.equal(p.grad, g)]
        assert not bad, (replay, bad[:8])
    del graph
    _lib.SINGLE_STREAM = True
    assert torch.equal(step().detach(), eager_loss)


# ------------------------------------------------------------------------------------------------ 5. greedy search
# seed 12: the float64 restatement decodes [10, 2, 1, 19], [29] and [] with smallest top-2 gaps 0.092, 0.250 and 0.673
GREEDY_SEED, GREEDY_T = 12, [12, 1, 5]


def _greedy_setup():
    """decoder + joint network and a ragged batch of encoder outputs: utterance 1 has T = 1, utterance 2 decodes to the empty
    hypothesis (its frames are small, so the blank bias wins).  The seed is one for which the float64 restatement alone has a
    top-2 gap above 1e-4 at every decision of every utterance."""
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    torch.manual_seed(GREEDY_SEED)
    dec, jn = TransducerDecoder(41, hidden_size=96, num_layers=2), JointNetwork(41, 64, 96, joint_space_size=64)
    with torch.no_grad():
        jn.lin_out.bias[0] += 1.0
    T = max(GREEDY_T)
    enc = torch.randn(3, T, 64) * 3.0
    enc[2] *= 0.01
    return dec, jn, enc, torch.tensor(GREEDY_T)


def _greedy_reference(dec, jn, enc, lens):
    _, emb, lay = R.decoder_params(dec)
    _, P = R.joint_params(jn)
    return [R.greedy_search(enc[b, : int(lens[b])].double(), emb, lay, P) for b in range(enc.shape[0])]


def test_greedy_search_batch_vs_cpu_restatement():
    from tavsr.inference.transducer import BeamSearchTransducer
    dec, jn, enc, lens = _greedy_setup()
    ref = _greedy_reference(dec, jn, enc, lens)
    bound = [gap > 1e-4 for _, _, gap in ref]
    assert sum(bound) / len(bound) == 1.0, [g for _, _, g in ref]
    assert ref[2][0] == [] and len(ref[0][0]) > 0 and int(lens[1]) == 1
    dec, jn = dec.cuda().eval(), jn.cuda().eval()
    search = BeamSearchTransducer(dec, jn, beam_size=1)
    enc_p = enc.clone()
    for b in range(3):
        enc_p[b, int(lens[b]):] = float("nan")              # frames past an utterance are never a decision
    for use_graph in (True, False):
        search.use_graph = use_graph
        out = search.decode(enc_p.cuda(), lens.cuda())
        for b, ((ys, score),) in enumerate(out):
            assert ys == [0] + ref[b][0], (use_graph, b, ys, ref[b][0])
            assert abs(score - ref[b][1]) < 1e-4 * max(1.0, abs(ref[b][1])), (b, score, ref[b][1])
    one = search(enc[0, : int(lens[0])].cuda())              # espnet's one-utterance call
    assert one[0].yseq == [0] + ref[0][0]


def test_speech2text_returns_the_search_ids_of_a_transducer_model():
    from tavsr.inference import Speech2Text
    model = _model(layers=1, hidden=96).cuda().eval()
    with torch.no_grad():
        model.joint_network.lin_out.bias[0] -= 0.5
    speech, slens, _, _ = _batch()
    s2t = Speech2Text(model, beam_size=1)
    assert s2t.beam_search_transducer is not None
    results = s2t(speech, slens)
    with torch.no_grad():
        enc, olens = model.encode(speech, slens)
    direct = s2t.beam_search_transducer.decode(enc, olens)
    ref = _greedy_reference(model.decoder, model.joint_network, enc.cpu(), olens.cpu())
    assert len(results) == 3
    for b, res in enumerate(results):
        text, tokens, ids, (ys, score) = res[0]
        assert ys == direct[b][0][0] and ids == [t for t in ys[1:] if t != 0] and tokens == [TOKENS_EN[t] for t in ids]
        assert text == "".join(tokens).replace("<space>", " ")
        if ref[b][2] > 1e-4:
            assert ids == ref[b][0], (b, ids, ref[b][0])


# ------------------------------------------------------------------------------------------------ 6. symbols
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes
    from tavsr import _lib
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    declared = set(re.findall(r"\b(tavsr_(?:lstm|rnnt)_[a-z0-9_]+)\s*\(", hdr))
    want = {"tavsr_lstm_fwd", "tavsr_lstm_bwd", "tavsr_lstm_step", "tavsr_lstm_wt", "tavsr_lstm_rows_per_wg", "tavsr_rnnt_ws",
            "tavsr_rnnt_joint_rows", "tavsr_rnnt_lattice", "tavsr_rnnt_lattice_ws", "tavsr_rnnt_lattice_lds_ok", "tavsr_rnnt_joint_grad",
            "tavsr_rnnt_mask_rows", "tavsr_rnnt_frame_z", "tavsr_rnnt_greedy_pick"}
    assert want <= declared
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in sorted(declared):
        assert hasattr(raw, n), n
        assert n in _lib.PROTOTYPES and getattr(_lib.lib(), n).argtypes == _lib.PROTOTYPES[n][1], n
