"""GPU: Mask-CTC on the HIP path (``model: maskctc`` / ``decoder: mlm``) - the non-causal decoder self-attention, the MLM
decoder and the two models' training step against the reference's fixtures, the two decoding kernels
(``tavsr_maskctc_init`` / ``tavsr_maskctc_step``) against the CPU restatement ``tests/maskctc_ref.py``, and the decoding
loop end to end: against ``maskctc_decode.npz``, batched, at model scale, hoisted / captured / single-stream.

Integer results are compared exactly.  Where the product's ids are compared with ids computed on the CPU, an utterance may
be left out only if one of its decision margins is at or below the bar (1e-4 in logit units - the bar of the greedy-id tests
in test_gpu_parity.py -, 1e-5 for the distance of a token probability to the threshold); fixtures and seeds were chosen so
that none is, and the tests assert that the left-out set is empty."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

import maskctc_ref as R
from helpers import TOKENS_EN, avsr_conf, golden, grad_ok, max_rel, rel_err, relu_gated_tol
from oracle.model import compact, fill_parameters_, synth

pytestmark = pytest.mark.gpu

H, DK = 4, 64
D = H * DK


def _model(conf, seed, task="asr"):
    from tavsr.tasks.asr import ASRTask
    from tavsr.tasks.avsr import AVSRTask
    conf = copy.deepcopy(conf)
    conf["token_list"] = list(TOKENS_EN)
    m = (AVSRTask if task == "avsr" else ASRTask).build_model(argparse.Namespace(**conf))
    fill_parameters_(m, seed=seed)
    return m.cuda()


def _avsr_small():
    return avsr_conf(R.AVSR_MASKCTC_YAML, num_blocks=2, dec_blocks=1)


# ------------------------------------------------------------------------------------------------ 5. attention
@pytest.mark.parametrize("route", ["fused", "core"])
@pytest.mark.parametrize("B,T,lens", [(3, 41, [41, 30, 5]), (2, 150, [150, 131]), (2, 300, [300, 257])])
def test_non_causal_key_padded_self_attention_matches_fp64(route, B, T, lens):
    """what ``causal=False`` selects for the MLM decoder's self-attention: T1 == T2, no positions, ragged key lengths, one to
    three key blocks - forward and every gradient on both attention routes, at the tolerances test_gpu_attn.py uses for its
    causal case (2e-5 / 5e-5 of the largest reference value)."""
    from tavsr import functional as F_
    from test_gpu_attn import _inputs, _ref
    q, k, v, _, _, _ = _inputs(B, T, T, False, seed=2 * T + 1)
    klens = torch.tensor(lens, device="cuda")
    q4, k4, v4 = (t.double().view(B, T, H, DK).detach().requires_grad_(True) for t in (q, k, v))
    ref, _ = _ref(q4, q4, k4, v4, None, klens, False)
    dctx = torch.randn(B * T, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    ref.backward(dctx.double().view(B, T, H, DK))
    dq, dk_, dv_ = (torch.full((B * T, D), float("nan"), device="cuda") for _ in range(3))
    if route == "fused":
        ctx, saved = F_._AttnFused.fwd(q, 0, k, 0, v, 0, B, T, T, H, DK, klens, False)
        F_._AttnFused.bwd(dctx, ctx, saved, q, 0, k, 0, v, 0, dq, 0, dk_, 0, dv_, 0, B, T, T, H, DK, klens, False)
    else:
        ctx, attn, tok = F_._SelfAttnCore.fwd(q, D, 0, k, D, 0, v, D, 0, B, T, T, H, DK, klens, False)
        F_._SelfAttnCore.bwd(dctx, attn, q, D, 0, k, D, 0, v, D, 0, dq, D, 0, dk_, D, 0, dv_, D, 0, B, T, T, H, DK, tok=tok)
    assert bool(torch.isfinite(ctx).all())
    err = (ctx.double().view(B, T, H, DK) - ref).abs().max() / ref.abs().max()
    assert err < 2e-5, float(err)
    for a, b, name in ((dq, q4.grad, "dq"), (dk_, k4.grad, "dk"), (dv_, v4.grad, "dv")):
        b = b.reshape(a.shape)
        assert bool(torch.isfinite(a).all()), name
        e = (a.double() - b).abs().max() / b.abs().max()
        assert e < 5e-5, (name, float(e))


# ------------------------------------------------------------------------------------------------ 6. decoder and models
def test_mlm_decoder_forward_backward_matches_fp64_restatement():
    from tavsr.decoder.mlm_decoder import MLMDecoder
    kw = dict(num_blocks=2, dropout_rate=0.0, positional_dropout_rate=0.0, self_attention_dropout_rate=0.0,
              src_attention_dropout_rate=0.0)
    ref = R.MLMDecoderRef(41, 256, **kw)
    fill_parameters_(ref, seed=61)
    dec = MLMDecoder(41, 256, **kw)
    dec.load_state_dict(ref.state_dict())
    assert sorted(dec.state_dict().keys()) == sorted(ref.state_dict().keys())
    ref, dec = ref.double().train(), dec.cuda().train()
    B, T, L = 3, 57, 19
    mem, hlens = synth((B, T, 256), seed=62), torch.tensor([57, 40, 31])
    ys, ylens = synth((B, L), seed=63, kind="int", lo=1, hi=42), torch.tensor([19, 11, 4])
    w = synth((B, L, 42), seed=64)
    valid = (torch.arange(L)[None, :] < ylens[:, None])[:, :, None]
    mr = mem.double().requires_grad_(True)
    lo, _ = ref(mr, hlens, ys, ylens)
    (lo * w.double() * valid).sum().backward()
    mg = mem.cuda().requires_grad_(True)
    lg, olens = dec(mg, hlens.cuda(), ys.cuda(), ylens.cuda())
    assert lg.shape == (B, L, 42) and olens.tolist() == ylens.tolist()
    (lg * (w * valid).cuda()).sum().backward()
    for b, n in enumerate(ylens.tolist()):          # rows l >= ys_in_lens[b] are padding: not part of the contract
        assert max_rel(lg[b, :n].cpu(), lo[b, :n]) < 1e-4, b
    assert grad_ok(mg.grad.cpu(), mr.grad, 1e-3)
    po = dict(ref.named_parameters())
    for n, p in dec.named_parameters():
        assert grad_ok(p.grad.cpu(), po[n].grad, 1e-3), n


def _train_vs_fixture(model, g, batch, tol):
    text, tlens = (torch.from_numpy(g[k]).cuda() for k in ("text", "tlens"))
    ys_in, ys_out = (torch.from_numpy(g[k]).cuda() for k in ("ys_in", "ys_out"))
    model.train()
    np.random.seed(int(g["np_seed"]))               # the model's own draw (mask_uniform on the host) ...
    loss, stats, weight = model(*[t.clone() for t in batch], text.clone(), tlens)
    loss.backward()
    assert [str(k) for k in g["stats_keys"]] == list(stats.keys()) and int(weight) == int(g["B"])
    for got, key in ((loss, "loss_train"), (stats["loss_ctc"], "loss_ctc"), (stats["loss_mlm"], "loss_mlm")):
        print(key, float(got.detach()), float(g[key].reshape(-1)[0]))
        assert rel_err(got.detach().cpu(), g[key]) < 1e-4, key
    assert abs(float(stats["acc_mlm"]) - float(g["acc_mlm"].reshape(-1)[0])) < 1e-6
    params = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("g_"):
            assert grad_ok(compact(params[k[2:]].grad.cpu()), g[k], relu_gated_tol(k[2:], tol)), k
    for n, v in zip(g["gnorm_keys"], g["gnorm_vals"]):
        got = float(params[str(n)].grad.norm())
        assert abs(got - v) <= relu_gated_tol(str(n), tol) * max(v, 1e-6) + 1e-6, (n, got, v)
    grads = [p.grad.clone() for p in model.parameters()]
    model.eval()                                    # (after ONE training step, as recorded: the lip front-end's BatchNorm statistics moved once)
    with torch.no_grad():
        enc, olens = model.encode(*[t.clone() for t in batch])
        logits, _ = model.decoder(enc, olens, ys_in, tlens)
    assert np.array_equal(olens.cpu().numpy(), g["olens"])
    for b, n in enumerate(tlens.tolist()):
        assert max_rel(logits[b, :n].cpu(), g["dec_logits"][b, :n]) < 1e-4, b
    model.train()
    for p in model.parameters():
        p.grad = None
    loss2 = model(*[t.clone() for t in batch], text.clone(), tlens, ys_in_pad=ys_in, ys_out_pad=ys_out)[0]      # ... and given masks
    loss2.backward()
    assert torch.equal(loss2, loss) and all(torch.equal(a, p.grad) for a, p in zip(grads, model.parameters()))


def test_maskctc_asr_model_vs_reference_golden():
    g = golden("maskctc_asr_3L")
    model = _model(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), 41)
    assert sorted(model.state_dict().keys()) == list(g["keys"])
    speech = synth((int(g["B"]), int(g["Tin"]), 80), seed=42).cuda()
    _train_vs_fixture(model, g, (speech, torch.from_numpy(g["slens"]).cuda()), 1e-3)      # tolerance of test_asr_model_vs_reference_golden


def test_maskctc_avsr_model_vs_reference_golden():
    g = golden("maskctc_avsr_2L")
    model = _model(_avsr_small(), 101, task="avsr")
    assert sorted(model.state_dict().keys()) == list(g["keys"])
    B, Ta, Tv = int(g["B"]), int(g["Ta"]), int(g["Tv"])
    batch = (synth((B, Ta, 80), seed=102).cuda(), torch.from_numpy(g["alens"]).cuda(), synth((B, Tv, 88, 88), seed=103).cuda(),
             torch.from_numpy(g["vlens"]).cuda())
    _train_vs_fixture(model, g, batch, 2e-3)                                             # tolerance of test_avsr_model_vs_reference_golden


def _dropout_step_setup():
    model = _model(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2, dropout=0.1), 3).train()
    B = 8
    speech = synth((B, 200, 80), seed=6).cuda()
    slens = torch.tensor([200 - 8 * i for i in range(B)]).cuda()
    text = synth((B, 20), seed=7, kind="int", lo=1, hi=40)
    tlens = torch.tensor([20 - 2 * (i % 5) for i in range(B)])
    tlens[0] = 20
    for i, l in enumerate(tlens):
        text[i, int(l):] = -1
    np.random.seed(5)
    ys_in, ys_out = R.mask_uniform_ref(text, model.mask_token, model.eos, -1)
    return model, (speech, slens, text.cuda(), tlens.cuda()), dict(ys_in_pad=ys_in.cuda(), ys_out_pad=ys_out.cuda())


def _step(model, batch, masks):
    from tavsr import ops
    for p in model.parameters():
        p.grad = None
    ops.manual_seed(11)
    loss = model(*batch, **masks)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), [p.grad.clone() for p in model.parameters()]


def test_maskctc_training_step_with_dropout_is_bitwise_reproducible():
    """the recipe's dropout rates on: the MLM decoder draws its masks from the same Philox mapping as the attention decoder, so two
    runs from the same generator state are bit-identical (style of test_full_size_training_step_is_bitwise_reproducible)"""
    model, batch, masks = _dropout_step_setup()
    a, b = _step(model, batch, masks), _step(model, batch, masks)
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0])
    for (n, _), x, y in zip(model.named_parameters(), a[1], b[1]):
        assert torch.equal(x, y), n
    c = _step(model.eval(), batch, masks)           # and the masks do something
    assert not torch.equal(a[0], c[0])


def test_maskctc_training_step_captured_is_bit_equal_to_eager():
    from tavsr import ops
    model, batch, masks = _dropout_step_setup()
    ref = _step(model, batch, masks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(model, batch, masks)
    torch.cuda.current_stream().wait_stream(side)
    params = list(model.parameters())
    for p in params:
        p.grad = None
    ops.manual_seed(11)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = model(*batch, **masks)[0]
        loss.backward()
    for rep in range(2):
        ops.manual_seed(11)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), ref[0]), rep
        for (n, p), want in zip(model.named_parameters(), ref[1]):
            assert torch.equal(p.grad, want), (rep, n)


# ------------------------------------------------------------------------------------------------ 7. the two kernels
def _init_ref(logits, hlens, mask_token, thr, K):
    out = []
    for b in range(logits.shape[0]):
        _, y_hat, prob = R.ctc_tokens(logits[b, : int(hlens[b])]) if int(hlens[b]) > 0 else (None, torch.zeros(0, dtype=torch.int64),
                                                                                           torch.zeros(0))
        masked = prob.double() < thr
        out.append((y_hat, prob, torch.where(masked, torch.full_like(y_hat, mask_token), y_hat), R.plan_of(int(masked.sum()), K)))
    return out


def _check_init(logits, hlens, thr, K, mask_token=41):
    from tavsr import ops
    B, T, V = logits.shape
    y_in, y_hat, prob, y_len, plan = ops.maskctc_init(logits.cuda(), hlens.cuda(), 0, mask_token, thr, K)
    y_in, y_hat, prob, y_len, plan = (t.cpu() for t in (y_in, y_hat, prob, y_len, plan))
    assert y_in.shape == (B, max(T, 1))
    for b, (rh, rp, ri, rplan) in enumerate(_init_ref(logits, hlens, mask_token, thr, K)):
        n = len(rh)
        assert int(y_len[b]) == n, (b, int(y_len[b]), n)
        assert torch.equal(y_hat[b, :n], rh) and torch.equal(y_in[b, :n], ri), b
        assert plan[b].tolist() == list(rplan), (b, plan[b].tolist(), rplan)
        assert np.allclose(prob[b, :n].numpy(), rp.numpy(), rtol=1e-6, atol=0), b          # fp32 rounding of a softmax value
        assert int(y_in[b, n:].abs().max() if n < y_in.shape[1] else 0) == 0                # padding is a valid id, never garbage
        assert int(y_hat[b, n:].abs().max() if n < y_in.shape[1] else 0) == 0 and float(prob[b, n:].abs().sum()) == 0.0
    return y_in, y_len, plan


def _median_thr(logits, hlens):
    p = np.sort(np.concatenate([r[1].numpy() for r in _init_ref(logits, hlens, 41, 0.0, 10)]).astype(np.float64))
    band = p[int(0.4 * len(p)): max(int(0.6 * len(p)), int(0.4 * len(p)) + 2)]
    i = int(np.argmax(np.diff(band)))
    assert band[i + 1] - band[i] > 1e-5           # far from fp32 rounding of either side's probability
    return float((band[i] + band[i + 1]) / 2)


@pytest.mark.parametrize("T", [1, 99, 499])
def test_maskctc_init_kernel_matches_restatement(T):
    B, V = 6, 41
    logits = 3.0 * synth((B, T, V), seed=70 + T)
    logits = logits[:, torch.repeat_interleave(torch.arange(T), synth((T,), seed=71, kind="int", lo=1, hi=5))[:T]].contiguous()
    hlens = torch.tensor([T, max(1, (3 * T) // 4), max(1, T // 2), 1, T, 0])
    logits[4, :, 0] += 30.0                                     # an utterance that is all blank: y_len = 0
    if T > 8:
        logits[0, 5, 7] = logits[0, 5, 3] = 40.0                # an exact tie: the lower index wins, as torch.argmax
        logits[1, 2, 40] = logits[1, 2, 0] = 40.0               # ... also against blank
        logits[2, 3, 9] = float("nan")                          # NaN is the maximum (ctc_greedy's rule)
        assert int(logits[0, 5].argmax()) == 3 and int(logits[1, 2].argmax()) == 0 and int(logits[2, 3].argmax()) == 9
    thr = _median_thr(logits[:4], hlens[:4]) if T > 8 else 0.5
    for thr_, K in ((thr, 10), (thr, 0), (thr, 1), (thr, 100000), (0.0, 10), (2.0, 10)):      # (0: nothing masked; 2: everything)
        y_in, y_len, plan = _check_init(logits, hlens, thr_, K)
        if thr_ == 0.0:
            rows = [0, 1, 3, 4, 5]              # (utterance 2's NaN frame is a token of probability -1 on both sides: below any threshold)
            assert int(plan[rows, 0].sum()) == 0 and int((y_in[rows] == 41).sum()) == 0
        if thr_ == 2.0:
            assert plan[:, 0].tolist() == y_len.tolist()
    assert int(y_len[4]) == 0 and int(y_len[5]) == 0


def _check_step(logits, y_in, y_len, plans, its, mask_token):
    from tavsr import ops
    plan = torch.tensor(plans, dtype=torch.int32)
    for it in its:
        got = ops.maskctc_step(logits.cuda(), y_in.clone().cuda(), y_len.cuda(), plan.cuda(), it, mask_token).cpu()
        for b in range(logits.shape[0]):
            n = int(y_len[b])
            want, _, _ = R.fill_pass(logits[b, :n], y_in[b, :n], mask_token, it, plans[b][1],
                                     min(plans[b][2], int((y_in[b, :n] == mask_token).sum())))
            assert torch.equal(got[b, :n], want), (it, b, got[b, :n].tolist(), want.tolist())
            assert torch.equal(got[b, n:], y_in[b, n:]), (it, b)


def test_maskctc_step_kernel_matches_restatement():
    B, L, V1, mask = 6, 61, 42, 41
    logits = synth((B, L, V1), seed=80)
    y_in = synth((B, L), seed=81, kind="int", lo=1, hi=41)
    y_in[synth((B, L), seed=82, kind="uniform") > 0.0] = mask              # about half masked
    y_len = torch.tensor([61, 40, 17, 61, 0, 5])
    y_in[3] = synth((L,), seed=83, kind="int", lo=1, hi=41)                 # nothing masked
    y_in[5, :5] = mask                                                      # everything masked
    counts = [int((y_in[b, : int(y_len[b])] == mask).sum()) for b in range(B)]
    # every utterance follows its own plan; utterance 1: per_iter larger than what is left (clamped); 3, 4: finished at once
    plans = [list(R.plan_of(counts[0], 10)), [counts[1], 3, 1000], list(R.plan_of(counts[2], 4)), [0, 0, 0], [0, 0, 0],
             list(R.plan_of(5, 10))]
    _check_step(logits, y_in, y_len, plans, range(0, 12), mask)


def test_maskctc_step_kernel_tie_rule_and_mask_token_winning():
    B, L, V1, mask = 2, 9, 42, 41
    logits = synth((B, L, V1), seed=90)
    y_in = torch.full((B, L), mask, dtype=torch.int64)
    y_in[:, 4] = 7
    logits[0, [1, 3, 6], 5] = 8.0                       # three equal maxima, two slots: positions 1 and 3 (the contract: lower first)
    logits[0, 2, mask] = 20.0                           # <mask> wins: takes a slot, stays masked, is a candidate again
    logits[0, 8, 11] = logits[0, 8, 30] = 9.5           # a tie inside a row: the lower column
    logits[1, 0, 2] = float("nan")                      # NaN is the largest (torch.max / torch.topk order)
    y_len = torch.tensor([9, 9])
    plans = [[8, 4, 4], [8, 8, 1]]
    from tavsr import ops
    got = ops.maskctc_step(logits.cuda(), y_in.clone().cuda(), y_len.cuda(), torch.tensor(plans, dtype=torch.int32).cuda(), 0, mask).cpu()
    assert got[0].tolist() == [mask, 5, mask, 5, 7, mask, mask, mask, 11]
    assert got[1].tolist() == [2, mask, mask, mask, 7, mask, mask, mask, mask]
    _check_step(logits[:1], y_in[:1], y_len[:1], plans[:1], range(0, 5), mask)


# ------------------------------------------------------------------------------------------------ 8 / 9. end to end
def _fixture_model():
    return _model(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), 41).eval()


def _margins_fail(mg):
    """the rule of the module docstring on (m_ctc, m_thr, m_fill, m_cand)"""
    return min(mg[0], mg[2], mg[3]) <= 1e-4 or mg[1] <= 1e-5


def test_decode_matches_reference_fixture_utterance_by_utterance():
    from tavsr.models.maskctc_model import MaskCTCInference
    g = golden("maskctc_decode")
    model = _fixture_model()
    left_out = []
    for u in range(int(g["n_utt"])):
        if _margins_fail(g[f"u{u}_margins"]):
            left_out.append(u)
            continue
        T, K, thr = int(g[f"u{u}_T"]), int(g[f"u{u}_K"]), float(g[f"u{u}_thr"])
        enc = R.synth_encoder_output(T, int(g[f"u{u}_seed"])).cuda()
        inf = MaskCTCInference(model, n_iterations=K, threshold_probability=thr)
        y_in, y_hat, prob, y_len, plan = inf.start(enc[None], torch.tensor([T]).cuda())
        n = int(y_len[0])
        assert y_hat[0, :n].cpu().tolist() == g[f"u{u}_y_hat"].tolist() and plan[0].cpu().tolist() == g[f"u{u}_plan"].tolist()
        if n:       # (logits of the product's own CTC-head GEMM, another summation order than the CPU's: the activation bar, not the
            #          1e-6 of the kernel test, where both sides read the same logits)
            assert max_rel(prob[0, :n].cpu(), g[f"u{u}_tok_prob"]) < 1e-4
        trace = []
        (yseq,) = inf.decode(enc[None], torch.tensor([T]).cuda(), trace=trace)
        want = g[f"u{u}_y_in"]
        assert len(trace) == len(want), (u, len(trace), len(want))
        for i, (a, b) in enumerate(zip(trace, want)):
            assert a[0, :n].cpu().tolist() == b.tolist(), (u, i)
        assert yseq == g[f"u{u}_yseq"].tolist(), u
        hyp = inf(enc)                                   # the reference's call: one utterance [T, D] -> Hypothesis
        assert hyp.yseq.cpu().tolist() == yseq and hyp.yseq[0] == hyp.yseq[-1] == model.mask_token
    assert left_out == []


def _padded_batch(g, us):
    Tm = max(int(g[f"u{u}_T"]) for u in us)
    enc = torch.zeros(len(us), Tm, 256)
    for i, u in enumerate(us):
        enc[i, : int(g[f"u{u}_T"])] = R.synth_encoder_output(int(g[f"u{u}_T"]), int(g[f"u{u}_seed"]))
    return enc.cuda(), torch.tensor([int(g[f"u{u}_T"]) for u in us]).cuda()


def test_batched_decode_gives_every_utterance_its_single_run():
    """all fixture utterances padded into one batch, one threshold (utterance 0's) and K = 10 for all: per utterance exactly the
    ids of its own single-utterance run (padding independence; num_iter differs from utterance to utterance), and those of the
    restatement wherever its margins bind."""
    from tavsr.models.maskctc_model import MaskCTCInference
    g = golden("maskctc_decode")
    model = _fixture_model()
    us = list(range(int(g["n_utt"])))
    thr, K = float(g["u0_thr"]), 10
    inf = MaskCTCInference(model, n_iterations=K, threshold_probability=thr)
    enc, lens = _padded_batch(g, us)
    batch = inf.decode(enc, lens)
    ref = R.build_asr_ref(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), TOKENS_EN).eval()
    fill_parameters_(ref, seed=41)
    left_out, iters = [], set()
    for i, u in enumerate(us):
        T = int(lens[i])
        (single,) = inf.decode(enc[i: i + 1, :T].contiguous(), lens[i: i + 1])
        assert batch[i] == single, u
        tr = R.maskctc_infer(ref.ctc.ctc_lo, ref.decoder, enc[i, :T].cpu(), ref.mask_token, K, thr)
        iters.add(tr["plan"][1])
        if not R.margins_ok(tr):
            left_out.append(u)
            continue
        assert batch[i] == tr["yseq"].tolist(), u
    print("num_iter in the batch", sorted(iters))
    assert len(iters) >= 3 and left_out == []


# ------------------------------------------------------------------------------------------------ 10. model scale
# Inputs and threshold of the two model-scale tests were chosen on the CPU, with the restatement alone: per batch slot the first
# input seed whose utterance has every logit margin >= 1e-3 and its threshold distance >= 1e-4 - ten times the bars - at the
# fixed threshold below (about the median token probability of these seeded-weight models: 37-48 of ~75 tokens start masked in the
# audio-only model, 29-58 of 40-80 in the audio-visual one), inside the batch it is tested in (an utterance's encoder output
# depends on the padded length of its batch: the cgMLP's convolution reads the padded frames, as in the reference).  The tests
# recompute the margins from the restatement's trace.
SCALE_THRESHOLD = 0.066
ASR_SCALE_SEEDS = (9004, 10007, 11008, 12001, 13002, 14009, 15003, 16002)
AVSR_SCALE_SEEDS = (9000, 10025, 11000, 12000)


def _scale_check(ref, model, inputs, thr=SCALE_THRESHOLD, K=10):
    from tavsr.models.maskctc_model import MaskCTCInference
    with torch.no_grad():
        enc, olens = ref.encode(*inputs)
        eg, og = model.encode(*[t.cuda() for t in inputs])
    assert olens.tolist() == og.cpu().tolist() and max_rel(eg.cpu(), enc) < 1e-4
    got = MaskCTCInference(model, n_iterations=K, threshold_probability=thr).decode(eg, og)
    left_out, smallest, masked, tokens = [], [math.inf, math.inf], 0, 0
    for b in range(enc.shape[0]):
        tr = R.maskctc_infer(ref.ctc.ctc_lo, ref.decoder, enc[b, : int(olens[b])], ref.mask_token, K, thr)
        smallest = [min(smallest[0], tr["m_ctc"], tr["m_fill"], tr["m_cand"]), min(smallest[1], tr["m_thr"])]
        masked, tokens = masked + tr["plan"][0], tokens + len(tr["y_hat"])
        if not R.margins_ok(tr):
            left_out.append(b)
            continue
        assert got[b] == tr["yseq"].tolist(), b
    print(f"threshold {thr}, {masked} of {tokens} positions masked, smallest logit margin {smallest[0]:.3e}, "
          f"smallest threshold distance {smallest[1]:.3e}")
    assert left_out == [] and masked > 0


def test_model_scale_decode_audio_only_12L_matches_restatement():
    """the 12-layer audio-only model with a 6-layer MLM decoder, batch 8 of 4 s inputs (ragged)"""
    conf = R.asr_maskctc_conf(num_blocks=12, dec_blocks=6)
    ref = R.build_asr_ref(conf, TOKENS_EN).eval()
    fill_parameters_(ref, seed=1234)
    model = _model(conf, 1234).eval()
    inputs = (torch.stack([synth((400, 80), seed=s) for s in ASR_SCALE_SEEDS]), torch.tensor([400 - 12 * i for i in range(8)]))
    _scale_check(ref, model, inputs)


def test_model_scale_decode_tailored_av_2L_matches_restatement():
    """the 2-layer tailored audio-visual model (raw 88 x 88 lip frames in), batch 4 of up to 4 s, ragged in both modalities"""
    conf = _avsr_small()
    ref = R.build_avsr_ref(conf, TOKENS_EN).eval()
    fill_parameters_(ref, seed=101)
    model = _model(conf, 101, task="avsr").eval()
    inputs = (torch.stack([synth((400, 80), seed=s) for s in AVSR_SCALE_SEEDS]), torch.tensor([400, 360, 300, 200]),
              torch.stack([synth((100, 88, 88), seed=s + 50000) for s in AVSR_SCALE_SEEDS]), torch.tensor([100, 90, 75, 50]))
    _scale_check(ref, model, inputs)


# ------------------------------------------------------------------------------------------------ 11. bit-equality
@pytest.fixture
def _streams_restored():
    from tavsr import _lib
    yield
    _lib.SINGLE_STREAM = False


def test_hoisted_captured_and_single_stream_decoding_are_bit_equal(_streams_restored):
    from tavsr import _lib
    from tavsr.models.maskctc_model import MaskCTCInference
    g = golden("maskctc_decode")
    model = _fixture_model()
    us = [1, 2, 3, 6]
    enc, lens = _padded_batch(g, us)
    inf = MaskCTCInference(model, n_iterations=10, threshold_probability=float(g["u1_thr"]))
    # the decoder's logits with and without the hoisted source-attention projections
    y_in, _, _, y_len, plan = inf.start(enc, lens)
    L = int(y_len.max())
    y0 = y_in[:, :L].contiguous()
    kv = model.decoder.prepare_memory(enc, lens)
    with torch.no_grad():
        a, _ = model.decoder(enc, lens, y0, y_len)
        b, _ = model.decoder(enc, lens, y0, y_len, memory_kv=kv)
    assert torch.equal(a, b)
    eager = inf.decode(enc, lens)
    assert inf.decode(enc, lens, hoist=False) == eager
    # the loop of a given (B, L, T) as one captured graph, replayed twice
    n_passes = int(plan[:, 1].max())
    y = y0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inf.passes(enc, lens, y0.clone(), y_len, y_len, plan, n_passes, memory_kv=kv)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inf.passes(enc, lens, y, y_len, y_len, plan, n_passes, memory_kv=kv)
    for rep in range(2):
        y.copy_(y0)
        graph.replay()
        torch.cuda.synchronize()
        ids = y.cpu().tolist()
        assert [[model.mask_token] + ids[i][: int(y_len[i])] + [model.mask_token] for i in range(len(us))] == eager, rep
    _lib.SINGLE_STREAM = True
    assert inf.decode(enc, lens) == eager


# ------------------------------------------------------------------------------------------------ 12. waveform to text
def test_speech2text_maskctc_from_waveform():
    """the cfg-1 WAV path of test_gpu_frontend.py (2 s synthetic waveform, log-mel front end in the model, 6-layer encoder)"""
    from tavsr.inference import Speech2TextMaskCTC
    conf = R.asr_maskctc_conf(num_blocks=6, dec_blocks=1)
    conf["input_size"] = None
    model = _model(conf, 51).eval()
    wav, wlen = (0.1 * synth((1, 32000), seed=52, kind="uniform")).cuda(), torch.tensor([32000]).cuda()
    with torch.no_grad():
        enc, olens = model.encode(wav, wlen)
        p = np.sort(model.ctc.softmax(enc)[0, : int(olens[0])].max(-1).values.cpu().numpy())
    s2t = Speech2TextMaskCTC(model, maskctc_n_iterations=10, maskctc_threshold_probability=float(p[len(p) // 2]))
    first = s2t(wav, wlen)
    again = s2t(wav, wlen)                              # (the second call replays the captured encoder)
    assert len(first) == 1 and len(first[0]) == 1
    text, token, token_int, hyp = first[0][0]
    yseq = hyp.yseq.tolist()
    assert yseq[0] == yseq[-1] == model.mask_token and len(yseq) > 2
    assert token_int == [t for t in yseq[1:-1] if t != 0] and 0 not in token_int and len(token_int) > 0
    assert token == [model.token_list[t] for t in token_int]
    assert isinstance(text, str) and text == "".join(token).replace("<mask>", "_").replace("<space>", " ")
    assert again[0][0][:3] == (text, token, token_int)
    default = Speech2TextMaskCTC(model)(wav, wlen)[0][0]      # the recipe's 0.99: every token starts masked
    assert len(default[3].yseq) == len(yseq)
