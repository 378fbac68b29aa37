"""Beam search with a scorer absent - a model without decoder (CTC prefix beam search, with or without LM), a model without CTC head
(attention beam search) - and the one-launch CTC search (tavsr_ctc_beam_search), against the oracle's restatement of espnet's
BatchBeamSearch built with the reduced scorer dict (espnet drops a scorer that is None or has weight 0: oracle/beam_search.py:274-284).

Oracle model, LM and inputs are those of tests/test_beam_search.py (T = 39 / 30 / 22 encoder frames).  The smallest gap between the
oracle's first and second hypothesis over the cases below is 1.28e-3 absolute (CTC-only, beam 10, utterance 0, score -100.8) - about
ten times the fp32 error of such a score - so the best hypothesis is compared token for token."""
import argparse
import functools

import pytest
import torch

from helpers import TOKENS_EN, asr_conf
from oracle import beam_search as BS
from oracle.model import build_asr_oracle, fill_parameters_, synth

pytestmark = pytest.mark.gpu

LM_KW = dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0)
V = len(TOKENS_EN)


@functools.lru_cache(maxsize=None)
def _oracle():
    m = build_asr_oracle(asr_conf(num_blocks=2, dec_blocks=2), TOKENS_EN).eval()
    fill_parameters_(m, seed=5)
    lm = BS.TransformerLMOracle(V, **LM_KW).eval()
    fill_parameters_(lm, seed=6)
    x = synth((3, 160, 80), seed=7)
    with torch.no_grad():
        enc, olens = m.encode(x, torch.tensor([160, 120, 88]))
    return m, lm, enc, olens


@functools.lru_cache(maxsize=None)
def _product(model_ctc_weight=None, input_size=80):
    """the product model with the oracle's parameters (filled by name); model_conf ctc_weight 1.0: no decoder, 0.0: no CTC head"""
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=2, dec_blocks=2)
    conf["input_size"] = input_size
    if model_ctc_weight is not None:
        conf["model_conf"]["ctc_weight"] = model_ctc_weight
    conf["token_list"] = TOKENS_EN
    pm = ASRTask.build_model(argparse.Namespace(**conf)).eval()
    fill_parameters_(pm, seed=5)
    assert (pm.decoder is None) == (model_ctc_weight == 1.0) and (pm.ctc is None) == (model_ctc_weight == 0.0)
    return pm.cuda()


@functools.lru_cache(maxsize=None)
def _product_lm():
    from tavsr.lm.transformer_lm import TransformerLM
    plm = TransformerLM(V, **LM_KW).eval()
    fill_parameters_(plm, seed=6)
    return plm.cuda()


@functools.lru_cache(maxsize=None)
def _reference(decoder, ctc, beam, lm_w, pen, ratio=0.0):
    """the oracle's search with the reduced scorer dict, one utterance at a time (computed once per case)"""
    m, lm, enc, olens = _oracle()
    ctc_w = 1.0 if not decoder else (0.0 if not ctc else 0.3)
    scorers = dict(decoder=BS.DecoderScorer(m.decoder) if decoder else None, ctc=BS.CTCPrefixScorer(ctc=m.ctc, eos=m.eos) if ctc else None,
                   length_bonus=BS.LengthBonus(V), lm=lm if lm_w else None)
    weights = dict(decoder=1.0 - ctc_w, ctc=ctc_w, lm=lm_w, length_bonus=pen)
    out = []
    with torch.no_grad():
        for u in range(3):
            bs = BS.BatchBeamSearch(scorers, weights, beam, V, m.sos, m.eos, pre_beam_score_key=None if ctc_w == 1.0 else "full")
            assert set(bs.weights) == {k for k, on in (("decoder", decoder), ("ctc", ctc), ("lm", lm_w), ("length_bonus", pen)) if on}
            hyps = bs.forward(enc[u, : int(olens[u])], maxlenratio=ratio)
            out.append([(h.yseq.tolist(), float(h.score)) for h in hyps])
    return out


def _check_against_reference(hip, ref):
    """the assertions of tests/test_beam_search.py:test_hip_beam_search_matches_oracle"""
    for u in range(3):
        assert len(hip[u]) > 0 and len(ref[u]) > 0
        assert hip[u][0][0] == ref[u][0][0], (u, hip[u][0], ref[u][0])
        print(f"utterance {u}: best score {hip[u][0][1]:.6f}, oracle {ref[u][0][1]:.6f}, rel {abs(hip[u][0][1] - ref[u][0][1]) / abs(ref[u][0][1]):.2e}")
        assert abs(hip[u][0][1] - ref[u][0][1]) < 2e-4 * abs(ref[u][0][1])
        top_h = {tuple(h[0]) for h in hip[u][:3]}
        top_r = {tuple(h[0]) for h in ref[u][:3]}
        assert len(top_h & top_r) >= 2, (u, top_h, top_r)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("pen", [0.0, 0.5])
@pytest.mark.parametrize("beam", [5, 10])
def test_ctc_only_search_matches_oracle(monkeypatch, beam, pen, fused):
    """a model without decoder, no LM: CTC prefix beam search over every token - in one launch, and token by token"""
    from tavsr.inference import beam_search as PBS
    monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", fused)
    _, _, enc, olens = _oracle()
    search = PBS.BatchBeamSearch(_product(1.0), None, beam, 1.0, 0.0, pen)
    hip = search.decode(enc.cuda(), olens.cuda())
    assert (search._captured.graph is None) == fused          # the route taken: one launch / a captured step
    _check_against_reference(hip, _reference(False, True, beam, 0.0, pen))


@pytest.mark.parametrize("beam", [5, 10])
def test_ctc_with_lm_search_matches_oracle(beam):
    from tavsr.inference.beam_search import BatchBeamSearch
    _, _, enc, olens = _oracle()
    hip = BatchBeamSearch(_product(1.0), _product_lm(), beam, 1.0, 0.6, 0.5).decode(enc.cuda(), olens.cuda())
    _check_against_reference(hip, _reference(False, True, beam, 0.6, 0.5))


@pytest.mark.parametrize("lm_w", [0.0, 0.6])
@pytest.mark.parametrize("beam", [5, 10])
def test_attention_only_search_matches_oracle(beam, lm_w):
    """a model without CTC head: plain top-K over the full scorers, no pre-beam, nothing of the CTC family launched"""
    from tavsr.inference.beam_search import BatchBeamSearch
    _, _, enc, olens = _oracle()
    search = BatchBeamSearch(_product(0.0), _product_lm() if lm_w else None, beam, 0.0, lm_w, 0.5)
    hip = search.decode(enc.cuda(), olens.cuda())
    assert search._captured.bufs.logp_ctc is None and search._captured.bufs.r_prev is None       # no CTC buffers
    _check_against_reference(hip, _reference(True, False, beam, lm_w, 0.5))


@pytest.mark.parametrize("beside", [True, False])
@pytest.mark.parametrize("lm_w", [0.0, 0.6])
def test_hybrid_model_without_pre_beam_matches_oracle(monkeypatch, lm_w, beside):
    """a hybrid model at ctc_weight 1.0 WITHOUT skip_zero_weight: the decoder still runs (at weight 0) and there is no pre-beam, so the
    CTC launch is handed every token as a candidate list - the form ``BatchBeamSearch._ctc_all_tokens`` keeps apart from the reduced
    step's ``cand=None``; beam 5: the one-launch beam update behind the scorers (CTC_BESIDE_SCORERS), and the launches behind them.
    espnet drops the decoder at weight 0: the oracle's search is the CTC (+ LM) one.  Smallest gap between the oracle's first and
    second hypothesis: 1.44e-3 absolute without LM (utterance 0, score -82.35; 4.1e-3 and 2.6e-2 for the others), 0.126 with the LM -
    the first about ten times the fp32 error of such a score, so the best hypothesis is compared token for token."""
    from tavsr import ops
    from tavsr.inference import beam_search as PBS
    monkeypatch.setattr(PBS, "CTC_BESIDE_SCORERS", beside)
    _, _, enc, olens = _oracle()
    search = PBS.BatchBeamSearch(_product(), _product_lm() if lm_w else None, 5, 1.0, lm_w, 0.5, skip_zero_weight=False)
    assert search.has_dec and search.has_ctc and not search.pre_beam and search.C == V and not search._ctc_all_tokens
    assert ops.beam_select_topk_ok(5, V)
    hip = search.decode(enc.cuda(), olens.cuda())
    assert search._captured.graph is not None
    _check_against_reference(hip, _reference(False, True, 5, lm_w, 0.5))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ratio", [-5, 0.5])
def test_ctc_only_search_with_a_token_budget_matches_oracle(monkeypatch, ratio, fused):
    """maxlenratio != 0: a fixed token budget per utterance, no end detection; the last iteration closes every hypothesis"""
    from tavsr.inference import beam_search as PBS
    monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", fused)
    _, _, enc, olens = _oracle()
    search = PBS.BatchBeamSearch(_product(1.0), None, 5, 1.0, 0.0, 0.5, maxlenratio=ratio)
    hip = search.decode(enc.cuda(), olens.cuda())
    want = [5, 5, 5] if ratio < 0 else [max(1, int(ratio * int(t))) for t in olens]
    assert all(n <= w for n, w in zip(search.n_steps, want)) and max(len(h[0]) for u in hip for h in u) <= max(want) + 2
    _check_against_reference(hip, _reference(False, True, 5, 0.0, 0.5, ratio))


def _synthetic(U, T, seed, scale=3.0):
    """encoder outputs the oracle is too slow for: scaled noise - peaky CTC posteriors at scale 3, nearly uniform ones at 0.02
    (a model before training), where every term of the recursion's sums carries weight and a sum rounded differently shows - ragged lengths"""
    enc = (scale * synth((U, T, 256), seed=seed)).cuda()
    lens = torch.tensor([T - (u * T) // 5 for u in range(U)]).cuda()
    return enc, lens


@pytest.mark.parametrize("U,T,K,scale", [(1, 300, 10, 3.0), (2, 97, 16, 3.0), (3, 64, 20, 3.0), (1, 17, 1, 3.0), (1, 99, 10, 0.02), (2, 64, 20, 0.02)])
def test_one_launch_search_equals_the_stepwise_route(monkeypatch, U, T, K, scale):
    """same hypothesis lists, bit-equal scores, same number of tokens searched - the stepwise route is the one checked against the
    oracle above (beams of up to 16: the one-launch beam update; 20: tavsr_beam_combine_topk)"""
    from tavsr import ops
    from tavsr.inference import beam_search as PBS
    enc, lens = _synthetic(U, T, seed=40 + T, scale=scale)
    assert ops.ctc_beam_search_ok(K, V, T)
    outs, steps = [], []
    for fused in (True, False):
        monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", fused)
        search = PBS.BatchBeamSearch(_product(1.0), None, K, 1.0, 0.0, 0.5)
        outs.append(search.decode(enc, lens))
        steps.append(search.n_steps)
        assert (search._captured.graph is None) == fused
    print(f"U {U} T {T} K {K}: tokens searched {steps[0]}, hypotheses {[len(o) for o in outs[0]]}")
    assert steps[0] == steps[1] and all(1 <= n <= int(l) for n, l in zip(steps[0], lens))
    assert all(len(o) > 0 for o in outs[0])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("U,T,K", [(1, 480, 10), (2, 480, 20)])
def test_one_launch_search_with_a_large_lattice_equals_the_stepwise_route(monkeypatch, U, T, K):
    """more than 64 KB of dynamic LDS (77 KB at beam 10, 156 KB of the 160 KiB at beam 20, T = 480): the launch must raise the function's
    dynamic-LDS limit first.  A budget of 12 tokens keeps the case short; the lattice is T frames long whatever the budget."""
    from tavsr import ops
    from tavsr.inference import beam_search as PBS
    assert ops.ctc_beam_search_ok(K, V, T) and 16 * K * T > 64 * 1024
    enc, lens = _synthetic(U, T, seed=11)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", fused)
        search = PBS.BatchBeamSearch(_product(1.0), None, K, 1.0, 0.0, 0.5, maxlenratio=-12)
        outs.append(search.decode(enc, lens))
        assert (search._captured.graph is None) == fused and search.n_steps == [12] * U
    assert all(len(o) == K for o in outs[0]) and outs[0] == outs[1]


def test_a_shape_the_one_launch_search_refuses_takes_the_stepwise_route(monkeypatch):
    from tavsr import ops
    from tavsr.inference import beam_search as PBS
    K = 20
    T = next(t for t in range(64, 4096) if not ops.ctc_beam_search_ok(K, V, t))      # the first frame count whose lattice does not fit
    assert ops.ctc_beam_search_ok(K, V, T - 1) and 16 * K * (T - 1) < 160 * 1024 <= 16 * K * T + 16 * 1024
    assert not ops.ctc_beam_search_ok(65, V, 8) and not ops.ctc_beam_search_ok(K, 65, 8) and not ops.ctc_beam_search_ok(0, V, 8)
    enc, lens = _synthetic(1, T, seed=3)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", fused)
        search = PBS.BatchBeamSearch(_product(1.0), None, K, 1.0, 0.0, 0.5, maxlenratio=-12)
        outs.append(search.decode(enc, lens))
        assert search._captured.graph is not None and search.n_steps == [12]
    assert len(outs[0][0]) > 0 and outs[0] == outs[1]


@pytest.mark.parametrize("mode", ["ctc_one_launch", "ctc_stepwise", "attention"])
def test_a_second_decode_of_the_same_shape_reuses_its_buffers(monkeypatch, mode):
    from tavsr.inference import beam_search as PBS
    monkeypatch.setattr(PBS, "CTC_SEARCH_FUSED", mode == "ctc_one_launch")
    pm = _product(0.0 if mode == "attention" else 1.0)
    w = 0.0 if mode == "attention" else 1.0
    with torch.no_grad():
        batches = [pm.encode(synth((2, 160, 80), seed=s).cuda(), torch.tensor(l).cuda()) for s, l in ((7, [160, 120]), (8, [160, 97]))]
    search = PBS.BatchBeamSearch(pm, None, 10, w, 0.0, 0.5)
    caps = []
    for enc, olens in batches:
        got = search.decode(enc, olens)
        caps.append(search._captured)
        want = PBS.BatchBeamSearch(pm, None, 10, w, 0.0, 0.5).decode(enc, olens)
        assert got == want and all(len(g) > 0 for g in got)
    assert caps[0] is caps[1]


@pytest.mark.parametrize("ctc_w,lm_w", [(1.0, 0.0), (1.0, 0.6), (0.0, 0.0)])
def test_skip_zero_weight_on_a_hybrid_model(ctc_w, lm_w):
    """a hybrid model with ctc_weight 0 / 1: the scorer of weight 0 left out (espnet's scorer set) against its launches at weight 0"""
    from tavsr.inference.beam_search import BatchBeamSearch
    _, _, enc, olens = _oracle()
    pm, plm = _product(), _product_lm() if lm_w else None
    keep = BatchBeamSearch(pm, plm, 5, ctc_w, lm_w, 0.5)
    skip = BatchBeamSearch(pm, plm, 5, ctc_w, lm_w, 0.5, skip_zero_weight=True)
    assert len(keep.scorers) == len(skip.scorers) + 1
    a, b = keep.decode(enc.cuda(), olens.cuda()), skip.decode(enc.cuda(), olens.cuda())
    for u in range(3):
        assert a[u][0][0] == b[u][0][0], (u, a[u][0], b[u][0])
        assert abs(a[u][0][1] - b[u][0][1]) <= 1e-5 * abs(a[u][0][1])


def test_null_operand_forms_of_the_beam_update_equal_the_torch_expressions():
    """tavsr_beam_select_topk / tavsr_beam_combine_topk / tavsr_beam_reorder with the decoder or the CTC operands NULL against the
    torch-op route of the step (log-softmax by tavsr_log_softmax_rows, then elementwise torch and torch.topk): same top_i, top_s bit-equal"""
    from tavsr import ops
    torch.manual_seed(1)
    U, K, eos, w_lm, w_len, w_ctc = 3, 5, V - 1, 0.6, 0.5, 0.7
    N = U * K
    z_lm = (torch.randn(N, V) * 3).cuda()
    dec = torch.log_softmax(torch.randn(N, V) * 3, dim=-1).cuda()
    psi, psi_abs = (torch.randn(N, V) * 4 - 20).cuda(), (torch.randn(N, V) * 4 - 40).cuda()
    eos_s, eos_abs, s_prev = (torch.randn(N) * 3 - 10).cuda(), (torch.randn(N) * 3 - 30).cuda(), (torch.randn(N) * 3 - 20).cuda()
    score = (torch.randn(N) * 5 - 30).cuda()
    score[3] = -float("inf")

    def torch_route(full, C, ctc):
        if not ctc:
            weighted = full + score.unsqueeze(1)
        else:
            cand = torch.topk(full, C, dim=-1)[1]
            p = torch.where(cand == eos, eos_s.unsqueeze(1), psi.gather(1, cand))
            ctc_full = torch.full((N, V), -10000000000.0, device="cuda") - s_prev.unsqueeze(1)
            ctc_full[:, eos] = eos_s
            ctc_full.scatter_(1, cand, p)
            weighted = full + w_ctc * ctc_full + score.unsqueeze(1)
        return torch.topk(weighted.view(U, K * V), K, dim=-1)

    # decoder absent: the row is w_lm log_softmax(z_lm) + add (pre-beam of 7, and every token), or add alone (every token)
    full_lm = ops.log_softmax_rows(z_lm, alpha=w_lm, add=w_len)
    for z, full, C in ((z_lm, full_lm, 7), (z_lm, full_lm, V), (None, torch.full((N, V), w_len, device="cuda"), V)):
        pa = psi_abs.clone()
        ts, ti, f_out, _, cand = ops.beam_select_topk(None, z, w_lm, w_len, psi, pa, eos_s, eos_abs, s_prev, score, eos, w_ctc, K, C, keep=True)
        want_s, want_i = torch_route(full, C, True)
        assert torch.equal(f_out, full) and torch.equal(ti, want_i) and torch.equal(ts, want_s)
        assert torch.equal(pa[:, eos], eos_abs) and torch.equal(pa[:, :eos], psi_abs[:, :eos])
        if C < V:
            assert torch.equal(cand, torch.topk(full, C, dim=-1)[1])
    # CTC absent: weighted = full + score, in the one-launch update and in tavsr_beam_combine(_topk)
    full_dl = ops.log_softmax_rows(z_lm, out=(0.3 * dec).contiguous(), alpha=w_lm, add=w_len, accumulate=True)
    for d, z, add, full in ((0.3 * dec, z_lm, w_len, full_dl), (dec + w_len, None, 0.0, dec + w_len)):
        want_s, want_i = torch_route(full, V, False)
        ts, ti = ops.beam_select_topk(d.contiguous(), z, w_lm, add, None, None, None, None, None, score, eos, 0.0, K, V)
        assert torch.equal(ti, want_i) and torch.equal(ts, want_s)
        ts, ti, w = ops.beam_combine_topk(full, None, None, None, None, None, None, score, eos, 0.0, K, keep_weighted=True)
        assert torch.equal(ti, want_i) and torch.equal(ts, want_s) and torch.equal(w, full + score.unsqueeze(1))
        assert torch.equal(ops.beam_combine(full, None, None, None, None, None, None, score, eos, 0.0), w)
    # re-ordering without CTC state
    steps, i = 9, 4
    yseq = torch.randint(0, V, (N, steps + 2)).cuda()
    anc = torch.randint(0, 1000, (N, steps), dtype=torch.int32).cuda()
    ctr = torch.tensor([i, i + 1], dtype=torch.int64).cuda()
    hist = torch.zeros(steps, 3, N, dtype=torch.int32).cuda()
    maxl = torch.tensor([20, i + 1, 20], dtype=torch.int32).cuda()
    outs = (None, None, torch.empty_like(yseq), torch.empty_like(anc), torch.empty(N, dtype=torch.int64).cuda(), torch.empty(N).cuda())
    ops.beam_reorder(want_i, want_s, None, None, None, yseq, anc, outs, K, V, ctr.view(torch.int32)[0:1], hist=hist, maxlen=maxl, eos=eos)
    prev = (want_i // V + (torch.arange(U).cuda() * K).view(U, 1)).view(N)
    new_tok = (want_i % V).view(N)
    y_want = yseq[prev]
    y_want[:, i + 1] = new_tok
    a_want = anc[prev].clone()
    a_want[:, i + 1] = torch.arange(N, dtype=torch.int32).cuda() + (i + 1) * N
    kill = (new_tok == eos) | (torch.arange(N).cuda() // K == 1)
    s_want = torch.where(kill, torch.full_like(want_s.view(N), -float("inf")), want_s.view(N))
    for g, w in zip(outs[2:], (y_want, a_want, new_tok, s_want)):
        assert torch.equal(g, w)
    assert torch.equal(hist[i, 0], new_tok.to(torch.int32)) and torch.equal(hist[i, 1], prev.to(torch.int32))
    assert torch.equal(hist[i, 2].view(torch.float32), want_s.view(N))


@pytest.mark.parametrize("model_ctc_weight", [1.0, 0.0])
def test_speech2text_on_models_with_one_scorer_module(model_ctc_weight):
    """waveform in, text out, on the CTC-only and the attention-only model: the token ids are those of decode() on model.encode's output"""
    from tavsr.inference.beam_search import BatchBeamSearch, Speech2Text
    pm = _product(model_ctc_weight, input_size=None)
    wav = 0.1 * synth((2, 24000), seed=21, kind="uniform")
    lens = torch.tensor([24000, 17600])
    wav[1, 17600:] = 0
    s2t = Speech2Text(pm, None, beam_size=5, ctc_weight=model_ctc_weight, lm_weight=0.0, penalty=0.5, nbest=2)
    res = s2t(wav.cuda(), lens.cuda())
    with torch.no_grad():
        enc, olens = pm.encode(wav.cuda(), lens.cuda())
    want = BatchBeamSearch(pm, None, 5, model_ctc_weight, 0.0, 0.5).decode(enc, olens, nbest=2)
    assert len(res) == 2 and all(1 <= len(r) <= 2 for r in res)
    for u in range(2):
        text, token, token_int, (ys, sc) = res[u][0]
        assert ys == want[u][0][0] and ys[0] == pm.sos and ys[-1] == pm.eos
        assert token_int == [t for t in ys[1:-1] if t != 0] and len(token) == len(token_int)
        assert text == "".join(token).replace("<space>", " ")
