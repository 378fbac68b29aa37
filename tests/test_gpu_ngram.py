"""The n-gram scorer on the device: tavsr_ngram_score (ops.ngram_score) against the float64 reference of tests/ngram_ref.py, and the
beam search with the n-gram on against the oracle's BatchBeamSearch with the reference scorer under "ngram".

Kernel tolerance 1e-4 absolute, derived: a score is a sum of at most 8 fp32 terms (one log10 p, up to 7 backoffs) of magnitude at
most 100, each stored with a rounding inside 2^-24 * 128 = 7.6e-6 (half an ulp below 128 is 3.8e-6), plus as many additions of sums that
stay below 128 in practice: 16 * 3.8e-6 = 6.1e-5 < 1e-4.  The generated models' values stay below 10, where the same count gives 8e-6;
the worst difference seen is printed by each case.

Search: models, LM and inputs of tests/test_gpu_search_modes.py; an order-3 generated model over TOKENS_EN at ngram_weight 0.9, beam 5.
Gaps between the oracle's first and second hypothesis (asserted >= 1e-3 in every case; measured on the CPU when the seed was chosen)
are printed by each case.  With the model seed below the smallest gap over the five cases is 7.7e-2 (decoder absent, utterance 0), and the
smallest margin between the 7th and 8th score at the oracle's pre-beam is 1.4e-4 (an exact tie there - two words of equal counts - would
leave the candidate set to the tie rule of topk; seeds with such a tie were passed over)."""
import argparse
import functools

import numpy as np
import pytest
import torch

import ngram_ref as R
from helpers import TOKENS_EN, asr_conf
from oracle import beam_search as BS
from oracle.model import build_asr_oracle, fill_parameters_, synth

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 3, 5)
VOCABS = (41, 64, 65, 300)
N_ROWS = 7


# ================================================================================================ kernel against the reference
def _token_list(V):
    """<blank>, <unk>, V - 4 words, <eos>, <sos/eos>; every 7th word is left out of the ARPA (its token scores as <unk>)"""
    words = [f"w{i}" for i in range(V - 4)]
    return ["<blank>", "<unk>"] + words + ["<eos>", "<sos/eos>"], [w for i, w in enumerate(words) if i % 7 != 3]


def _planted(W, order):
    """sentences that put the cases the kernel test asserts into the counts: a context of order - 1 words with 12 continuations (a
    highest-order hit, first and last child of a wide range), and two words r, q that occur nowhere else - r .. r q gives a child
    range of length 1, (.. q </s>) a listed context without children, (q r) a suffix that is not listed"""
    C = list(W[1:order])
    wide = [[W[0]] + C + [x] for x in W[2:14]]
    r, q = W[-2], W[-1]
    return wide + [[r] * max(order - 1, 1) + [q]], C, r, q


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    root = tmp_path_factory.mktemp("ngram")
    cache = {}

    def get(order, V):
        if (order, V) not in cache:
            tokens, W = _token_list(V)
            planted, C, r, q = _planted(W, order)
            sents = R.random_sentences(W[:-2], 6 * V, seed=100 * order + V) + planted
            path = root / f"o{order}_v{V}.arpa"
            R.write_arpa(path, sents, order, W)
            ref = R.RefNgram(path, tokens)
            tid = {t: i for i, t in enumerate(tokens)}
            rng = np.random.RandomState(order + V)
            L = order + 3                                           # columns: <sos>, order + 1 tokens, one the scorer never reads
            known = [tid[w] for w in W[:-2]]
            tails = [[tid[w] for w in [W[0]] + C],                                                      # the wide context
                     [tid[r]] * (order - 1),                                                            # child range of length 1
                     [tid[r]] * max(order - 3, 0) + ([tid[q]] if order >= 3 else []) + [tid["<eos>"]],  # listed, no children
                     [tid[q], tid[r]],                                                                  # a suffix that is not listed
                     [tid["<blank>"], tid[W[1]]],                                                       # <unk> inside the context
                     [],
                     []]
            rows = []
            for n, tail in enumerate(tails):
                body = [int(x) for x in rng.choice(known, size=order + 1)]
                if n == 6:                                          # a planted sentence from its start: hits behind short contexts
                    body[:order] = [tid[w] for w in [W[0]] + C]
                tail = tail[-(order + 1):]
                body[len(body) - len(tail):] = tail
                rows.append([V - 1] + body + [tid["<eos>"]])
            yseq = torch.tensor(rows, dtype=torch.int64)
            assert yseq.shape == (N_ROWS, L)
            from tavsr.lm.ngram import NgramLM
            cache[order, V] = (ref, NgramLM.from_arpa(path, tokens, "cuda"), yseq)
        return cache[order, V]
    return get


def _want(ref, yseq, step):
    return np.stack([ref.score(row[:step + 1]) for row in yseq.tolist()])


def _tags(ref, yseq, steps):
    """which of the planted cases the inputs contain: the reference's trace of every (row, step, token)"""
    tags = set()
    order = ref.order
    for step in steps:
        for row in yseq.tolist():
            ctx = ref.context_words(row[:step + 1])
            if "<unk>" in ctx[1:] or (len(ctx) == order - 1 and "<unk>" in ctx):
                tags.add("unk_in_context")
            for v, w in enumerate(ref.word_of):
                ev = ref.trace(ctx, w)[1]
                if w == "<unk>" and ref.token_list[v] != "<unk>":
                    tags.add("unk_token")
                for j, listed, hit, nkids, pos in ev:
                    if j == 0:
                        if sum(1 for e in ev if e[1] and e[0] > 0) >= 1 and len(ctx) == order - 1:
                            tags.add("chain_to_unigram")
                        continue
                    if not listed:
                        tags.add("unlisted_suffix")
                        continue
                    if nkids == 0:
                        tags.add("no_children")
                    if nkids == 1:
                        tags.add("range_1")
                    if hit and j == order - 1:
                        tags.add("top_hit")
                    if hit and nkids >= 9 and pos == 0:
                        tags.add("first_of_9")
                    if hit and nkids >= 9 and pos == nkids - 1:
                        tags.add("last_of_9")
    return tags


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("order", ORDERS)
def test_kernel_matches_the_reference(models, order, V):
    from tavsr import ops
    ref, lm, yseq = models(order, V)
    steps = (0, 1, 2, order + 1)
    # the planted cases are IN the inputs (order 1 has no context; order 2's one-word contexts are all listed where the model has <unk>)
    need = {"unk_token"}
    if order >= 2:
        need |= {"top_hit", "chain_to_unigram", "no_children", "range_1", "first_of_9", "last_of_9", "unk_in_context"}
    if order >= 3:
        need |= {"unlisted_suffix"}
    tags = _tags(ref, yseq, steps)
    assert need <= tags, (order, V, need - tags)
    worst = 0.0
    for N in (1, N_ROWS):
        y = yseq[:N].cuda()
        for step in steps:
            got = ops.ngram_score(lm, y, step)
            want = _want(ref, yseq[:N], step)
            assert got.shape == (N, V) and got.dtype == torch.float32
            err = float(np.max(np.abs(got.double().cpu().numpy() - want)))
            worst = max(worst, err)
            assert err < 1e-4, (order, V, N, step, err)
    print(f"order {order} V {V}: cases {sorted(tags)}, worst |kernel - reference| = {worst:.2e}")


def test_alpha_add_accumulate_candidates_and_row_stride(models):
    from tavsr import ops
    ref, lm, yseq = models(3, 65)
    V, step = 65, 4
    y = yseq.cuda()
    want = torch.from_numpy(_want(ref, yseq, step))
    base = (torch.arange(N_ROWS * V, dtype=torch.float32).view(N_ROWS, V) * 0.25 - 7.0)
    # alpha and add without accumulate, into a row holding NaN (every element is written)
    out = torch.full((N_ROWS, V), float("nan"), device="cuda")
    assert ops.ngram_score(lm, y, step, out=out, alpha=0.9, add=0.5) is out
    assert not bool(torch.isnan(out).any()) and float((out.double().cpu() - (0.9 * want + 0.5)).abs().max()) < 1e-4
    fresh = ops.ngram_score(lm, y, step)                      # under TAVSR_POISON=nan a new block holds NaN
    assert not bool(torch.isnan(fresh).any()) and torch.equal(fresh, ops.ngram_score(lm, y, step))
    # accumulate onto known values
    out = base.clone().cuda()
    ops.ngram_score(lm, y, step, out=out, alpha=-0.3, accumulate=True)
    assert float((out.double().cpu() - (base.double() - 0.3 * want)).abs().max()) < 1e-4
    assert torch.equal(out, base.cuda() + (-0.3 * fresh))      # the kernel's own arithmetic: out + alpha * s + 0
    # a candidate list: these tokens alone, the rest of the row untouched; a padded row stride
    cand = torch.stack([torch.randperm(V, generator=torch.Generator().manual_seed(n))[:9] for n in range(N_ROWS)]).cuda()
    wide = torch.zeros(N_ROWS, V + 3, device="cuda")
    wide[:, :V] = base.cuda()
    wide[:, V:] = 123.0
    ops.ngram_score(lm, y, step, out=wide[:, :V], alpha=0.9, accumulate=True, cand=cand)
    expect = base.cuda().clone()
    expect.scatter_(1, cand, (base.cuda() + 0.9 * fresh).gather(1, cand))
    assert torch.equal(wide[:, :V], expect) and bool((wide[:, V:] == 123.0).all())


def test_device_counter_equals_host_index_inside_a_captured_graph(models):
    from tavsr import ops
    ref, lm, yseq = models(5, 300)
    y = yseq.cuda()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(N_ROWS, 300, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ngram_score(lm, y, 0, out=out, step_dev=ctr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ngram_score(lm, y, 0, out=out, alpha=0.9, step_dev=ctr)
    for step in (0, 2, 6):
        ctr.fill_(step)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.ngram_score(lm, y, step, alpha=0.9)), step
    # a counter beyond the buffer is clamped to its last column (never an index past the row)
    ctr.fill_(1000)
    graph.replay()
    assert torch.equal(out, ops.ngram_score(lm, y, y.shape[1] - 1, alpha=0.9))


def test_refusals(models):
    from tavsr import _lib
    _, lm, yseq = models(2, 41)
    y, out = yseq.cuda(), torch.full((N_ROWS, 41), 7.0, device="cuda")
    p = _lib.ptr

    def call(order, word):
        return _lib.lib().tavsr_ngram_score(word, p(lm.logp), p(lm.backoff), p(lm.child_begin), lm.n_unigrams, order, lm.bos_word, -100.0,
                                            p(lm.word_map), p(y), y.stride(0), y.shape[1], 1, None, None, 0, 1.0, 0.0, 0, p(out), 41,
                                            N_ROWS, 41, _lib.stream())
    assert call(_lib.ENUMS["TAVSR_NGRAM_MAX_ORDER"] + 1, p(lm.word)) == _lib.ENUMS["TAVSR_EUNSUPPORTED"]
    assert "order 9" in _lib.lib().tavsr_last_error_string().decode()
    assert call(2, None) == _lib.ENUMS["TAVSR_EINVAL"]
    assert call(0, p(lm.word)) == _lib.ENUMS["TAVSR_EINVAL"]
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    assert call(2, p(lm.word)) == 0


# ================================================================================================ search against the oracle
LM_KW = dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0)
V = len(TOKENS_EN)
BEAM, W_NGRAM, PEN = 5, 0.9, 0.5
SEED = 1                                                     # of the generated order-3 model


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
    return pm.cuda()


@functools.lru_cache(maxsize=None)
def _product_lm():
    from tavsr.lm.transformer_lm import TransformerLM
    plm = TransformerLM(V, **LM_KW).eval()
    fill_parameters_(plm, seed=6)
    return plm.cuda()


def _arpa_words():
    """the words of the search's n-gram: TOKENS_EN without the specials and without the digits 7 - 9 (tokens that score as <unk>)"""
    return [t for t in TOKENS_EN if not t.startswith("<") and t not in "789"] + ["<space>"]


def write_search_arpa(path, planted_token=None):
    """order 3 over TOKENS_EN; ``planted_token``: every n-gram that ends in it is rewritten to log10 p = -30, so that the token scores
    -30 (plus backoffs <= 0) in every context"""
    words = _arpa_words()
    R.write_arpa(path, R.random_sentences(words, 400, seed=SEED, max_len=12, skew=0.8), 3, words)
    if planted_token is not None:
        out = []
        for line in open(path).read().split("\n"):
            f = line.split("\t")
            if len(f) >= 2 and f[1].split(" ")[-1] == planted_token:
                f[0] = "-30.0"
            out.append("\t".join(f))
        open(path, "w").write("\n".join(out))
    return path


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    return write_search_arpa(tmp_path_factory.mktemp("search") / "chars3.arpa")


CASES = {                                     # name: (decoder, ctc, lm_weight, ngram_scorer)
    "hybrid": (True, True, 0.0, "full"),
    "hybrid_lm": (True, True, 0.6, "full"),
    "no_decoder": (False, True, 0.0, "full"),         # the n-gram is the only full scorer beside the length bonus
    "no_ctc": (True, False, 0.0, "full"),
    "hybrid_part": (True, True, 0.0, "part"),
}
_REF = {}


def reference(path, name):
    """the oracle's search with the reference scorer under "ngram", one utterance at a time (computed once per case)"""
    if name in _REF:
        return _REF[name]
    decoder, ctc, lm_w, mode = CASES[name]
    m, lm, enc, olens = _oracle()
    ng = R.RefNgram(path, TOKENS_EN)
    ctc_w = 0.3 if (decoder and ctc) else (1.0 if ctc else 0.0)
    if name == "no_decoder":
        ctc_w = 0.3                                      # a pre-beam with the n-gram alone to rank: the case the lifted refusal opens
    scorers = dict(decoder=BS.DecoderScorer(m.decoder) if decoder else None, ctc=BS.CTCPrefixScorer(ctc=m.ctc, eos=m.eos) if ctc else None,
                   length_bonus=BS.LengthBonus(V), lm=lm if lm_w else None,
                   ngram=R.OracleNgramPart(ng) if mode == "part" else R.OracleNgramFull(ng))
    weights = dict(decoder=(1.0 - ctc_w) if decoder else 0.0, ctc=ctc_w, lm=lm_w, length_bonus=PEN, ngram=W_NGRAM)
    out = []
    with torch.no_grad():
        for u in range(3):
            bs = BS.BatchBeamSearch(scorers, weights, BEAM, V, m.sos, m.eos, pre_beam_score_key="full")
            if mode == "part":
                bs.part["ngram"] = bs.full.pop("ngram")
            assert "ngram" in bs.weights and bs.do_pre_beam == ctc
            hyps = bs.forward(enc[u, : int(olens[u])])
            out.append([(h.yseq.tolist(), float(h.score)) for h in hyps])
    _REF[name] = (out, ctc_w)
    return _REF[name]


def _search(path, name, **kw):
    from tavsr.inference.beam_search import BatchBeamSearch
    from tavsr.lm.ngram import NgramLM
    decoder, ctc, lm_w, mode = CASES[name]
    _, ctc_w = reference(path, name)
    pm = _product(None if (decoder and ctc) else (1.0 if ctc else 0.0))
    ng = NgramLM.from_arpa(path, TOKENS_EN, "cuda")
    return BatchBeamSearch(pm, _product_lm() if lm_w else None, BEAM, ctc_w, lm_w, PEN, ngram=ng, ngram_weight=W_NGRAM, ngram_scorer=mode, **kw)


def _check_against_reference(hip, ref):
    """the assertions of tests/test_gpu_search_modes.py:_check_against_reference, and the oracle's own margin"""
    for u in range(3):
        assert len(hip[u]) > 0 and len(ref[u]) > 1
        gap = ref[u][0][1] - ref[u][1][1]
        print(f"utterance {u}: best score {hip[u][0][1]:.6f}, oracle {ref[u][0][1]:.6f}, rel {abs(hip[u][0][1] - ref[u][0][1]) / abs(ref[u][0][1]):.2e}, "
              f"oracle's first - second {gap:.3e}")
        assert gap >= 1e-3, (u, gap)
        assert hip[u][0][0] == ref[u][0][0], (u, hip[u][0], ref[u][0])
        assert abs(hip[u][0][1] - ref[u][0][1]) < 2e-4 * abs(ref[u][0][1])
        top_h = {tuple(h[0]) for h in hip[u][:3]}
        top_r = {tuple(h[0]) for h in ref[u][:3]}
        assert len(top_h & top_r) >= 2, (u, top_h, top_r)


@pytest.mark.parametrize("name", list(CASES))
def test_search_with_ngram_matches_oracle(arpa, name):
    _, _, enc, olens = _oracle()
    search = _search(arpa, name)
    assert search.scorers[-1] == "ngram" and search.has_ngram
    if name == "no_decoder":
        assert search.pre_beam and not search.has_dec and not search.has_lm
    hip = search.decode(enc.cuda(), olens.cuda())
    assert search._captured.graph is not None
    _check_against_reference(hip, reference(arpa, name)[0])


@pytest.mark.parametrize("name", list(CASES))
def test_eager_and_captured_routes_agree_bit_for_bit(monkeypatch, arpa, name):
    from tavsr.inference import beam_search as PBS
    _, _, enc, olens = _oracle()
    outs = []
    for graph in (True, False):
        monkeypatch.setattr(PBS, "GRAPH_STEP", graph)
        search = _search(arpa, name)
        outs.append(search.decode(enc.cuda(), olens.cuda()))
        assert (search._captured is not None) == graph
    assert all(len(o) > 0 for o in outs[0]) and outs[0] == outs[1]


def test_a_planted_ngram_drives_a_token_out_of_the_best_hypothesis(tmp_path):
    """the n-gram must change the search: a token of the best hypothesis found without n-gram gets log10 p = -30 in every context -
    the best hypothesis then differs and does not contain the token (weight 0.9: -27 per occurrence against scores of about -3 per token)"""
    from tavsr.inference.beam_search import BatchBeamSearch
    from tavsr.lm.ngram import NgramLM
    _, _, enc, olens = _oracle()
    pm = _product()
    plain = BatchBeamSearch(pm, None, BEAM, 0.3, 0.0, PEN).decode(enc.cuda(), olens.cuda())
    words = set(_arpa_words())
    tok = next(t for t in plain[0][0][0][1:-1] if TOKENS_EN[t] in words)
    ng = NgramLM.from_arpa(write_search_arpa(tmp_path / "planted.arpa", TOKENS_EN[tok]), TOKENS_EN, "cuda")
    hip = BatchBeamSearch(pm, None, BEAM, 0.3, 0.0, PEN, ngram=ng, ngram_weight=W_NGRAM).decode(enc.cuda(), olens.cuda())
    assert hip[0][0][0] != plain[0][0][0] and tok not in hip[0][0][0], (tok, hip[0][0], plain[0][0])


def test_a_second_decode_reuses_the_captured_step_and_toggling_the_ngram_restores_the_first_result(arpa):
    from tavsr.inference.beam_search import BatchBeamSearch
    _, _, enc, olens = _oracle()
    search = _search(arpa, "hybrid")
    ng = search.ngram
    with_ng = search.decode(enc.cuda(), olens.cuda())
    cap = search._captured
    assert search.decode(enc.cuda(), olens.cuda()) == with_ng and search._captured is cap
    # without, with, without on one batch: the scorer set is part of the captured step's key
    search.ngram = None
    assert search.scorers[-1] != "ngram"
    without = search.decode(enc.cuda(), olens.cuda())
    assert search._captured is not cap and without != with_ng
    assert without == BatchBeamSearch(_product(), None, BEAM, 0.3, 0.0, PEN).decode(enc.cuda(), olens.cuda())
    search.ngram = ng
    assert search.decode(enc.cuda(), olens.cuda()) == with_ng
    search.ngram = None
    assert search.decode(enc.cuda(), olens.cuda()) == without
    # weight 0 drops the scorer as None does
    assert BatchBeamSearch(_product(), None, BEAM, 0.3, 0.0, PEN, ngram=ng, ngram_weight=0.0).scorers == search.scorers


def test_part_without_pre_beam_is_full_and_the_one_launch_route_is_not_taken(arpa):
    from tavsr.inference.beam_search import BatchBeamSearch
    from tavsr.lm.ngram import NgramLM
    _, _, enc, olens = _oracle()
    ng = NgramLM.from_arpa(arpa, TOKENS_EN, "cuda")
    outs = []
    for mode in ("full", "part"):
        search = BatchBeamSearch(_product(1.0), None, BEAM, 1.0, 0.0, PEN, ngram=ng, ngram_weight=W_NGRAM, ngram_scorer=mode)
        assert not search.pre_beam and not search._ngram_part
        outs.append(search.decode(enc.cuda(), olens.cuda()))
        assert search._captured.graph is not None              # token by token: the one-launch CTC search has no n-gram
    assert outs[0] == outs[1] and all(len(o) > 0 for o in outs[0])
    with pytest.raises(ValueError):                            # a part n-gram gives the pre-beam nothing to rank: the refusal stays
        BatchBeamSearch(_product(1.0), None, BEAM, 0.3, 0.0, PEN, ngram=ng, ngram_scorer="part")
    with pytest.raises(ValueError):
        BatchBeamSearch(_product(1.0), None, BEAM, 0.3, 0.0, PEN, ngram=ng, ngram_scorer="both")


def test_speech2text_with_an_ngram_file(arpa):
    from tavsr.inference.beam_search import BatchBeamSearch, Speech2Text
    from tavsr.lm.ngram import NgramLM
    pm = _product(None, input_size=None)
    wav = 0.1 * synth((1, 24000), seed=21, kind="uniform")
    lens = torch.tensor([24000])
    s2t = Speech2Text(pm, None, beam_size=BEAM, ctc_weight=0.3, lm_weight=0.0, penalty=PEN, nbest=2, ngram_file=str(arpa))
    assert s2t.beam_search.scorers == ("decoder", "ctc", "length_bonus", "ngram") and s2t.beam_search.w_ngram == 0.9
    res = s2t(wav.cuda(), lens.cuda())
    with torch.no_grad():
        enc, olens = pm.encode(wav.cuda(), lens.cuda())
    ng = NgramLM.from_arpa(arpa, TOKENS_EN, "cuda")
    want = BatchBeamSearch(pm, None, BEAM, 0.3, 0.0, PEN, ngram=ng, ngram_weight=0.9).decode(enc, olens, nbest=2)
    text, token, token_int, (ys, sc) = res[0][0]
    assert ys == want[0][0][0] and sc == want[0][0][1] and ys[0] == pm.sos and ys[-1] == pm.eos
    assert token_int == [t for t in ys[1:-1] if t != 0] and text == "".join(token).replace("<space>", " ")
    assert Speech2Text(pm, None, beam_size=BEAM, ctc_weight=0.3, lm_weight=0.0, ngram_file=str(arpa), ngram_weight=0.0).beam_search.scorers == \
        ("decoder", "ctc", "length_bonus")
