"""GPU: the time-synchronous beam search (tavsr/inference/timesync.py, csrc/timesync.hip) against the fp64 restatement of espnet's
BeamSearchTimeSync (tests/timesync_ref.py), the scorer launches for rows at different depths against torch fp64, and the model-level
search against the restatement driven by the oracle's decoder and LM.

Synthetic inputs: z = N(0, 1) * scale with z[:, 0] += 1, log-softmax, cast to fp32; seeds 0 .. n-1 are the utterances of ONE batch.
The optional "decoder" is a bigram table: row(prefix) = log_softmax(2 N(0, 1) [V, V])[prefix[-1]], w_ctc 0.3, w_dec 0.7.  An
utterance is BINDING when the reference's mingap (the smallest distance, over its frames, between what the beam / the pre-beam keeps
and what it drops) exceeds 1e-4, the project's greedy-id bar: there the hypothesis lists must be equal, token for token and in order.

Every test here that touches the product fails at the parent commit: the entries (tavsr_timesync_*, tavsr_tree_attn_rows,
tavsr_embed_pe_rows), the module and the ``time_sync`` keyword do not exist there.  ``test_the_inputs_exercise_re_entry_and_the_merge``
runs the fp64 reference alone - a condition on the inputs - and passes there too.

What the inputs do NOT exercise: with the CTC term alone the reference counts 0 re-entries on every shape, so the routes without scorer
(the one-launch search, the stepped search with NULL rows) never meet a prefix that comes back into the beam; canonical node identity
is exercised by the stepped route with the decoder term only (20 and 10 re-entries over the utterances of the first two shapes)."""
import argparse
import functools

import numpy as np
import pytest
import torch

from helpers import TOKENS_EN, asr_conf
from timesync_ref import timesync_search

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3, 30, 2, 40), (7, 2, 40, 1, 40), (70, 10, 40, 3, 20), (41, 10, 25, 3, 20)]      # V, K, T, scale, n
BINDING = 1e-4
# Largest |score - fp64 reference| over the binding utterances of every shape and route, measured on the MI355X: 1.474e-5 (V 70, beam
# 10, with the decoder term, scores down to -75; 1.3e-6 .. 9.7e-6 for the other shapes and routes): fp32 sums of ~40 terms.  Asserted: 8 x.
MEASURED = 1.5e-5
TOL = 8 * MEASURED


def _lpz(V, T, scale, seed):
    z = np.random.RandomState(seed).standard_normal((T, V)) * scale
    z[:, 0] += 1.0
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _bigram(V):
    z = 2.0 * np.random.RandomState(1000 + V).standard_normal((V, V))
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(shape):
    V, K, T, scale, n = shape
    return np.stack([_lpz(V, T, scale, s) for s in range(n)])


@functools.lru_cache(maxsize=None)
def _reference(shape, dec):
    """the fp64 search of every utterance of the shape's batch, computed once"""
    V, K, T, scale, n = shape
    tab = _bigram(V).astype(np.float64)
    kw = dict(w_ctc=0.3, w_dec=0.7, dec_row=lambda l: tab[l[-1]]) if dec else dict(w_ctc=0.3)
    return [timesync_search(lpz, K, V - 1, pen=0.5, **kw) for lpz in _batch(shape)]


def _search(shape, dec, **kw):
    from tavsr.inference.timesync import TimeSyncSearch
    V, K, T, scale, n = shape
    if not dec:
        return TimeSyncSearch(V, V - 1, K, 0.3, 0.0, 0.0, 0.5, **kw)
    tab = torch.from_numpy(_bigram(V)).cuda()
    return TimeSyncSearch(V, V - 1, K, 0.3, 0.7, 0.0, 0.5, dec_fn=lambda rows, out: tab[rows.tok], **kw)      # torch indexing, no host read


def _decode(shape, dec, lens=None, search=None):
    V, K, T, scale, n = shape
    lpz = torch.from_numpy(_batch(shape)).cuda()
    lens = torch.full((n,), T, dtype=torch.int64) if lens is None else lens
    search = _search(shape, dec) if search is None else search
    return search.search(lpz, lens.cuda()), search


def _compare(shape, got, ref):
    V, K, T, scale, n = shape
    binding = [u for u in range(n) if ref[u].mingap > BINDING]
    worst = 0.0
    for u in binding:
        assert [h[0] for h in got[u]] == [h[0] for h in ref[u].hyps], (u, got[u][:2], ref[u].hyps[:2])
        worst = max(worst, max(abs(g[1] - r[1]) for g, r in zip(got[u], ref[u].hyps)))
    low = min(r[1] for u in binding for r in ref[u].hyps)
    print(f"shape {shape}: binding {len(binding)}/{n}, largest score deviation {worst:.3e} (scores down to {low:.1f})")
    assert len(binding) >= 0.8 * n                       # a condition on the inputs (reference alone)
    assert worst <= TOL
    return worst


def test_the_inputs_exercise_re_entry_and_the_merge():
    """conditions on the inputs, asserted on the reference alone: over the first two shapes a prefix re-enters the beam after it had
    dropped out of dp (canonical node identity is exercised) and the fell-off-the-beam merge runs"""
    for dec in (False, True):
        for shape in SHAPES[:2]:
            refs = _reference(shape, dec)
            re, mg = sum(r.reentries for r in refs), sum(r.merges for r in refs)
            print(f"shape {shape}, decoder {dec}: re-entries {re}, merges {mg}")
            assert mg >= 100 and (re >= 1 or not dec)      # (the CTC term alone never brings a prefix back here: 0 re-entries measured)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_launch_search_matches_the_reference(shape):
    got, search = _decode(shape, False)
    assert search.route == "one_launch"
    _compare(shape, got, _reference(shape, False))


@pytest.mark.parametrize("shape", SHAPES)
def test_stepped_search_with_a_decoder_matches_the_reference(shape):
    """scorer rows filled on the device from the bigram table; the frame step is a replayed graph"""
    got, search = _decode(shape, True)
    assert search.route == "graph"
    _compare(shape, got, _reference(shape, True))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_routes_agree_bit_for_bit_without_scorer(monkeypatch, shape):
    from tavsr.inference import timesync as TS
    one, _ = _decode(shape, False)
    monkeypatch.setattr(TS, "ONE_LAUNCH", False)
    graph, s = _decode(shape, False)
    assert s.route == "graph"
    monkeypatch.setattr(TS, "GRAPH_STEP", False)
    eager, s = _decode(shape, False)
    assert s.route == "eager"
    assert one == graph == eager and all(len(h) > 0 for h in one)


LARGE_LDS = (600, 20, 8, 3, 4)      # V, K, T, scale, n: pre-beam 30, 1220 entries, a dp table of 4096 places


@pytest.mark.parametrize("dec", [False, True])
def test_a_shape_with_more_than_48_kb_of_lds_matches_the_reference(dec):
    """the state image alone is 50 KB, the frame's tables 85 KB: both kernels must raise their dynamic-LDS limit before the launch
    (one launch without the decoder term, the stepped route with it)"""
    from tavsr import ops
    V, K, T, scale, n = LARGE_LDS
    words, off = ops.timesync_ws(K, V, T, int(1.5 * K))
    assert off["parent"] * 4 > 48 * 1024                 # (the trie follows the state image in the workspace)
    got, search = _decode(LARGE_LDS, dec)
    assert search.route == ("graph" if dec else "one_launch")
    _compare(LARGE_LDS, got, _reference(LARGE_LDS, dec))


@pytest.mark.parametrize("dec", [False, True])
def test_ragged_batch_equals_every_utterance_alone(dec):
    shape = SHAPES[0]
    V, K, T, scale, n = shape
    n = 8
    lens = torch.tensor([T - (3 * u) % T for u in range(n)], dtype=torch.int64)
    lens[5] = 1
    lpz = torch.from_numpy(_batch(shape)[:n]).cuda()
    together = _search(shape, dec).search(lpz, lens.cuda())
    alone = _search(shape, dec)
    ref = []
    for u in range(n):
        one = alone.search(lpz[u:u + 1], lens[u:u + 1].cuda())
        assert one[0] == together[u], u                                       # bit for bit
        tab = _bigram(V).astype(np.float64)
        kw = dict(w_ctc=0.3, w_dec=0.7, dec_row=lambda l: tab[l[-1]]) if dec else dict(w_ctc=0.3)
        ref.append(timesync_search(_batch(shape)[u][: int(lens[u])], K, V - 1, pen=0.5, **kw))
    for u in range(n):
        if ref[u].mingap > BINDING:
            assert [h[0] for h in together[u]] == [h[0] for h in ref[u].hyps], u
            assert max(abs(g[1] - r[1]) for g, r in zip(together[u], ref[u].hyps)) <= TOL


def test_a_tie_at_the_threshold_keeps_every_tied_token():
    """V = 9, K = 2: C = 3.  Frame 0 has blank and token 3 on top and tokens 2, 4, 5, 7 tied at the third-largest value: all four are
    candidates, six in all.  The "decoder" (a bigram table) makes 7 by far the likeliest token after <sos>, so (<sos>, 7) enters the beam
    - if 7 is a candidate.  A top-C that cut the tie after three tokens would have dropped it (7 is the last of the tied in token order)."""
    from tavsr.inference.timesync import TimeSyncSearch
    V, K, T, sos = 9, 2, 2, 8
    lpz = np.full((T, V), -6.0, dtype=np.float32)
    lpz[0, [0, 3]] = [-0.5, -1.0]
    lpz[0, [2, 4, 5, 7]] = -2.0
    lpz[1, [0, 1, 3]] = [-0.4, -1.5, -2.5]
    tab = np.full((V, V), -4.0, dtype=np.float32)
    tab[sos, 7] = -0.1
    ref = timesync_search(lpz, K, sos, w_ctc=0.3, w_dec=0.7, dec_row=lambda l: tab[l[-1]].astype(np.float64))
    assert ref.ncand_max == 6 and [h[0] for h in ref.hyps] == [[sos, sos], [sos, 7, sos]]
    cut = timesync_search(lpz, K, sos, w_ctc=0.3, w_dec=0.7, dec_row=lambda l: np.where(np.arange(V) == 7, -np.inf, tab[l[-1]].astype(np.float64)))
    assert all(7 not in h[0] for h in cut.hyps)                           # (what the search gives when 7 cannot be taken)
    dtab = torch.from_numpy(tab).cuda()
    search = TimeSyncSearch(V, sos, K, 0.3, 0.7, dec_fn=lambda rows, out: dtab[rows.tok])
    got = search.search(torch.from_numpy(lpz)[None].cuda(), torch.tensor([T]).cuda())[0]
    assert [h[0] for h in got] == [h[0] for h in ref.hyps]
    assert max(abs(g[1] - r[1]) for g, r in zip(got, ref.hyps)) <= TOL


def test_more_ties_than_the_candidate_list_holds_raise():
    """V = 12, K = 2: C = 3, the list holds 6; a frame with 8 equal values at the threshold is refused after the search, and the other
    utterance of the batch is not what is named"""
    from tavsr.inference.timesync import TimeSyncSearch
    V, K, T = 12, 2, 3
    lpz = np.stack([_lpz(V, T, 2, 0), _lpz(V, T, 2, 1)])
    lpz[1, 1, :] = np.log(1.0 / 12)
    lpz[1, 1, 8:] = np.float32(np.log(1.0 / 12)) - 1.0
    search = TimeSyncSearch(V, V - 1, K, 1.0)
    with pytest.raises(RuntimeError, match=r"utterances \[1\].*tie"):
        search.search(torch.from_numpy(lpz.astype(np.float32)).cuda(), torch.tensor([T, T]).cuda())
    ok = search.search(torch.from_numpy(lpz[:1].astype(np.float32)).cuda(), torch.tensor([T]).cuda())
    assert len(ok[0]) > 0


@pytest.mark.parametrize("dec", [False, True])
def test_a_second_search_of_the_same_shape_replays_and_gives_identical_results(monkeypatch, dec):
    from tavsr.inference import timesync as TS
    monkeypatch.setattr(TS, "ONE_LAUNCH", False)
    shape = SHAPES[3]
    first, search = _decode(shape, dec)
    assert not search.replayed and search.route == "graph"
    graph = search._bufs.graph
    second, _ = _decode(shape, dec, search=search)
    assert search.replayed and search._bufs.graph is graph
    assert first == second
    # another batch through the same capture, then the first again
    V, K, T, scale, n = shape
    other = torch.from_numpy(np.stack([_lpz(V, T, scale, 100 + s) for s in range(n)])).cuda()
    lens = torch.full((n,), T, dtype=torch.int64).cuda()
    got = search.search(other, lens)
    assert search.replayed and got == _search(shape, dec).search(other, lens) and got != first
    assert _decode(shape, dec, search=search)[0] == first


def test_shapes_that_do_not_fit_are_refused_before_any_launch():
    from tavsr import ops
    from tavsr._lib import TavsrError
    assert ops.timesync_ok(10, 41, 99, 15) and ops.timesync_ok(20, 5000, 400, 30)
    assert not ops.timesync_ok(65, 500, 10, 97) and not ops.timesync_ok(10, 41, 99, 42) and not ops.timesync_ok(64, 30000, 10, 96)
    with pytest.raises(TavsrError, match="not supported"):
        ops.timesync_ws(64, 30000, 10, 96)
    ws = torch.zeros(1, 16, dtype=torch.int32).cuda()
    with pytest.raises(TavsrError, match="rc=-3"):
        ops.timesync_search(torch.zeros(1, 10, 30000).cuda(), torch.tensor([10]).cuda(), ws, 64, 96, 1, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------- scorer launches at different depths
DEPTHS = [0, 1, 63, 64, 65, 130, 1, 0, 64]      # keys per row; 0: the row is untouched


@pytest.mark.parametrize("dk", [64, 32, 128])      # 128: the kernel's form with 32 lanes along the head dimension
def test_tree_attention_with_keys_per_row_against_torch_fp64(dk):
    from tavsr import ops
    H, N, ld = 4, len(DEPTHS), 136
    D = H * dk
    g = torch.Generator().manual_seed(dk)
    pool = 700
    kpool, vpool = torch.randn(pool, D, generator=g), torch.randn(pool, D, generator=g)
    qkv = torch.randn(N, 3 * D, generator=g)
    anc = torch.stack([torch.randperm(pool - N, generator=g)[:ld] for _ in range(N)]).to(torch.int32)
    for n, d in enumerate(DEPTHS):
        if d:
            anc[n, d - 1] = pool - N + n                           # the row's own pool row
    nkeys = torch.tensor(DEPTHS, dtype=torch.int32)
    kp, vp, q = kpool.cuda(), vpool.cuda(), qkv.cuda()
    out = torch.full((N, D), 7.0).cuda()
    got = ops.tree_attn_rows(q[:, :D], kp, vp, anc.cuda(), nkeys.cuda(), ld, H, dk, q[:, D:2 * D], q[:, 2 * D:], out=out).cpu()
    worst = 0.0
    for n, d in enumerate(DEPTHS):
        own = pool - N + n
        if d == 0:
            assert torch.equal(got[n], torch.full((D,), 7.0))                                  # left alone
            assert torch.equal(kp[own].cpu(), kpool[own]) and torch.equal(vp[own].cpu(), vpool[own])
            continue
        assert torch.equal(kp[own].cpu(), qkv[n, D:2 * D]) and torch.equal(vp[own].cpu(), qkv[n, 2 * D:])      # appended
        rows = anc[n, :d].long()
        k64, v64 = kpool[rows].double(), vpool[rows].double()
        k64[-1], v64[-1] = qkv[n, D:2 * D].double(), qkv[n, 2 * D:].double()
        qh = qkv[n, :D].double().view(H, dk)
        att = torch.softmax(torch.einsum("hd,jhd->hj", qh, k64.view(d, H, dk)) / dk ** 0.5, dim=-1)
        want = torch.einsum("hj,jhd->hd", att, v64.view(d, H, dk)).reshape(D)
        worst = max(worst, float((got[n].double() - want).abs().max()))
    untouched = torch.ones(pool, dtype=torch.bool)
    untouched[[pool - N + n for n, d in enumerate(DEPTHS) if d]] = False
    assert torch.equal(kp.cpu()[untouched], kpool[untouched]) and torch.equal(vp.cpu()[untouched], vpool[untouched])
    print(f"dk {dk}: largest deviation from fp64 {worst:.2e}")
    assert worst < 2e-5      # fp32 softmax over <= 130 keys of N(0, 1) values: ~130 * 2^-24 relative on sums of magnitude <= 3


def test_embed_pe_with_a_position_per_row_against_torch_fp64():
    from tavsr import ops
    g = torch.Generator().manual_seed(3)
    Vv, D, L = 41, 256, 131
    table, pe = torch.randn(Vv, D, generator=g), torch.randn(L, D, generator=g)
    pos = torch.tensor(DEPTHS + [500, -3], dtype=torch.int32)                       # beyond the table: clamped
    ids = torch.randint(0, Vv, (pos.numel(),), generator=g)
    got = ops.embed_pe_rows(ids.cuda(), table.cuda(), pe.cuda(), 16.0, pos.cuda()).cpu()
    want = table[ids].double() * 16.0 + pe[pos.long().clamp(0, L - 1)].double()
    assert float((got.double() - want).abs().max()) < 1e-5                          # one fp32 multiply-add on values of magnitude <= 70


# ---------------------------------------------------------------------------------------------- model level
LM_KW = dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0)
V = len(TOKENS_EN)


@functools.lru_cache(maxsize=None)
def _oracle():
    """oracle model, LM and inputs of tests/test_gpu_search_modes.py (T = 39 / 30 / 22 encoder frames, 2 + 2 blocks)"""
    from oracle import beam_search as BS
    from oracle.model import build_asr_oracle, fill_parameters_, synth
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
    from oracle.model import fill_parameters_
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
    from oracle.model import fill_parameters_
    from tavsr.lm.transformer_lm import TransformerLM
    plm = TransformerLM(V, **LM_KW).eval()
    fill_parameters_(plm, seed=6)
    return plm.cuda()


@functools.lru_cache(maxsize=None)
def _model_reference(beam, lm_w, decoder=True):
    """the restatement driven by the oracle's one-step scores (DecoderScorer / TransformerLMOracle.batch_score on the whole prefix)"""
    from oracle import beam_search as BS
    m, lm, enc, olens = _oracle()
    scorer = BS.DecoderScorer(m.decoder)
    out = []
    with torch.no_grad():
        lpz_all = m.ctc.log_softmax(enc)
        for u in range(3):
            T = int(olens[u])
            mem = enc[u: u + 1, :T]

            def dec_row(l):
                return scorer.batch_score(torch.tensor([l]), [None], mem)[0][0].double().numpy()

            def lm_row(l):
                return lm.batch_score(torch.tensor([l]), [None], None)[0][0].double().numpy()

            r = timesync_search(lpz_all[u, :T].double().numpy(), beam, m.sos, w_ctc=0.3 if decoder else 1.0, w_dec=0.7 if decoder else 0.0,
                                w_lm=lm_w, pen=0.5, dec_row=dec_row if decoder else None, lm_row=lm_row if lm_w else None)
            out.append(r.hyps)
    return out


def _check_against_reference(hip, ref):
    """the assertions of tests/test_gpu_search_modes.py (copied)"""
    for u in range(3):
        assert len(hip[u]) > 0 and len(ref[u]) > 0
        assert hip[u][0][0] == ref[u][0][0], (u, hip[u][0], ref[u][0])
        print(f"utterance {u}: best score {hip[u][0][1]:.6f}, reference {ref[u][0][1]:.6f}, rel {abs(hip[u][0][1] - ref[u][0][1]) / abs(ref[u][0][1]):.2e}")
        assert abs(hip[u][0][1] - ref[u][0][1]) < 2e-4 * abs(ref[u][0][1])
        top_h = {tuple(h[0]) for h in hip[u][:3]}
        top_r = {tuple(h[0]) for h in ref[u][:3]}
        assert len(top_h & top_r) >= 2, (u, top_h, top_r)


@pytest.mark.parametrize("lm_w", [0.0, 0.6])
@pytest.mark.parametrize("beam", [5, 10])
def test_model_level_search_matches_the_reference(beam, lm_w):
    """all three utterances (T = 39 / 30 / 22) in one batched decode; ctc_weight 0.3"""
    from tavsr.inference.timesync import BeamSearchTimeSync
    _, _, enc, olens = _oracle()
    search = BeamSearchTimeSync(_product(), _product_lm() if lm_w else None, beam, 0.3, lm_w, 0.5)
    hip = search.decode(enc.cuda(), olens.cuda())
    assert search.route == "graph"
    _check_against_reference(hip, _model_reference(beam, lm_w))
    again = search.decode(enc.cuda(), olens.cuda())
    assert search.search.replayed and again == hip


def test_a_model_without_decoder_takes_the_one_launch_route():
    from tavsr.inference.timesync import BeamSearchTimeSync
    _, _, enc, olens = _oracle()
    search = BeamSearchTimeSync(_product(1.0), None, 5, 1.0, 0.0, 0.5)
    hip = search.decode(enc.cuda(), olens.cuda())
    assert search.route == "one_launch"
    _check_against_reference(hip, _model_reference(5, 0.0, decoder=False))


def test_speech2text_time_sync():
    """the reference's result tuples; with timestamps=True the fifth element; the token ids are those of decode() on model.encode"""
    from oracle.model import synth
    from tavsr.inference.beam_search import Speech2Text
    from tavsr.inference.timesync import BeamSearchTimeSync
    pm = _product(None, input_size=None)
    wav = 0.1 * synth((2, 24000), seed=21, kind="uniform")
    lens = torch.tensor([24000, 17600])
    wav[1, 17600:] = 0
    s2t = Speech2Text(pm, None, beam_size=5, ctc_weight=0.3, lm_weight=0.0, penalty=0.5, nbest=2, time_sync=True)
    assert isinstance(s2t.beam_search, BeamSearchTimeSync)
    res = s2t(wav.cuda(), lens.cuda())
    with torch.no_grad():
        enc, olens = pm.encode(wav.cuda(), lens.cuda())
    want = BeamSearchTimeSync(pm, None, 5, 0.3, 0.0, 0.5).decode(enc, olens, nbest=2)
    assert len(res) == 2 and all(1 <= len(r) <= 2 for r in res)
    for u in range(2):
        text, token, token_int, (ys, sc) = res[u][0]
        assert ys == want[u][0][0] and ys[0] == pm.sos and ys[-1] == pm.sos
        assert token_int == [t for t in ys[1:-1] if t != 0] and len(token) == len(token_int)
        assert text == "".join(token).replace("<space>", " ")
    timed = Speech2Text(pm, None, beam_size=5, ctc_weight=0.3, lm_weight=0.0, penalty=0.5, nbest=2, time_sync=True, timestamps=True)
    res_t = timed(wav.cuda(), lens.cuda())
    for u in range(2):
        assert len(res_t[u][0]) == 5 and res_t[u][0][:3] == res[u][0][:3]
        rec = res_t[u][0][4]
        assert rec is None or isinstance(rec, dict)
