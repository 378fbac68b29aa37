"""GPU: the transducer beam searches ALSD and TSD (tavsr/inference/transducer.py, csrc/rnnt_search.hip) against the float64
restatement of espnet's two searches (tests/rnnt_search_ref.py).

Inputs.  ``TransducerDecoder(V, hidden_size=96, num_layers=2)`` and ``JointNetwork(V, 64, 96, joint_space_size=64)`` as torch
initialises them under the shape's seed, ``lin_out.weight`` scaled by ``gain`` and ``bias`` added to ``lin_out.bias[0]``, ten
utterances ``enc = 3 randn`` drawn under the same seed.  An untrained joint makes ALSD degenerate (every result at the maximum
length, near-tied lists, no merges); with the gain and the blank bias the lengths are mixed, equal prefixes merge and results of
several lengths compete.  (seed, gain, bias) per shape were chosen by running the float64 reference alone (``SHAPES``):

    (V, K, T)       seed gain bias   binding of 10: ALSD TSD(2) TSD(3)   merges: ALSD TSD(2) TSD(3)
    (7, 3, 10)         1  2.5  4.5                    10    10     10               6     75     83
    (41, 4, 12)        1  2.0  4.5                    10    10     10               3     31     31
    (70, 10, 8)        5  2.0  4.5                     9    10      8              15     96     96
    (1100, 4, 6)       5  2.5  4.0                     9    10     10               1      2      2

``test_inputs_meet_the_conditions`` asserts what the parity tests rely on, on the reference alone (it passes without the feature).
An utterance is *binding* when the reference's smallest decision margin is above 1e-4; parity is asked of binding utterances.

Scores.  The same search runs in fp32 with the CPU restatement; its largest |score - float64| over the compared hypotheses of the
binding utterances is what fp32 costs this computation, and the GPU may be four times as far from float64 (floor 1e-5 max(1,
|score|)).  GPU / CPU-fp32 ratio of that largest error, measured on an MI355X: in ``test_parity_with_the_float64_reference``'s
docstring."""
import functools
import os
import re

import pytest
import torch

import rnnt_ref as R
import rnnt_search_ref as S
from helpers import ROOT, TOKENS_EN

pytestmark = pytest.mark.gpu

U, HID, JOINT, DENC = 10, 96, 64, 64
SHAPES = {(7, 3, 10): (1, 2.5, 4.5), (41, 4, 12): (1, 2.0, 4.5), (70, 10, 8): (5, 2.0, 4.5), (1100, 4, 6): (5, 2.5, 4.0)}
SEARCHES = [("alsd", {}), ("tsd", {"max_sym_exp": 2}), ("tsd", {"max_sym_exp": 3})]
IDS = [f"{s}{kw.get('max_sym_exp', '')}" for s, kw in SEARCHES]


@functools.lru_cache(maxsize=None)
def _setup(shape):
    """(decoder, joint network, enc [U, T, DENC]) on the CPU; never modified"""
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    V, K, T = shape
    seed, gain, bias = SHAPES[shape]
    torch.manual_seed(seed)
    dec, jn = TransducerDecoder(V, hidden_size=HID, num_layers=2), JointNetwork(V, DENC, HID, joint_space_size=JOINT)
    with torch.no_grad():
        jn.lin_out.weight *= gain
        jn.lin_out.bias[0] += bias
    return dec.eval(), jn.eval(), torch.randn(U, T, DENC) * 3.0


def _ref_one(dec, jn, enc_u, K, search, kw, dtype=torch.float64, **more):
    """-> (hyps, merges, mingap, from_final) of one utterance"""
    _, emb, lay = R.decoder_params(dec, dtype)
    _, P = R.joint_params(jn, dtype)
    info = {}
    fn = S.alsd if search == "alsd" else S.tsd
    extra = dict(info=info) if search == "alsd" else {}
    return fn(enc_u.to(dtype), emb, lay, P, K, **kw, **more, **extra) + (info.get("from_final", True),)


@functools.lru_cache(maxsize=None)
def _reference(shape, which, dtype=torch.float64):
    dec, jn, enc = _setup(shape)
    search, kw = SEARCHES[which]
    return [_ref_one(dec, jn, enc[u], shape[1], search, kw, dtype) for u in range(U)]


@functools.lru_cache(maxsize=None)
def _cuda(shape):
    import copy
    dec, jn, enc = _setup(shape)
    return copy.deepcopy(dec).cuda().eval(), copy.deepcopy(jn).cuda().eval(), enc.cuda()


def _search(shape, which, **kw):
    from tavsr.inference.transducer import BeamSearchTransducer
    dec, jn, _ = _cuda(shape)
    search, conf = SEARCHES[which]
    return BeamSearchTransducer(dec, jn, beam_size=shape[1], search_type=search, **conf, **kw)


def _full(T):
    return torch.full((U,), T, dtype=torch.int64).cuda()


# ------------------------------------------------------------------------------------------------ 1. the inputs
@pytest.mark.parametrize("shape", list(SHAPES))
def test_inputs_meet_the_conditions(shape):
    """on the float64 reference alone: >= 80 % of the batch binding and merges > 0 for every search, ALSD results of two or more
    lengths in some utterance's final and not every best hypothesis at the maximum length; and, over the four shapes, a TSD best
    hypothesis of two or more labels (shape (7, 3, 10), max_sym_exp = 3)"""
    V, K, T = shape
    for which, (search, kw) in enumerate(SEARCHES):
        ref = _reference(shape, which)
        binding = sum(gap > S.BINDING for _, _, gap, _ in ref)
        merges = sum(m for _, m, _, _ in ref)
        print(f"    {shape} {IDS[which]}: binding {binding}/{U}, merges {merges}")
        assert binding >= 0.8 * U and merges > 0, (shape, IDS[which], binding, merges)
        if search == "alsd":
            finals = [hyps for hyps, _, _, from_final in ref if from_final]
            assert any(len({len(y) for y, _ in hyps}) >= 2 for hyps in finals)
            longest = min(50, T - 1) + 1                     # a result of `final` has at most min(u_max, T - 1) labels
            assert not all(len(hyps[0][0]) == longest for hyps in finals)
    two = [len(hyps[0][0]) - 1 >= 2 for s in SHAPES for w in (1, 2) for hyps, _, _, _ in _reference(s, w)]
    assert any(two)


# ------------------------------------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize("which", range(len(SEARCHES)), ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_with_the_float64_reference(shape, which):
    """binding utterances: the returned list equals the reference's token for token down to the first near-tied neighbours, and
    every compared score is within 4 x the CPU fp32 chain's largest error (floor 1e-5 max(1, |score|)).  The test prints the GPU's
    and the fp32 chain's largest error and their ratio per shape and search.  Measured on an MI355X, largest |score - float64|:

        (V, K, T)        ALSD: gpu   cpu-fp32 ratio    TSD (2 and 3 alike): gpu   cpu-fp32 ratio
        (7, 3, 10)          7.0e-6    4.8e-6  1.44                           1.4e-6    9.3e-7  1.48
        (41, 4, 12)         8.4e-6    5.4e-6  1.55                           2.0e-6    1.2e-6  1.65
        (70, 10, 8)         5.1e-6    4.1e-6  1.24                           2.5e-6    1.7e-6  1.42
        (1100, 4, 6)        6.4e-6    6.5e-6  0.99                           4.3e-6    2.9e-6  1.45"""
    V, K, T = shape
    _, _, enc = _cuda(shape)
    ref, f32 = _reference(shape, which), _reference(shape, which, torch.float32)
    out = _search(shape, which, nbest=10000).decode(enc, _full(T))
    e32, egpu, worst = 0.0, 0.0, []
    for u in range(U):
        hyps, _, gap, _ = ref[u]
        if gap <= S.BINDING:
            continue
        depth = S.parity_depth(hyps)
        assert [ys for ys, _ in out[u][:depth]] == [ys for ys, _ in hyps[:depth]], (u, out[u][:depth], hyps[:depth])
        cpu = {tuple(ys): sc for ys, sc in f32[u][0]}
        for (ys, sc), (_, got) in zip(hyps[:depth], out[u]):
            if tuple(ys) in cpu:
                e32 = max(e32, abs(cpu[tuple(ys)] - sc))
            egpu = max(egpu, abs(got - sc))
            worst.append((abs(got - sc), sc))
    print(f"    {shape} {IDS[which]}: gpu {egpu:.3e}   fp32-on-cpu {e32:.3e}   ratio {egpu / max(e32, 1e-30):.2f}")
    for err, sc in worst:
        assert err <= max(4.0 * e32, 1e-5 * max(1.0, abs(sc))), (err, e32, sc)


# ------------------------------------------------------------------------------------------------ 3. ragged batch
@pytest.mark.parametrize("which", range(len(SEARCHES)), ids=IDS)
def test_ragged_batch_equals_every_utterance_searched_alone(which):
    shape = (41, 4, 12)
    V, K, T = shape
    _, _, enc = _cuda(shape)
    lens = [T, 1, 5, 12, 3, 1, 7, 9, 2, 11]
    enc_p = enc.clone()
    for u, n in enumerate(lens):
        enc_p[u, n:] = float("nan")                         # frames past an utterance are never read
    search = _search(shape, which, nbest=5)
    out = search.decode(enc_p, torch.tensor(lens).cuda())
    assert all(len(o) >= 1 for o in out)
    for u, n in enumerate(lens):
        alone = search.decode(enc[u: u + 1, :n].contiguous(), torch.tensor([n]).cuda())[0]
        assert out[u] == alone, (u, n, out[u], alone)       # the lists and the bits of the scores
    # T_u = 1 against the reference: ALSD runs one step; the best result is the blank extension or one label
    dec, jn, enc_c = _setup(shape)
    search1 = _search(shape, which, nbest=10000)
    out1 = search1.decode(enc_p, torch.tensor(lens).cuda())
    for u in (1, 5):
        hyps, _, gap, _ = _ref_one(dec, jn, enc_c[u, :1], K, *SEARCHES[which])
        if gap > S.BINDING:
            depth = S.parity_depth(hyps)
            assert [ys for ys, _ in out1[u][:depth]] == [ys for ys, _ in hyps[:depth]]
            assert abs(out1[u][0][1] - hyps[0][1]) < 1e-4 * max(1.0, abs(hyps[0][1]))


# ------------------------------------------------------------------------------------------------ 4. graph and eager
@pytest.mark.parametrize("which", [0, 2], ids=[IDS[0], IDS[2]])
def test_graph_and_eager_routes_are_bit_equal_and_the_graph_is_kept(which):
    shape = (41, 4, 12)
    V, K, T = shape
    _, _, enc = _cuda(shape)
    search = _search(shape, which, nbest=10000)
    a = search.decode(enc, _full(T))
    graph = search._cap["graph"]
    assert graph is not None
    b = search.decode(enc.flip(0).contiguous(), _full(T))       # the same shape: the kept graph is replayed on new inputs
    assert search._cap["graph"] is graph and b == a[::-1]
    c = search.decode(enc[:3, :7].contiguous(), _full(7)[:3])  # another shape captures again
    assert search._cap["graph"] is not graph
    search.use_graph = False
    assert search.decode(enc, _full(T)) == a                    # eager: the same launches, the same bits
    assert search.decode(enc[:3, :7].contiguous(), _full(7)[:3]) == c
    one = search(enc[0])                                        # espnet's one-utterance call
    assert [(h.yseq, h.score) for h in one] == a[0]
    assert search.search_algorithm(enc[0])[0].yseq == a[0][0][0]


# ------------------------------------------------------------------------------------------------ 5. nbest and score_norm
@pytest.mark.parametrize("which", [0, 1], ids=IDS[:2])
def test_nbest_and_score_norm_follow_the_reference(which):
    shape = (7, 3, 10)
    V, K, T = shape
    dec, jn, enc_c = _setup(shape)
    _, _, enc = _cuda(shape)
    for score_norm in (True, False):
        out = _search(shape, which, nbest=3, score_norm=score_norm).decode(enc, _full(T))
        big = _search(shape, which, score_norm=score_norm).decode(enc, _full(T), nbest=10000)
        checked = 0
        for u in range(U):
            hyps, _, gap, from_final = _ref_one(dec, jn, enc_c[u], K, *SEARCHES[which], score_norm=score_norm)
            assert len(out[u]) == min(3, len(hyps)) and len(big[u]) == len(hyps)      # nbest above the list returns the list
            assert out[u] == big[u][:3]
            if gap > S.BINDING and from_final:
                depth = min(3, S.parity_depth(hyps, score_norm))
                assert [ys for ys, _ in out[u][:depth]] == [ys for ys, _ in hyps[:depth]], (score_norm, u)
                checked += 1
        assert checked >= 0.8 * U - 1


# ------------------------------------------------------------------------------------------------ 6. beam_size = 1
def test_beam_size_one_is_the_greedy_search_for_every_search_type():
    from tavsr.inference.transducer import BeamSearchTransducer
    import copy
    shape = (41, 4, 12)
    dec, jn, enc = _cuda(shape)
    jn = copy.deepcopy(jn)
    with torch.no_grad():
        jn.lin_out.bias[0] -= 4.0                           # (under the shape's blank bias the greedy search emits nothing)
    lens = torch.tensor([12, 1, 5, 12, 3, 1, 7, 9, 2, 11]).cuda()
    want = BeamSearchTransducer(dec, jn, beam_size=1).decode(enc, lens)
    assert any(len(ys) > 1 for ((ys, _),) in want)
    for kind in ("alsd", "tsd", "nsc", "maes"):
        assert BeamSearchTransducer(dec, jn, beam_size=1, search_type=kind, u_max=3, max_sym_exp=4).decode(enc, lens) == want


# ------------------------------------------------------------------------------------------------ 7. the row reduce alone
@pytest.mark.parametrize("V", [63, 64, 65, 1025])
def test_row_topk_vs_torch_float64(V):
    from tavsr import ops
    torch.manual_seed(V)
    N, K = 6, 5
    x = torch.randn(N, V) * 3.0
    x[1, [7, 3, 40, 11]] = x[1].max() + 1.0                 # planted ties above everything: ids 3, 7, 11, 40 in this order
    x[2, 0] = x[2].max() + 5.0                              # the blank is never a label, however large
    x[4, V - 1] = x[4, V - 2] = x[4].max() + 2.0            # a tie in the last lane / the last workgroup pass
    row_t = torch.tensor([0, 3, 0, -1, 2, 0], dtype=torch.int32).cuda()
    lpb = torch.full((N,), 7.0).cuda()
    topv, topi = torch.full((N, K), 7.0).cuda(), torch.full((N, K), -7, dtype=torch.int32).cuda()
    ops.rnnt_row_topk(x.cuda(), K, row_t, out=(lpb, topv, topi))
    lp = x.double().log_softmax(-1)
    for n in range(N):
        if n == 3:                                          # a skipped row is left untouched
            assert float(lpb[n]) == 7.0 and topv[n].tolist() == [7.0] * K and topi[n].tolist() == [-7] * K
            continue
        vals, ids, _ = S.topk_labels(lp[n], K)
        assert topi[n].tolist() == ids, (n, topi[n].tolist(), ids)
        assert float((topv[n].cpu().double() - vals).abs().max()) < 1e-5 and abs(float(lpb[n]) - float(lp[n, 0])) < 1e-5
    assert topi[1].tolist()[:4] == [3, 7, 11, 40] and topi[4].tolist()[:2] == [V - 2, V - 1] and 0 not in topi[2].tolist()
    lpb2, topv2, topi2 = ops.rnnt_row_topk(x.cuda(), K)     # no row_t: every row
    assert torch.equal(topi2[[0, 1, 2, 4, 5]], topi[[0, 1, 2, 4, 5]]) and torch.equal(topv2[[0, 1, 2, 4, 5]], topv[[0, 1, 2, 4, 5]])
    assert topi2[3].tolist() == S.topk_labels(lp[3], K)[1]


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_a_shape_that_does_not_fit_is_refused_before_any_launch():
    from tavsr import ops
    from tavsr.inference.transducer import BeamSearchTransducer
    assert ops.rnnt_search_ok("alsd", 10, 41, 100) and ops.rnnt_search_ok("tsd", 10, 5000, 100, max_sym_exp=3)
    assert ops.rnnt_search_ok("alsd", 64, 5000, 400) and ops.rnnt_search_ok("tsd", 64, 5000, 400, max_sym_exp=8)
    assert not ops.rnnt_search_ok("alsd", 65, 5000, 100) and not ops.rnnt_search_ok("tsd", 65, 5000, 100)
    assert not ops.rnnt_search_ok("alsd", 10, 10, 100) and not ops.rnnt_search_ok("tsd", 4, 41, 100, max_sym_exp=9)
    with pytest.raises(ValueError, match="beam <= 64"):
        ops.rnnt_search_ws("alsd", 65, 5000, 100)
    dec, jn, enc = _cuda((70, 10, 8))
    for kind in ("alsd", "tsd"):
        search = BeamSearchTransducer(dec, jn, beam_size=65, search_type=kind)
        with pytest.raises(ValueError, match="beam <= 64"):
            search.decode(enc, _full(8))
        assert search._cap is None                          # refused in front of every allocation and launch
    words, off = ops.rnnt_search_ws("alsd", 4, 41, 12)
    assert off["nodes"] == 1 + 4 * (12 + 11) and off["list"] == 4 * (12 + 11) and words > off["list_score"] + off["list"]
    words, off = ops.rnnt_search_ws("tsd", 4, 41, 12, max_sym_exp=3)
    assert off["nodes"] == 1 + 4 * 12 * 2 and off["list"] == 4 * 3


# ------------------------------------------------------------------------------------------------ 9. Speech2Text
@pytest.mark.parametrize("kind", ["alsd", "tsd"])
def test_speech2text_runs_the_beam_searches_of_a_transducer_model(kind):
    from tavsr.inference import Speech2Text
    from test_gpu_rnnt import _batch, _model
    model = _model(layers=1, hidden=96).cuda().eval()
    with torch.no_grad():
        model.joint_network.lin_out.weight *= 2.0
        model.joint_network.lin_out.bias[0] += 4.5
    speech, slens, _, _ = _batch()
    s2t = Speech2Text(model, beam_size=4, nbest=2, transducer_conf={"search_type": kind})
    assert s2t.beam_search_transducer.search_type == kind and s2t.beam_search_transducer.nbest == 2
    results = s2t(speech, slens)
    with torch.no_grad():
        enc, olens = model.encode(speech, slens)
    direct = s2t.beam_search_transducer.decode(enc, olens, nbest=2)
    assert len(results) == enc.shape[0]
    bound = 0
    for b, res in enumerate(results):
        assert 1 <= len(res) <= 2 and len(res) == len(direct[b])
        for r, (text, tokens, ids, (ys, score)) in enumerate(res):
            assert (ys, score) == direct[b][r] and ids == [t for t in ys[1:] if t != 0] and tokens == [TOKENS_EN[t] for t in ids]
            assert text == "".join(tokens).replace("<space>", " ")
        hyps, _, gap, _ = _ref_one(model.decoder, model.joint_network, enc[b, : int(olens[b])].cpu(), 4, kind, {})
        if gap > S.BINDING:
            depth = min(len(res), S.parity_depth(hyps))
            assert [r[3][0] for r in res[:depth]] == [ys for ys, _ in hyps[:depth]], (b, res, hyps[:2])
            bound += 1
    print(f"    {kind}: {bound}/{len(results)} utterances binding")


# ------------------------------------------------------------------------------------------------ 10. symbols
def test_the_search_symbols_are_declared_exported_and_bound():
    import ctypes
    from tavsr import _lib
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    declared = set(re.findall(r"\b(tavsr_rnnt_[a-z0-9_]+)\s*\(", hdr))
    want = {"tavsr_rnnt_search_ok", "tavsr_rnnt_search_ws", "tavsr_rnnt_search_ws_offset", "tavsr_rnnt_search_init", "tavsr_rnnt_search_z",
            "tavsr_rnnt_row_topk", "tavsr_rnnt_gather_state", "tavsr_rnnt_alsd_step", "tavsr_rnnt_tsd_step"}
    assert want <= declared
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in sorted(want):
        assert hasattr(raw, n), n
        assert n in _lib.PROTOTYPES and getattr(_lib.lib(), n).argtypes == _lib.PROTOTYPES[n][1], n
