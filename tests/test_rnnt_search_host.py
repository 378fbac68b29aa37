"""CPU: the restatements of espnet's ALSD and TSD transducer searches (tests/rnnt_search_ref.py) against first principles - a
hypothesis's score is a sum over a SUBSET of its alignments, so it can never exceed the likelihood of ``rnnt_ref.rnnt_nll`` on
the same logits, and reaches it where the posterior is peaked - their small parts, and the argument handling of
``BeamSearchTransducer`` and ``Speech2Text`` for the two searches (the last two tests fail without the feature)."""
import argparse
import math

import pytest
import torch

import rnnt_ref as R
import rnnt_search_ref as S
from test_rnnt_host import rnnt_conf


def _net(V=7, H=32, J=24, De=16, seed=3, gain=3.0, bias=4.0):
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    torch.manual_seed(seed)
    dec, jn = TransducerDecoder(V, hidden_size=H, num_layers=2), JointNetwork(V, De, H, joint_space_size=J)
    with torch.no_grad():
        jn.lin_out.weight *= gain
        jn.lin_out.bias[0] += bias
    _, emb, lay = R.decoder_params(dec)
    _, P = R.joint_params(jn)
    return emb, lay, P


def _searches():
    """(name, search, keywords, info): ``info["from_final"]`` is False where ALSD returned its unfinished beam"""
    a, b = {}, {}
    return [("alsd", S.alsd, dict(info=a), a), ("alsd_u2", S.alsd, dict(u_max=2, info=b), b), ("tsd2", S.tsd, dict(max_sym_exp=2), {}),
            ("tsd3", S.tsd, dict(max_sym_exp=3), {})]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_no_hypothesis_scores_above_the_likelihood_of_all_its_alignments(seed):
    emb, lay, P = _net(seed=3 + seed, gain=2.0, bias=4.5)
    torch.manual_seed(40 + seed)
    enc = torch.randn(7, 16, dtype=torch.float64) * 3.0
    merged = 0
    for name, fn, kw, info in _searches():
        hyps, merges, gap = fn(enc, emb, lay, P, 3, **kw)
        merged += merges
        assert info.get("from_final", True), name      # every result is a finished hypothesis: all T frames and the last blank
        assert hyps and gap >= 0.0 and all(y[0] == 0 and all(0 < t < 7 for t in y[1:]) for y, _ in hyps)
        assert len({tuple(y) for y, _ in hyps}) == len(hyps), name      # equal prefixes were merged, not listed twice
        for y, score in hyps:
            ll = -S.nll_of(enc, emb, lay, P, y)
            assert score <= ll + 1e-9, (name, y, score, ll)
    assert merged > 0      # logaddexp merges happened: double counting would have broken the bound above


def test_peaked_posterior_gives_the_likelihood_itself():
    """lin_out scaled up (x 60, blank bias + 45) until one path carries the mass: the best hypothesis' score is the likelihood to
    1e-6.  Seed 18 is one where the peaked path leaves every frame again (an untrained prediction network can prefer a label at
    every depth, and ALSD then never reaches the last frame): the best results have 5, 2, 1 and 2 labels."""
    emb, lay, P = _net(seed=18, gain=60.0, bias=45.0)
    torch.manual_seed(50)
    enc = torch.randn(6, 16, dtype=torch.float64) * 3.0
    for name, fn, kw, info in _searches():
        hyps, _, _ = fn(enc, emb, lay, P, 3, score_norm=False, **kw)
        assert info.get("from_final", True), name
        y, score = hyps[0]
        ll = -S.nll_of(enc, emb, lay, P, y)
        assert len(y) > 1 and abs(score - ll) < 1e-6, (name, y, score, ll)


def test_alsd_with_one_frame_runs_one_step():
    emb, lay, P = _net()
    torch.manual_seed(7)
    enc = torch.randn(1, 16, dtype=torch.float64) * 3.0
    hyps, merges, _ = S.alsd(enc, emb, lay, P, 3)
    net = S.Net(enc, emb, lay, P)
    assert hyps == [([0], float(net.logp(0, (0,))[0]))] and merges == 0      # u_max = min(50, T - 1) = 0: i = 0 only
    hyps, _, _ = S.tsd(enc, emb, lay, P, 3)
    assert hyps[0][0] in ([0], [0, hyps[0][0][-1]]) and len(hyps) == 3


def test_recombine_keeps_the_place_of_the_first_occurrence():
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    out, merges = S.recombine([(t(-1.0), (0, 1)), (t(-2.0), (0, 2)), (t(-3.0), (0, 1)), (t(-4.0), (0, 3)), (t(-5.0), (0, 2))])
    assert [y for _, y in out] == [(0, 1), (0, 2), (0, 3)] and merges == 2
    assert abs(float(out[0][0]) - math.log(math.exp(-1.0) + math.exp(-3.0))) < 1e-12
    assert abs(float(out[1][0]) - math.log(math.exp(-2.0) + math.exp(-5.0))) < 1e-12 and float(out[2][0]) == -4.0
    kept, gap = S.best([(t(-1.0), "a"), (t(-0.5), "b"), (t(-1.0), "c"), (t(-3.0), "d")], 3)
    assert [y for _, y in kept] == ["b", "a", "c"] and gap == 2.0      # stable: "a" stays in front of its equal "c"
    vals, ids, gap = S.topk_labels(torch.tensor([9.0, 1.0, 3.0, 3.0, 0.0, 3.0]), 2)
    assert ids == [2, 3] and vals.tolist() == [3.0, 3.0] and gap == 0.0      # blank is not a label; the lower id first among equals


def test_sort_nbest_under_both_score_norm_values():
    from tavsr.inference.transducer import sort_nbest
    hyps = [(-4.0, (0, 5, 6, 7)), (-1.5, (0,)), (-2.0, (0, 3)), (-1.5, (0, 9))]      # keys: -1.0, -1.5, -1.0, -0.75 / the scores
    out, gap = S.sort_nbest(hyps, True)
    assert [y for _, y in out] == [(0, 9), (0, 5, 6, 7), (0, 3), (0,)] and abs(gap - 0.25) < 1e-12      # stable among the -1.0 keys
    assert [s for s, _ in out] == [-1.5, -4.0, -2.0, -1.5]                                              # the score stays un-normalised
    out, gap = S.sort_nbest(hyps, False, nbest=3)
    assert [y for _, y in out] == [(0,), (0, 9), (0, 3)] and gap == 0.0
    # the product's host-side sort is the same function of (yseq, score)
    mine = [(list(y), s) for s, y in hyps]
    assert [tuple(y) for y, _ in sort_nbest(mine, True, 10)] == [(0, 9), (0, 5, 6, 7), (0, 3), (0,)]
    assert [tuple(y) for y, _ in sort_nbest(mine, False, 3)] == [(0,), (0, 9), (0, 3)]
    assert S.parity_depth([([0, 1], -1.0), ([0], -0.6), ([0, 2], -1.20001), ([0, 3], -2.0)]) == 1      # keys -0.5, -0.6, -0.600005, -1.0
    assert S.parity_depth([([0, 1], -1.0), ([0], -0.6)]) == 2 and S.parity_depth([([0], -1.0), ([0, 1], -2.0)]) == 1


def test_constructor_takes_the_two_built_searches_and_refuses_the_rest():
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    from tavsr.inference.transducer import BeamSearchTransducer
    dec, jn = TransducerDecoder(11, hidden_size=32, num_layers=2), JointNetwork(11, 16, 32, joint_space_size=24)
    a = BeamSearchTransducer(dec, jn, beam_size=4, search_type="alsd", u_max=7, score_norm=False, nbest=3)
    assert a.search_algorithm == a.align_length_sync_decoding and (a.u_max, a.score_norm, a.nbest, a.beam_size) == (7, False, 3, 4)
    t = BeamSearchTransducer(dec, jn, beam_size=4, search_type="tsd", max_sym_exp=3, nstep=2, prefix_alpha=2, expansion_gamma=1.0,
                             expansion_beta=1)
    assert t.search_algorithm == t.time_sync_decoding and t.max_sym_exp == 3 and t.score_norm is True
    for kind in ("default", "nsc", "maes"):
        with pytest.raises(ValueError, match="beam_size=1") as err:
            BeamSearchTransducer(dec, jn, beam_size=4, search_type=kind)
        assert "alsd" in str(err.value) and "tsd" in str(err.value)
        g = BeamSearchTransducer(dec, jn, beam_size=1, search_type=kind)
        assert g.search_algorithm == g.greedy_search
    for kind in ("alsd", "tsd"):
        g = BeamSearchTransducer(dec, jn, beam_size=1, search_type=kind)      # beam_size = 1 is the greedy search for every type
        assert g.search_algorithm == g.greedy_search
        with pytest.raises(ValueError, match="lm"):
            BeamSearchTransducer(dec, jn, beam_size=4, search_type=kind, lm=object())
    with pytest.raises(ValueError, match="search_type"):
        BeamSearchTransducer(dec, jn, beam_size=4, search_type="bogus")


def test_speech2text_passes_transducer_conf_to_the_search():
    from tavsr.inference import Speech2Text
    from tavsr.tasks.asr import ASRTask
    import tavsr.inference
    assert tavsr.inference.__all__ == ["Speech2Text", "Speech2TextMaskCTC"]
    model = ASRTask.build_model(argparse.Namespace(**rnnt_conf()))
    s2t = Speech2Text(model, beam_size=4, nbest=2, transducer_conf={"search_type": "tsd", "max_sym_exp": 3, "score_norm": False})
    bs = s2t.beam_search_transducer
    assert bs is s2t.beam_search and (bs.search_type, bs.max_sym_exp, bs.score_norm, bs.nbest, bs.beam_size) == ("tsd", 3, False, 2, 4)
    bs = Speech2Text(model, beam_size=4, transducer_conf={"search_type": "alsd", "u_max": 9}).beam_search_transducer
    assert (bs.search_type, bs.u_max, bs.nbest) == ("alsd", 9, 1) and bs.search_algorithm == bs.align_length_sync_decoding
    with pytest.raises(ValueError, match="beam_size=1"):
        Speech2Text(model, beam_size=4, transducer_conf={"search_type": "maes"})
    for kw in (dict(lm=torch.nn.Linear(1, 1)), dict(ngram_file="x.arpa"), dict(time_sync=True)):      # the refusals stay
        with pytest.raises(ValueError, match="transducer"):
            Speech2Text(model, beam_size=4, transducer_conf={"search_type": "alsd"}, **kw)
    # a model without a transducer decoder ignores the keyword
    from helpers import asr_conf
    plain = ASRTask.build_model(argparse.Namespace(**asr_conf(num_blocks=1)))
    assert Speech2Text(plain, beam_size=2, transducer_conf={"search_type": "alsd"}).beam_search_transducer is None
