"""CPU: the fp64 restatement of espnet's BeamSearchTimeSync (tests/timesync_ref.py) - that it is a correct CTC prefix search, a
hand-written case with the repeat-token branch, a tie at the pre-beam's threshold - and the refusals of the product's class."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

from timesync_ref import lae, timesync_search


def _log_softmax(z):
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("seed", range(10))
def test_unpruned_search_gives_the_ctc_likelihood_of_every_prefix(seed):
    """C = V and a beam that prunes nothing (V = 3, T = 5: at most 2^0 + .. + 2^5 = 63 prefixes over {1, 2}): the CTC term of every
    finite-scored prefix is -ctc_loss(prefix) in fp64 - the search is a correct prefix search, not a plausible one"""
    V, T, sos = 3, 5, 2
    lpz = _log_softmax(np.random.RandomState(seed).standard_normal((T, V)))
    # (<sos> = 2 is an ordinary token: prefixes hold 1s and 2s)
    res = timesync_search(lpz, 400, sos, w_ctc=1.0, C=V)
    lp = torch.from_numpy(lpz).view(T, 1, V)
    seen = 0
    for toks, score in res.hyps:
        assert toks[0] == sos and toks[-1] == sos
        y = toks[1:-1]
        if score == -math.inf:
            continue
        if len(y) == 0:
            want = float(lpz[:, 0].sum())
        else:
            want = -float(torch.nn.functional.ctc_loss(lp, torch.tensor([y]), torch.tensor([T]), torch.tensor([len(y)]), blank=0,
                                                       reduction="sum", zero_infinity=False))
        assert abs(score - want) < 2e-15, (toks, score, want)
        seen += 1
    # every label sequence CTC can emit in 5 frames is there
    feasible = sum(1 for n in range(T + 1) for y in itertools.product((1, 2), repeat=n)
                   if n + sum(a == b for a, b in zip(y, y[1:])) <= T)
    assert seen == feasible


def test_three_frames_by_hand_with_the_repeat_branch():
    """V = 3 (blank, a = 1, <sos> = 2), K = 2, C = 3 (every token), w_ctc = 1, 3 frames, worked by hand:
    frame 0: (s) b, (s,a), (s,s): p_nb(s,s) = p0[s] + p_b(s) - the repeat branch: <sos> is an ordinary token and l[-1] of (s,)"""
    p = np.log(np.array([[0.6, 0.3, 0.1], [0.5, 0.4, 0.1], [0.2, 0.7, 0.1]]))
    res = timesync_search(p, 2, 2, w_ctc=1.0, C=3)
    # by hand, frame 0: dp[(s)] = (p0[s] + -inf, p0[b]) = (-inf, log .6); (s,a): (log .3, -inf); (s,s): (log .1, -inf); beam (s), (s,a)
    # frame 1 from (s) [pl = log .6] and (s,a) [pl = log .3, nb = log .3, b = -inf]:
    #   (s): b = .5 * .6 = .30; nb += p1[s] * p_nb(s) = 0                         -> .30
    #   (s,a): from (s): nb = .4 * .6 = .24; own repeat: .4 * .3 = .12; blank: b = .5 * .3 = .15     -> .51
    #   (s,s): nb = .1 * p_b(s) = .06, and it was expanded in frame 0 and fell off: b = .5 * .1 = .05, nb += .1 * .1 = .01   -> .12
    #   (s,a,a): nb = .4 * p_b(s,a) = 0; (s,a,s): .1 * .3 = .03
    # beam: (s,a) .51, (s) .30.  frame 2 from (s,a) [nb .36, b .15] and (s) [nb 0, b .30]:
    #   (s,a): blank .2 * .51 = .102; repeat .7 * .36 = .252; from (s): .7 * .30 = .21        -> .564
    #   (s): .2 * .30 = .06;  (s,a,a): .7 * .15 = .105;  (s,a,s): .1 * .51 = .051, + fell off in frame 1: b = .2 * .03, nb += .1 * .03 -> .060
    #   (s,s): .1 * .30 = .03, + fell off: b = .2 * .12 = .024, nb += .1 * .07 = .007 -> .061
    assert [h[0] for h in res.hyps] == [[2, 1, 2], [2, 1, 1, 2]]
    assert abs(res.hyps[0][1] - math.log(0.564)) < 1e-12 and abs(res.hyps[1][1] - math.log(0.105)) < 1e-12
    assert res.merges >= 2


def test_a_tie_at_the_threshold_keeps_every_tied_token():
    """C = 2 of V = 5, the second-largest value shared by three tokens: all of them are candidates, in token order"""
    p = np.log(np.array([[0.4, 0.15, 0.15, 0.15, 0.15], [0.4, 0.3, 0.1, 0.1, 0.1]]))
    p[0, 1:] = p[0, 1]
    res = timesync_search(p[:1], 4, 4, w_ctc=1.0, C=2)
    assert res.ncand_max == 5
    assert [h[0] for h in res.hyps] == [[4, 4], [4, 1, 4], [4, 2, 4], [4, 3, 4]]      # (4, 4, 4) has the same score and came last
    assert abs(res.hyps[1][1] - res.hyps[3][1]) == 0.0


def test_logaddexp_of_two_impossible_events():
    assert lae(-math.inf, -math.inf) == -math.inf and lae(-math.inf, -1.0) == -1.0 and abs(lae(0.0, 0.0) - math.log(2)) < 1e-15


def _model(ctc=True, V=41):
    return types.SimpleNamespace(ctc=object() if ctc else None, decoder=None, token_list=["t"] * V, sos=V - 1, eos=V - 1, blank_id=0)


def test_refusals_name_the_remedy():
    from tavsr.inference.timesync import BeamSearchTimeSync
    with pytest.raises(ValueError, match="without a CTC head.*time_sync=False"):
        BeamSearchTimeSync(_model(ctc=False), None, 10, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match=r"int\(1.5 \* beam_size\) = 45 tokens of a vocabulary of 41.*27"):
        BeamSearchTimeSync(_model(), None, 30, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="n-gram.*never.*reads it"):
        BeamSearchTimeSync(_model(), None, 10, 1.0, 0.0, 0.0, ngram=object())
    ok = BeamSearchTimeSync(_model(), None, 27, 1.0, 0.0, 0.0, maxlenratio=0.5, minlenratio=0.1)      # accepted and unused
    assert ok.search.C == 40 and not ok.has_dec and not ok.has_lm


def test_more_frames_than_the_scorers_take_keys_are_refused_before_any_launch():
    """with a scorer a prefix may reach T + 1 keys, tavsr_tree_attn_rows takes 1024: T = 1024 is refused up front (CPU tensors: nothing
    was launched), T = 1023 and a search with the CTC term alone pass the check"""
    from tavsr import ops
    from tavsr.inference.timesync import TimeSyncSearch
    assert ops.TREE_ROWS_MAX_KEYS == 1024
    scored = TimeSyncSearch(41, 40, 10, 0.3, 0.7, dec_fn=lambda rows, out: out)
    with pytest.raises(ValueError, match="1024 frames.*at most 1023 encoder frames"):
        scored.search(torch.zeros(1, 1024, 41), torch.tensor([1024]))
    scored.check_frames(1023)
    TimeSyncSearch(41, 40, 10, 1.0).check_frames(5000)


def test_speech2text_refuses_an_ngram_with_time_sync(tmp_path):
    from tavsr.inference.beam_search import Speech2Text
    m = _model()
    m.eval = lambda: m
    with pytest.raises(ValueError, match="n-gram"):
        Speech2Text(m, None, beam_size=5, ctc_weight=1.0, lm_weight=0.0, ngram_file=str(tmp_path / "lm.arpa"), time_sync=True)
