"""CTC forced alignment, host side: the float64 reference of tests/ctc_align_ref.py against brute force over every frame
labelling, the timestamp helpers of tavsr/utils/timestamps.py, and what Speech2Text / model.align refuse at construction."""
import argparse
import math

import numpy as np
import pytest

import ctc_align_ref as R

# (T, V, target): repeats, L = 0, tight, infeasible by one frame, a bad label, everything at T <= 6, V <= 4
TINY = [
    (1, 3, []), (1, 3, [2]), (3, 3, [1, 2]), (4, 3, [1, 1]), (5, 4, [3, 3, 1]), (6, 3, [1, 2, 1]), (6, 4, [2, 2, 2]),
    (6, 2, [1, 1, 1]), (5, 3, [2, 1, 2, 1, 2]), (2, 3, [1, 1]), (4, 3, [1, 1, 1]), (3, 3, [1, 2, 1, 2]), (4, 3, []),
    (6, 4, [1, 2, 3]), (5, 3, [1, 2, 2]),
]


@pytest.mark.parametrize("T,V,target", TINY)
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_brute_force(T, V, target, seed):
    rng = np.random.default_rng(100 * seed + T + 7 * V + len(target))
    lp = R.log_softmax(rng.standard_normal((T, V)))
    want = R.brute_force(lp, T, target)
    align, frame_lp, span, score, path = R.align_ref(lp, T, target)
    assert R.feasible(T, target, V) == (want > -np.inf)
    if want == -np.inf:
        assert score == -np.inf and (align == -1).all() and (frame_lp == 0).all() and (span == -1).all()
        return
    assert abs(score - want) < 1e-12
    assert R.collapse(align[:T]) == target
    assert abs(R.path_score(lp, align, T) - want) < 1e-12 and abs(frame_lp.sum() - want) < 1e-12
    assert np.array_equal(span, R.spans_of_align(align, T, target).reshape(len(target), 2))


def test_reference_shorter_utterance_and_padding():
    rng = np.random.default_rng(3)
    lp = R.log_softmax(rng.standard_normal((6, 4)))
    align, frame_lp, span, score, _ = R.align_ref(lp, 4, [1, 3], Lmax=4)
    assert abs(score - R.brute_force(lp[:4], 4, [1, 3])) < 1e-12
    assert (align[4:] == -1).all() and (frame_lp[4:] == 0).all() and (span[2:] == -1).all() and (span[:2] >= 0).all()
    assert R.align_ref(lp, 0, [])[3] == 0.0 and R.align_ref(lp, 0, [1])[3] == -np.inf
    assert R.align_ref(lp, 6, [4])[3] == -np.inf and R.align_ref(lp, 6, [0])[3] == -np.inf      # label >= V; label == blank


def test_reference_tie_rule():
    """all-zero logits: every path ties.  The end state is the last blank (S-2 does not beat it), and walking back the smaller
    move wins, so the path stays there for as long as that state was reachable: the labels come as early as possible"""
    align, _, span, score, path = R.align_ref(R.log_softmax(np.zeros((9, 5))), 9, [1, 2, 3])
    assert path == [1, 3, 5, 6, 6, 6, 6, 6, 6]
    assert align.tolist() == [1, 2, 3, 0, 0, 0, 0, 0, 0] and span.tolist() == [[0, 1], [1, 2], [2, 3]]
    assert abs(score - 9 * math.log(1 / 5)) < 1e-12


def test_planted_path_is_recovered():
    for seed, (T, L, V) in enumerate([(16, 7, 5), (17, 8, 41), (40, 15, 41)]):
        logits, target, path = R.planted(seed, T, L, V)
        for dtype in (np.float64, np.float32):
            got = R.align_ref(R.log_softmax(logits, dtype), T, target, dtype=dtype)
            assert got[4] == path


# ------------------------------------------------------------------------------------------------ timestamps.py
def test_token_and_word_times():
    from tavsr.utils.timestamps import timestamp_record, token_times, word_times
    tokens = ["<space>", "h", "i", "<space>", "<space>", "y", "o", "u", "<space>"]
    span = [[0, 1], [2, 4], [4, 5], [6, 7], [7, 8], [9, 10], [10, 13], [13, 14], [15, 16], [-1, -1]]
    frame_lp = [-0.1 * (t % 4) for t in range(16)]
    timed = token_times(tokens, span, frame_lp, 0.04)
    assert [t[0] for t in timed] == tokens
    assert timed[1][1] == pytest.approx(0.08) and timed[1][2] == pytest.approx(0.16)
    assert timed[1][3] == pytest.approx(math.exp((frame_lp[2] + frame_lp[3]) / 2))
    assert timed[6][3] == pytest.approx(math.exp(sum(frame_lp[10:13]) / 3))
    words = word_times(timed)
    assert [w[0] for w in words] == ["hi", "you"]      # leading, doubled and trailing <space>: no empty word
    assert words[0][1] == pytest.approx(0.08) and words[0][2] == pytest.approx(0.20)
    assert words[1][1] == pytest.approx(0.36) and words[1][2] == pytest.approx(0.56)
    assert words[0][3] == pytest.approx(min(timed[1][3], timed[2][3]))
    assert words[1][3] == pytest.approx(min(t[3] for t in timed[5:8]))
    assert word_times([]) == [] and word_times(timed[:1]) == []
    rec = timestamp_record(tokens, span, frame_lp, -3.5, 0.02)
    assert rec["score"] == -3.5 and rec["tokens"][1][2] == pytest.approx(0.08) and [w[0] for w in rec["words"]] == ["hi", "you"]
    assert timestamp_record(tokens, span, frame_lp, -math.inf) is None
    assert timestamp_record([], [], [0.0] * 4, -1.0) == {"tokens": [], "words": [], "score": -1.0}
    with pytest.raises(ValueError, match="no frames"):
        token_times(["a"], [[-1, -1]], frame_lp)


# ------------------------------------------------------------------------------------------------ construction
def _model(model_ctc_weight=None):
    from helpers import TOKENS_EN, asr_conf
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=1, dec_blocks=1)
    if model_ctc_weight is not None:
        conf["model_conf"]["ctc_weight"] = model_ctc_weight
    conf["token_list"] = TOKENS_EN
    return ASRTask.build_model(argparse.Namespace(**conf)).eval()


def test_timestamps_need_a_ctc_head():
    import torch
    from tavsr.inference.beam_search import Speech2Text
    att_only, hybrid = _model(0.0), _model()
    assert att_only.ctc is None
    with pytest.raises(ValueError, match="CTC head"):
        Speech2Text(att_only, None, beam_size=5, ctc_weight=0.0, lm_weight=0.0, timestamps=True)
    assert Speech2Text(att_only, None, beam_size=5, ctc_weight=0.0, lm_weight=0.0).timestamps is False
    with pytest.raises(ValueError, match="frame_seconds"):
        Speech2Text(hybrid, None, beam_size=5, ctc_weight=0.3, lm_weight=0.0, timestamps=True, frame_seconds=0.0)
    s2t = Speech2Text(hybrid, None, beam_size=5, ctc_weight=0.3, lm_weight=0.0, timestamps=True)
    assert s2t.timestamps is True and s2t.frame_seconds == 0.04
    with pytest.raises(ValueError, match="CTC head"):
        att_only.align(torch.zeros(1, 8, 80), torch.tensor([8]), torch.ones(1, 2, dtype=torch.int64), torch.tensor([2]))
