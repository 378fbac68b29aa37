"""The host half of the beam search (tavsr/inference/search_host.py) against the oracle's own loop (oracle/beam_search.py:339-345:
``post_process`` + ``end_detect`` per utterance), on synthetic per-token records - no device, no model.

Records [steps, 3, U * K] (token, slot the hypothesis extended, score bits) as a captured step writes them: every finite slot of
token i + 1 extends a slot of token i that was finite, not <eos> and of the same utterance; about one slot in five ends with <eos>;
some slots are -inf; all scores differ.  The records run on for all 12 tokens of every utterance, as the device's do: the host must
ignore what lies behind an utterance's end."""
import numpy as np
import pytest
import torch

from oracle import beam_search as BS
from tavsr.inference.search_host import HostSearch, max_tokens

U, K, V, STEPS = 3, 4, 9, 12
SOS = EOS = V - 1
LENS = [12, 9, 5]          # frames per utterance: the per-utterance maxlen at maxlenratio 0

# (maxlenratio, score lost per token, {utterance: token at which its whole beam ends with <eos>}, stops [end_detect, running == 0, last],
#  tokens at which end_detect's condition holds under a token budget, where it does not apply)
# A loss of 6 per token puts what ends three tokens after the best ended hypothesis more than 10 (end_detect's D_end) below it: end
# detection fires as soon as three consecutive lengths have ended hypotheses.  A loss of 0.05 keeps all scores within 12 * 0.05 + 1
# of each other: it cannot fire.  The counts are what the oracle's loop reports for these records (seed 3), asserted so that a
# change of the generator cannot leave a way of stopping uncovered without a failure.
CASES = {
    "end_detection_fires": (0.0, 6.0, {}, [1, 1, 1], 0),
    "end_detection_silent": (0.0, 0.05, {1: 4}, [0, 2, 1], 0),
    "budget_of_7": (-7, 6.0, {2: 3}, [0, 1, 2], 0),
    "ratio_0.5": (0.5, 6.0, {0: 2}, [0, 1, 2], 0),
    # the records of the first case under a budget of 12 tokens: at two tokens end_detect's condition holds and must NOT stop the search
    "budget_of_12_ignores_end_detection": (-12, 6.0, {}, [0, 1, 2], 2),
}


def _records(seed, loss, all_eos):
    g = torch.Generator().manual_seed(seed)
    N = U * K
    tok = torch.zeros(STEPS, N, dtype=torch.int64)
    back = torch.zeros(STEPS, N, dtype=torch.int64)
    score = torch.full((STEPS, N), -float("inf"))
    parents = [[u * K] for u in range(U)]                       # token 0 extends the <sos> hypothesis in slot 0 of each utterance
    parent_score = torch.zeros(N)
    for i in range(STEPS):
        for u in range(U):
            if not parents[u]:
                continue
            for k in range(K):
                n = u * K + k
                if i > 0 and float(torch.rand((), generator=g)) < 0.15:       # an empty slot
                    continue
                p = parents[u][int(torch.randint(len(parents[u]), (), generator=g))]
                back[i, n] = p
                ends = all_eos.get(u) == i or float(torch.rand((), generator=g)) < 0.2
                tok[i, n] = EOS if ends else int(torch.randint(1, V - 1, (), generator=g))
                score[i, n] = parent_score[p] - loss - float(torch.rand((), generator=g))
        parents = [[n for n in range(u * K, (u + 1) * K) if bool(torch.isfinite(score[i, n])) and int(tok[i, n]) != EOS] for u in range(U)]
        parent_score = score[i].clone()
    finite = score[torch.isfinite(score)]
    assert finite.unique().numel() == finite.numel()
    rec = torch.stack([tok.to(torch.int32), back.to(torch.int32), score.view(torch.int32)], dim=1).contiguous()
    return rec


def _oracle_loop(rec, maxlenratio):
    """oracle/beam_search.py:330-346 per utterance, ``search`` replaced by the records' hypotheses of token i"""
    bs = BS.BatchBeamSearch({}, {}, K, V, SOS, EOS)
    np_rec = rec.numpy()
    score = rec[:, 2].view(torch.float32)
    retired = torch.zeros(STEPS, U * K, dtype=torch.bool)
    out, searched, stops, ignored = [], [], [0, 0, 0], 0
    for u, frames in enumerate(LENS):
        if maxlenratio == 0:                                    # oracle/beam_search.py:331-336
            maxlen = frames
        elif maxlenratio < 0:
            maxlen = -1 * int(maxlenratio)
        else:
            maxlen = max(1, int(maxlenratio * frames))
        ended, i_end = [], None
        for i in range(maxlen):
            slots = [n for n in range(u * K, (u + 1) * K) if bool(torch.isfinite(score[i, n]))]
            best = []
            for n in slots:
                toks, cur = [], n
                for t in range(i, -1, -1):
                    toks.append(int(np_rec[t, 0, cur]))
                    cur = int(np_rec[t, 1, cur])
                best.append(BS.Hypothesis(yseq=torch.tensor([SOS] + toks[::-1]), score=float(score[i, n])))
            n_ended = len(ended)
            running = bs.post_process(i, maxlen, best, ended)
            gone = {id(h) for h in ended[n_ended:]}
            for n, h in zip(slots, best):                       # (post_process of the last iteration replaces every hypothesis)
                retired[i, n] = i == maxlen - 1 or id(h) in gone
            i_end = i
            if maxlenratio == 0.0 and BS.end_detect(ended, i):
                stops[0] += 1
                break
            ignored += int(BS.end_detect(ended, i) and i < maxlen - 1)      # a token budget: end detection does not stop the search
            if len(running) == 0:
                stops[1 if i < maxlen - 1 else 2] += 1
                break
        retired[i_end, u * K:(u + 1) * K] = True                # the utterance has stopped: its whole beam is retired ...
        retired[i_end + 1:, u * K:(u + 1) * K] = True           # ... and stays so
        searched.append(i_end + 1)
        out.append([(h.yseq.tolist(), float(h.score)) for h in sorted(ended, key=lambda h: h.score, reverse=True)])
    return out, searched, retired, stops, ignored


@pytest.mark.parametrize("case", list(CASES))
def test_host_search_equals_the_oracle_loop_over_the_same_records(case):
    maxlenratio, loss, all_eos, want_stops, want_ignored = CASES[case]
    rec = _records(seed=3, loss=loss, all_eos=all_eos)
    want, searched, retired, stops, ignored = _oracle_loop(rec, maxlenratio)
    print(f"{case}: stops by [end detection, running == 0, last iteration] = {stops}, tokens searched {searched}, "
          f"ended {[len(w) for w in want]}, tokens at which a token budget ignores end detection: {ignored}")
    assert stops == want_stops and ignored == want_ignored       # the case covers what its name says
    host = HostSearch(float(maxlenratio), LENS, K, SOS, EOS)
    assert host.maxl == max_tokens(maxlenratio, LENS) and host.steps == max(host.maxl)
    for i in range(STEPS):                                      # (as decode() does: until no utterance searches any more)
        kill = host.step_from_records(rec, i)
        assert torch.equal(kill, retired[i]), (i, kill.view(U, K), retired[i].view(U, K))
        if not bool(host.active.any()):
            break
    assert i + 1 == max(searched)
    assert host.n_host.tolist() == searched
    assert host.nbest() == want
    assert host.nbest(2) == [w[:2] for w in want]


def test_every_way_an_utterance_stops_is_covered():
    total = np.sum([CASES[c][3] for c in CASES], axis=0)
    assert all(total >= 1), total
    assert CASES["end_detection_fires"][3][0] >= 1 and CASES["end_detection_silent"][3][0] == 0


def test_max_tokens_is_espnets_rule():
    assert max_tokens(0.0, LENS) == [12, 9, 5]
    assert max_tokens(-7, LENS) == [7, 7, 7]
    assert max_tokens(0.5, LENS) == [6, 4, 2]
    assert max_tokens(0.01, LENS) == [1, 1, 1]
