"""Host-side helpers that turn a CTC forced alignment (``ops.ctc_align``: per-token frame spans and per-frame
log-probabilities) into token and word timestamps.  Plain Python on values already read from the device."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

Timed = Tuple[str, float, float, float]      # (token or word, start in seconds, end in seconds, confidence)


def token_times(tokens: Sequence[str], span, frame_lp, frame_seconds: float = 0.04) -> List[Timed]:
    """``span`` [>= len(tokens)][2] (first frame, last frame + 1) and ``frame_lp`` [frames] of one aligned hypothesis ->
    (token, start_s, end_s, conf) per token; conf = exp(mean frame_lp over the token's frames)."""
    out = []
    for tok, (b, e) in zip(tokens, span):
        b, e = int(b), int(e)
        if not 0 <= b < e:
            raise ValueError(f"token {tok!r} has no frames in the alignment: span ({b}, {e})")
        conf = math.exp(sum(float(v) for v in frame_lp[b:e]) / (e - b))
        out.append((tok, b * frame_seconds, e * frame_seconds, conf))
    return out


def word_times(timed_tokens: Sequence[Timed], space: str = "<space>") -> List[Timed]:
    """words = the runs of tokens between ``space`` tokens: (word, start of its first token, end of its last token, the
    minimum confidence of its tokens).  A leading, trailing or doubled ``space`` yields no empty word."""
    words, run = [], []

    def close():
        if run:
            words.append(("".join(t[0] for t in run), run[0][1], run[-1][2], min(t[3] for t in run)))
            run.clear()

    for t in timed_tokens:
        if t[0] == space:
            close()
        else:
            run.append(t)
    close()
    return words


def timestamp_record(tokens: Sequence[str], span, frame_lp, score: float, frame_seconds: float = 0.04,
                     space: str = "<space>") -> Optional[dict]:
    """the record ``Speech2Text(timestamps=True)`` attaches to a hypothesis, or None for one that CTC cannot emit
    (``score`` = -inf: the alignment was infeasible)"""
    if score == -math.inf:
        return None
    timed = token_times(tokens, span, frame_lp, frame_seconds)
    return {"tokens": timed, "words": word_times(timed, space), "score": float(score)}
