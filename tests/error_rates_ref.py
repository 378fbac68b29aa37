"""Plain restatements for the error-rate tests: a Levenshtein distance vectorised over one lattice row with numpy, and the three
symbol-sequence builders of ``ErrorCalculator`` written from its host string code (tavsr/models/espnet_model.py)."""
from itertools import groupby

import numpy as np


def levenshtein(a, b) -> int:
    """unit-cost edit distance of two sequences of hashable symbols; row i from row i - 1 in three vector steps: the
    substitution and deletion candidates elementwise, the insertion chain cur[j] = min(cand[j], cur[j-1] + 1) as a running
    minimum of cand[j] - j."""
    sym = {}
    a = np.array([sym.setdefault(x, len(sym)) for x in a], dtype=np.int64)
    b = np.array([sym.setdefault(x, len(sym)) for x in b], dtype=np.int64)
    j = np.arange(len(b) + 1)
    prev = j.copy()
    for i, ca in enumerate(a, 1):
        cand = np.empty(len(b) + 1, dtype=np.int64)
        cand[0] = i
        cand[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != ca))
        prev = np.minimum.accumulate(cand - j) + j
    return int(prev[-1])


def split_words(cps, is_space):
    """``str.split()`` over code points and their whitespace flags: the maximal runs of unflagged code points, as tuples"""
    words, cur = [], []
    for c, s in zip(cps, is_space):
        if s:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        words.append(tuple(cur))
    return words


def ctc_chars(char_list, sym_space, sym_blank, y, ref):
    """(hypothesis, reference) character lists of ``ErrorCalculator.cer_ctc`` for one utterance"""
    drop = {-1, char_list.index(sym_blank)} | ({char_list.index(sym_space)} if sym_space in char_list else set())
    hyp = "".join(char_list[i] for i, _ in groupby(y) if i not in drop)
    tru = "".join(char_list[i] for i in ref if i not in drop)
    return list(hyp), list(tru)


def att_text(char_list, sym_space, sym_blank, y, ref):
    """(hypothesis, reference) strings of ``ErrorCalculator.__call__`` for one utterance"""
    ymax = ref.index(-1) if -1 in ref else len(ref)
    h = "".join(char_list[i] for i in y[:ymax]).replace(sym_space, " ").replace(sym_blank, "")
    r = "".join(char_list[i] for i in ref if i != -1).replace(sym_space, " ")
    return h, r


def att_chars(char_list, sym_space, sym_blank, y, ref):
    h, r = att_text(char_list, sym_space, sym_blank, y, ref)
    return list(h.replace(" ", "")), list(r.replace(" ", ""))


def att_words(char_list, sym_space, sym_blank, y, ref):
    h, r = att_text(char_list, sym_space, sym_blank, y, ref)
    return h.split(), r.split()


BUILDERS = {"ctc_chars": ctc_chars, "att_chars": att_chars, "att_words": att_words}


def counts(char_list, sym_space, sym_blank, ys_hat, ys_pad, mode):
    """(errs, ref_n) lists over the utterances, as ``ErrorCalculator.counts``"""
    errs, ref_n = [], []
    for y, ref in zip(ys_hat, ys_pad):
        h, r = BUILDERS[mode](char_list, sym_space, sym_blank, list(y), list(ref))
        errs.append(levenshtein(h, r) if (r or mode != "ctc_chars") else 0)
        ref_n.append(len(r))
    return errs, ref_n


# token lists of the tests: the shipped character inventory (helpers.TOKENS_EN), a BPE-like list with word-boundary pieces, <unk>,
# <sos/eos> and a token that holds a literal space, and the same pieces with the one-character word boundary as sym_space
TOKENS_BPE = ["<blank>", "<unk>", "<space>", "▁the", "▁a", "ing", "s", "▁", "new york", "é", "\U0010ffff", "t", "h", "<sos/eos>"]
TOKENS_BPE_SYMS = ("<space>", "<blank>")
TOKENS_UNDERBAR_SYMS = ("▁", "<blank>")
