"""N-gram language model for the beam search: an ARPA file as device-resident tables (``ops.ngram_score``, csrc/ngram.hip).

The reference builds espnet's ``NgramFullScorer`` / ``NgramPartScorer`` over a KenLM model (src/inference/avsr_inference.py:166-178)
and espnet scores on the host, one ``kenlm.BaseScore`` call per token and hypothesis.  Here the file is parsed once, in Python,
into a forward trie the kernel walks; ``kenlm`` is not needed.

Semantics (written from espnet 202402's espnet/nets/scorers/ngram.py and KenLM's documented behaviour; neither can be imported here,
so they are PARITY UNPINNED in the sense of oracle/leaves.py - the product is compared against tests/ngram_ref.py, a float64
restatement of this text):

* For a hypothesis ``y = [sos, t1 .. tm]`` the context is the word sequence ``<s>, word(t1) .. word(tm)``, cut to its last
  ``order - 1`` words.  Position 0 is always ``<s>``, whatever ``token_list[sos]`` says (espnet starts from the null context and
  scores ``"<s>"`` first).
* The score of candidate ``v`` is standard backoff over that context, from the longest suffix to the shortest: if the n-gram
  (suffix, word(v)) is listed, its log10 p plus the backoffs gathered so far; otherwise the suffix's backoff is added - 0 when the
  suffix itself is not listed - and the suffix loses its oldest word.  The unigram level always ends the chain.
* The value is the file's log10 number, NOT converted to natural log (espnet adds ``BaseScore``'s return value as it is).
* Nothing is added when a hypothesis ends (``final_score`` is 0), and the scorer's state is the hypothesis' own token history:
  nothing is carried or re-ordered by the beam update.

Table layout: include/tavsr.h at ``tavsr_ngram_score`` - one numbering of all n-grams (unigrams first, node = word id; then the
bigrams sorted by (parent, word); ...), ``word`` / ``logp`` / ``backoff`` per node, ``child_begin`` in CSR form; int32 indices, fp32
values.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from .._lib import ENUMS

MAX_ORDER = ENUMS["TAVSR_NGRAM_MAX_ORDER"]      # the kernel keeps one LDS slot per context word
UNK_LOGP = -100.0                               # KenLM's log10 p of an unknown word when the model lists no <unk>


def parse_arpa(path) -> List[List[Tuple[Tuple[str, ...], float, float, int]]]:
    """ARPA text -> per order k = 1 .. n the list of (words, log10 p, log10 backoff, line number).  ``\\data\\`` with ``ngram k=n``
    counts, sections ``\\k-grams:`` of lines ``log10p<TAB>w1 .. wk[<TAB>backoff]`` (a missing backoff is 0), ``\\end\\``.
    Every refusal is a ValueError that names the line."""
    with open(path, encoding="utf-8") as f:
        lines = f.read().split("\n")
    where = lambda no: f"{path}:{no}"
    counts, sections = {}, []
    state, k, cur, head_no = "start", 0, None, 0
    ended = False
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if not line:
            continue
        if state == "start":
            if line != "\\data\\":
                raise ValueError(f"{where(no)}: expected \\data\\, found {line!r}")
            state = "counts"
            continue
        if line.startswith("\\"):
            if state == "counts":
                order = max(counts, default=0)
                if order == 0 or sorted(counts) != list(range(1, order + 1)):
                    raise ValueError(f"{where(no)}: the header lists the orders {sorted(counts)}: an ARPA model has orders 1 .. n, n >= 1")
                if order > MAX_ORDER:
                    raise ValueError(f"{where(no)}: order {order} is above the maximum of {MAX_ORDER} (TAVSR_NGRAM_MAX_ORDER)")
            elif len(cur) != counts[k]:
                raise ValueError(f"{where(head_no)}: section \\{k}-grams: has {len(cur)} lines, the header says ngram {k}={counts[k]}")
            if line == "\\end\\":
                if k != max(counts):
                    raise ValueError(f"{where(no)}: \\end\\ after {k} of {max(counts)} sections")
                ended = True
                break
            if line != f"\\{k + 1}-grams:" or k + 1 not in counts:
                raise ValueError(f"{where(no)}: expected \\{k + 1}-grams: or \\end\\, found {line!r}")
            state, k, cur, head_no = "grams", k + 1, [], no
            sections.append(cur)
            continue
        if state == "counts":
            head = line.replace(" ", "")
            try:
                assert head.startswith("ngram")
                kk, cnt = (int(x) for x in head[len("ngram"):].split("="))
            except (AssertionError, ValueError):
                raise ValueError(f"{where(no)}: expected `ngram k=n`, found {line!r}") from None
            if kk < 1 or cnt < 0 or kk in counts:
                raise ValueError(f"{where(no)}: bad header line {line!r}" + (": order 0" if kk == 0 else ""))
            counts[kk] = cnt
            continue
        fields = line.split()
        if len(fields) not in (k + 1, k + 2):
            raise ValueError(f"{where(no)}: a {k}-gram line has {k + 1} or {k + 2} fields, found {len(fields)}: {line!r}")
        try:
            lp = float(fields[0])
            bo = float(fields[k + 1]) if len(fields) == k + 2 else 0.0
        except ValueError:
            raise ValueError(f"{where(no)}: non-numeric field in {line!r}") from None
        if not (np.isfinite(lp) and np.isfinite(bo)):
            raise ValueError(f"{where(no)}: non-finite value in {line!r}")
        cur.append((tuple(fields[1:k + 1]), lp, bo, no))
    if not ended:
        raise ValueError(f"{path}:{len(lines)}: no \\end\\" if state != "start" else f"{path}:1: no \\data\\ header")
    return sections


class NgramLM:
    """the tables of one ARPA model on one device, and the map from the model's token ids to the ARPA's words"""

    def __init__(self, sections, token_list: Sequence[str], device="cuda", name="<arpa>"):
        self.order = len(sections)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"{name}: order {self.order} outside 1 .. {MAX_ORDER}")
        where = lambda no: f"{name}:{no}"
        vocab = {}
        for words, _, _, no in sections[0]:
            if words[0] in vocab:
                raise ValueError(f"{where(no)}: {words[0]!r} is listed twice")
            vocab[words[0]] = len(vocab)
        self.n_unigrams = len(vocab)
        if self.n_unigrams == 0:
            raise ValueError(f"{name}: no unigrams")
        word = [np.arange(self.n_unigrams, dtype=np.int64)]
        logp = [np.array([g[1] for g in sections[0]], dtype=np.float64)]
        backoff = [np.array([g[2] for g in sections[0]], dtype=np.float64)]
        child_begin = []
        node_of = {(w,): i for w, i in vocab.items()}       # the previous level's n-grams -> node
        base = self.n_unigrams                                # first node of the level being built
        for k in range(2, self.order + 1):
            grams = sections[k - 1]
            parent = np.empty(len(grams), dtype=np.int64)
            last = np.empty(len(grams), dtype=np.int64)
            for g, (words, _, _, no) in enumerate(grams):
                p = node_of.get(words[:-1])
                if p is None:
                    raise ValueError(f"{where(no)}: the prefix {' '.join(words[:-1])!r} of this {k}-gram is not among the {k - 1}-grams")
                w = vocab.get(words[-1])
                if w is None:
                    raise ValueError(f"{where(no)}: the word {words[-1]!r} is not among the unigrams")
                parent[g], last[g] = p, w
            key = parent * self.n_unigrams + last
            perm = np.argsort(key, kind="stable")
            dup = np.nonzero(np.diff(key[perm]) == 0)[0]
            if dup.size:
                raise ValueError(f"{where(grams[int(perm[dup[0] + 1])][3])}: this {k}-gram is listed twice")
            word.append(last[perm])
            logp.append(np.array([grams[g][1] for g in perm], dtype=np.float64))
            backoff.append(np.array([grams[g][2] for g in perm], dtype=np.float64))
            # children of the previous level's nodes (numbered first .. base - 1): counts -> CSR
            first = base - len(word[-2])
            cnt = np.bincount(parent[perm] - first, minlength=len(word[-2]))
            child_begin.append(base + np.concatenate([[0], np.cumsum(cnt)[:-1]]))
            node_of = {grams[g][0]: base + r for r, g in enumerate(perm.tolist())}
            base += len(grams)
        self.n_nodes = base
        if self.n_nodes >= 2 ** 31 - 1:
            raise ValueError(f"{name}: {self.n_nodes} n-grams do not fit int32 indices")
        # the last level has no children: empty ranges at the end of the numbering
        child_begin.append(np.full(len(word[-1]) + 1, self.n_nodes, dtype=np.int64))
        # Token id -> word id, as espnet's Ngrambase.__init__: the word of token i is token_list[i] with "<eos>" replaced by "</s>"; a
        # word the ARPA does not list is "<unk>"; without "<unk>" in the ARPA such a token has no word (-1) and scores UNK_LOGP.
        # QUIRK, kept on purpose: an espnet2 token list ends in "<sos/eos>", which is not the string "<eos>", so the id of <sos/eos>
        # scores as <unk> - exactly as under espnet.  (Position 0 of a hypothesis is <s> regardless: see the module docstring.)
        unk = vocab.get("<unk>", -1)
        wmap = [vocab.get("</s>" if t == "<eos>" else t, unk) for t in token_list]
        self.bos_word = vocab.get("<s>", -1)
        self.unk_logp = UNK_LOGP
        self.words = list(vocab)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(np.int32))).to(device)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(np.float32))).to(device)
        self.word, self.child_begin = i32(word), i32(child_begin)
        self.logp, self.backoff = f32(logp), f32(backoff)
        self.word_map = torch.tensor(wmap, dtype=torch.int32).to(device)
        assert self.word.numel() == self.n_nodes and self.child_begin.numel() == self.n_nodes + 1

    @classmethod
    def from_arpa(cls, path, token_list: Sequence[str], device="cuda") -> "NgramLM":
        return cls(parse_arpa(path), token_list, device, name=str(path))

    @property
    def device(self):
        return self.word.device

    def to(self, device) -> "NgramLM":
        for n in ("word", "child_begin", "logp", "backoff", "word_map"):
            setattr(self, n, getattr(self, n).to(device))
        return self
