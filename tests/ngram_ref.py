"""Host reference of the n-gram scorer (tavsr/lm/ngram.py, tavsr_ngram_score): a float64, dict-based restatement of the ARPA
format and of the scoring semantics, a generator of small proper backoff models, and the scorer objects the oracle's beam search
takes.  Nothing here imports the product.

Semantics restated (espnet 202402 espnet/nets/scorers/ngram.py over KenLM; parity unpinned, see the product module's docstring):
the context of a hypothesis [sos, t1 .. tm] is <s>, word(t1) .. word(tm) cut to its last order - 1 words; the score of a word is
standard backoff from the longest context suffix down to the unigram, in log10; a suffix that is not listed contributes backoff 0;
word(token i) = token_list[i] with "<eos>" -> "</s>", unlisted words -> "<unk>", and -100 at the unigram level where the model has
no "<unk>"."""
import collections
import math

import numpy as np

UNK_LOGP = -100.0


def parse_arpa(path):
    """-> [ {words tuple: (log10 p, log10 backoff)} for k = 1 .. n ]; a plain reader for well-formed files (the product's parser is
    the one that refuses)"""
    grams, cur = [], None
    for line in open(path, encoding="utf-8"):
        line = line.strip()
        if not line or line == "\\data\\" or line.startswith("ngram "):
            continue
        if line == "\\end\\":
            break
        if line.startswith("\\"):
            cur = {}
            grams.append(cur)
            continue
        f = line.split()
        k = len(grams)
        cur[tuple(f[1:k + 1])] = (float(f[0]), float(f[k + 1]) if len(f) == k + 2 else 0.0)
    return grams


class RefNgram:
    def __init__(self, path, token_list):
        self.grams = parse_arpa(path)
        self.order = len(self.grams)
        self.token_list = list(token_list)
        listed = {w[0] for w in self.grams[0]}
        self.has_unk = "<unk>" in listed
        # token -> word (None: no word at all)
        self.word_of = []
        for t in self.token_list:
            w = "</s>" if t == "<eos>" else t
            self.word_of.append(w if w in listed else ("<unk>" if self.has_unk else None))
        # context tuple -> the words that continue it, in the order of the unigram section (the product numbers its words by it)
        rank = {w[0]: i for i, w in enumerate(self.grams[0])}
        self.children = collections.defaultdict(list)
        for k in range(1, self.order):
            for g in self.grams[k]:
                self.children[g[:-1]].append(g[-1])
        for kids in self.children.values():
            kids.sort(key=rank.__getitem__)

    def context_words(self, tokens):
        """tokens = [sos, t1 .. tm] -> the context's words (None for a token without word), cut to order - 1"""
        words = ["<s>"] + [self.word_of[t] for t in tokens[1:]]
        return tuple(words[len(words) - min(len(words), self.order - 1):])

    def trace(self, ctx, w):
        """backoff chain of word ``w`` (None: a token without word) behind context ``ctx`` -> (log10 score, events): events is a list
        of (suffix length j, listed?, hit?, number of children, position of the hit among them or -1) from the longest suffix down,
        ending with the level that hit (j = 0: the unigram level)"""
        acc, events = 0.0, []
        for j in range(len(ctx), 0, -1):
            suf = ctx[len(ctx) - j:]
            if None in suf or suf not in self.grams[j - 1]:
                events.append((j, False, False, 0, -1))
                continue
            kids = self.children.get(suf, ())
            hit = w is not None and suf + (w,) in self.grams[j]
            events.append((j, True, hit, len(kids), kids.index(w) if hit else -1))
            if hit:
                return self.grams[j][suf + (w,)][0] + acc, events
            acc += self.grams[j - 1][suf][1]
        events.append((0, True, True, len(self.grams[0]), -1))
        return (self.grams[0][(w,)][0] if w is not None else UNK_LOGP) + acc, events

    def score_words(self, ctx, words):
        return np.array([self.trace(tuple(ctx), w)[0] for w in words], dtype=np.float64)

    def score(self, tokens):
        """[sos, t1 .. tm] -> float64 [V]: log10 score of every token"""
        ctx = self.context_words(list(tokens))
        return np.array([self.trace(ctx, w)[0] for w in self.word_of], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ generated models
def counts_from_sentences(sentences, order):
    """k-gram counts, k = 1 .. order, of sentences wrapped in <s> .. </s> (the unigram <s> is not counted: it is never predicted)"""
    counts = [collections.Counter() for _ in range(order)]
    for s in sentences:
        ws = ["<s>"] + list(s) + ["</s>"]
        for k in range(1, order + 1):
            for a in range(len(ws) - k + 1):
                g = tuple(ws[a:a + k])
                if g[-1] != "<s>":
                    counts[k - 1][g] += 1
    return counts


def random_sentences(words, n_sent, seed, max_len=8, skew=1.3):
    """sentences over ``words`` with a Zipf-like unigram distribution (a few frequent words give wide child ranges)"""
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, len(words) + 1) ** skew
    p /= p.sum()
    return [[words[i] for i in rng.choice(len(words), size=rng.randint(1, max_len + 1), p=p)] for _ in range(n_sent)]


def write_arpa(path, sentences, order, words, discount=0.6, with_unk=True):
    """Interpolated absolute discounting in float64, written in backoff form.  Vocabulary = ``words`` + </s> (+ <unk>); <s> is listed
    with log10 p = -99 as ARPA files do.
        p_1(w)       = max(c(w) - D, 0) / c(.) + D N1+(.) / c(.) / |vocabulary|
        p_k(w | ctx) = max(c(ctx w) - D, 0) / c(ctx .) + g(ctx) p_{k-1}(w | ctx[1:]),   g(ctx) = D N1+(ctx .) / c(ctx .)
    An n-gram is listed when its count is positive (every unigram of the vocabulary is listed); the backoff of a listed context is
    log10 g(ctx), and 0 for an n-gram that never continues; the highest order has no backoff column.  For an unlisted (ctx, w) the
    model's value is g(ctx) p_{k-1}(w | ctx[1:]) - what the backoff chain computes - so every conditional distribution sums to 1
    over the vocabulary (plus 1e-99 for <s>), for contexts that never occurred too."""
    vocab = list(words) + ["</s>"] + (["<unk>"] if with_unk else [])
    counts = counts_from_sentences(sentences, order)
    ctx_total = [collections.Counter() for _ in range(order)]      # [k - 1][ctx] = sum_w c(ctx w), ctx of length k - 1
    ctx_types = [collections.Counter() for _ in range(order)]
    for k in range(order):
        for g, c in counts[k].items():
            ctx_total[k][g[:-1]] += c
            ctx_types[k][g[:-1]] += 1

    def gamma(ctx):
        k = len(ctx)
        return discount * ctx_types[k][ctx] / ctx_total[k][ctx]

    def prob(ctx, w):
        """the model's p(w | ctx), by its definition (recursive interpolation; an unseen context passes to the shorter one)"""
        k = len(ctx)
        if k == 0:
            return max(counts[0][(w,)] - discount, 0.0) / ctx_total[0][()] + gamma(()) / len(vocab)
        if ctx_total[k][ctx] == 0:
            return prob(ctx[1:], w)
        return max(counts[k][ctx + (w,)] - discount, 0.0) / ctx_total[k][ctx] + gamma(ctx) * prob(ctx[1:], w)

    sections = []
    for k in range(1, order + 1):
        if k == 1:
            listed = [("<s>",)] + [(w,) for w in vocab]
        else:
            listed = sorted(counts[k - 1])
        rows = []
        for g in listed:
            lp = -99.0 if g == ("<s>",) else math.log10(prob(g[:-1], g[-1]))
            bo = None
            if k < order:
                bo = math.log10(gamma(g)) if ctx_total[k][g] > 0 else None
            rows.append((lp, g, bo))
        sections.append(rows)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, rows in enumerate(sections, 1):
            f.write(f"ngram {k}={len(rows)}\n")
        for k, rows in enumerate(sections, 1):
            f.write(f"\n\\{k}-grams:\n")
            for lp, g, bo in rows:
                f.write(f"{lp!r}\t{' '.join(g)}" + ("" if bo is None else f"\t{bo!r}") + "\n")
        f.write("\n\\end\\\n")
    return vocab


# ------------------------------------------------------------------------------------------------ scorers for oracle.beam_search
class OracleNgramFull:
    """the reference scorer in the shape oracle.beam_search.BatchBeamSearch takes for a full scorer"""

    def __init__(self, ref: RefNgram):
        self.ref = ref

    def batch_init_state(self, x):
        return None

    def batch_score(self, ys, states, xs):
        import torch
        rows = np.stack([self.ref.score(y.tolist()) for y in ys])
        return torch.from_numpy(rows).to(xs.dtype), [None] * len(ys)

    def select_state(self, state, i, new_id=None):
        return None


class OracleNgramPart(OracleNgramFull):
    """the same scores as a partial scorer: zeros off the candidate ids"""

    def batch_score_partial(self, y, ids, state, x):
        import torch
        full, _ = self.batch_score(y, state, x)
        out = torch.zeros_like(full)
        out.scatter_(1, ids, full.gather(1, ids))
        return out, [None] * len(y)
