"""The n-gram scorer without a GPU: the float64 reference (tests/ngram_ref.py) checks itself - generated models are proper
distributions, and its backoff agrees with a brute-force recursion written here - then the product's ARPA parser, word map and
tables (tavsr/lm/ngram.py, built on the CPU) against it."""
import itertools

import numpy as np
import pytest
import torch

import ngram_ref as R

WORDS = ["a", "b", "c", "d"]                     # + </s> + <unk>: a 6-word vocabulary


def _model(tmp_path, order, seed=0, with_unk=True, n_sent=40):
    path = tmp_path / f"m{order}_{seed}.arpa"
    vocab = R.write_arpa(path, R.random_sentences(WORDS, n_sent, seed, max_len=6, skew=0.7), order, WORDS, with_unk=with_unk)
    return path, vocab


def _contexts(vocab, order):
    """every context the scorer can meet, up to length order - 1: words of the vocabulary, with and without <s> in front"""
    for n in range(order):
        for c in itertools.product(vocab, repeat=n):
            yield c
            if n + 1 <= order - 1:
                yield ("<s>",) + c


def _brute(grams, ctx, w):
    """backoff by its textbook recursion: p(w | ctx) = listed value, else backoff(ctx) * p(w | ctx[1:])"""
    if len(ctx) == 0:
        return grams[0][(w,)][0]
    if ctx + (w,) in grams[len(ctx)]:
        return grams[len(ctx)][ctx + (w,)][0]
    return (grams[len(ctx) - 1][ctx][1] if ctx in grams[len(ctx) - 1] else 0.0) + _brute(grams, ctx[1:], w)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_generated_models_are_proper_and_the_reference_agrees_with_brute_force(tmp_path, order):
    path, vocab = _model(tmp_path, order)
    assert len(vocab) == 6
    ref = R.RefNgram(path, vocab)
    assert ref.order == order
    seen = unseen = 0
    worst = 0.0
    for ctx in _contexts(vocab, order):
        s = ref.score_words(ctx, vocab + ["<s>"])
        total = float(np.sum(10.0 ** s))
        worst = max(worst, abs(total - 1.0))
        assert abs(total - 1.0) < 1e-9, (ctx, total)
        want = np.array([_brute(ref.grams, tuple(ctx), w) for w in vocab + ["<s>"]])
        assert np.array_equal(s, want) or np.max(np.abs(s - want)) < 1e-12, ctx
        if len(ctx):
            listed = tuple(ctx) in ref.grams[len(ctx) - 1]
            seen, unseen = seen + listed, unseen + (not listed)
    print(f"order {order}: {seen} listed and {unseen} unlisted contexts, worst |sum - 1| = {worst:.2e}")
    assert order < 3 or (seen > 0 and unseen > 0)          # contexts never seen in the counts are covered


def test_word_map_rules(tmp_path):
    path, vocab = _model(tmp_path, 3)
    tokens = ["<blank>", "a", "b", "zzz", "<eos>", "<sos/eos>", "<unk>"]
    ref = R.RefNgram(path, tokens)
    assert ref.word_of == ["<unk>", "a", "b", "<unk>", "</s>", "<unk>", "<unk>"]
    g = ref.grams
    # <eos> scores as </s>, a token the ARPA does not list as <unk>; behind the empty history the context is <s>
    s = ref.score([5])
    assert ref.context_words([5]) == ("<s>",) and ref.context_words([1]) == ("<s>",)
    near = lambda x: pytest.approx(x, abs=1e-12)
    assert s[4] == near(_brute(g, ("<s>",), "</s>")) and s[3] == near(_brute(g, ("<s>",), "<unk>")) and s[3] == s[0] == s[5]
    assert s[1] == near(_brute(g, ("<s>",), "a"))
    # position 0 is <s> whatever token stands there; later positions are the tokens' words
    assert np.array_equal(ref.score([1, 2]), ref.score([5, 2])) and ref.context_words([1, 2, 3]) == ("b", "<unk>")
    assert ref.score([0, 1, 2])[1] == near(_brute(g, ("a", "b"), "a"))
    # without <unk> in the ARPA: -100 at the unigram level, behind the context's backoffs
    path2, _ = _model(tmp_path, 2, seed=1, with_unk=False)
    ref2 = R.RefNgram(path2, tokens)
    assert ref2.word_of[3] is None and ref2.word_of[0] is None and ref2.word_of[4] == "</s>"
    s2 = ref2.score([5])
    assert s2[3] == R.UNK_LOGP + ref2.grams[0][("<s>",)][1] and s2[3] < -100.0 + 1.0
    ref1 = R.RefNgram(_model(tmp_path, 1, seed=2, with_unk=False)[0], tokens)
    assert ref1.score([5, 1])[3] == -100.0
    # such a token inside the context: no suffix through it is listed (backoff 0)
    assert ref2.score([5, 3])[1] == ref2.grams[0][("a",)][0]


def _product_lm(path, tokens):
    from tavsr.lm.ngram import NgramLM
    return NgramLM.from_arpa(path, tokens, device="cpu")


def walk_tables(lm, tokens):
    """the kernel's walk (csrc/ngram.hip) over the product's tables, on the host in float64 of the fp32 values -> [V]"""
    word, logp, bo, cb = (t.numpy() for t in (lm.word, lm.logp, lm.backoff, lm.child_begin))
    wmap = lm.word_map.numpy()

    def child(node, w):
        if w < 0:
            return -1
        kids = word[cb[node]:cb[node + 1]]
        assert np.all(np.diff(kids) > 0)
        pos = int(np.searchsorted(kids, w))
        return int(cb[node]) + pos if pos < len(kids) and kids[pos] == w else -1

    ctx = [lm.bos_word] + [int(wmap[t]) for t in tokens[1:]]
    ctx = ctx[len(ctx) - min(len(ctx), lm.order - 1):]
    nodes = []
    for j in range(1, len(ctx) + 1):
        suf = ctx[len(ctx) - j:]
        node = suf[0]
        for w in suf[1:]:
            node = child(node, w) if node >= 0 else -1
        nodes.append(node)
    out = np.empty(len(wmap))
    for v, w in enumerate(wmap):
        acc, val = 0.0, None
        for j in range(len(ctx), 0, -1):
            node = nodes[j - 1]
            if node < 0:
                continue
            h = child(node, int(w))
            if h >= 0:
                val = float(logp[h]) + acc
                break
            acc += float(bo[node])
        out[v] = val if val is not None else (float(logp[w]) if w >= 0 else lm.unk_logp) + acc
    return out


@pytest.mark.parametrize("order,with_unk", [(1, True), (2, True), (3, True), (5, True), (3, False)])
def test_product_tables_walked_on_the_host_give_the_reference_scores(tmp_path, order, with_unk):
    path, vocab = _model(tmp_path, order, seed=3, with_unk=with_unk, n_sent=60)
    tokens = ["<blank>", "<unk>", "a", "b", "c", "d", "zzz", "<eos>", "<sos/eos>"]
    ref, lm = R.RefNgram(path, tokens), _product_lm(path, tokens)
    assert lm.order == order and lm.n_unigrams == len(ref.grams[0]) and lm.n_nodes == sum(len(g) for g in ref.grams)
    assert lm.word.dtype == lm.child_begin.dtype == lm.word_map.dtype == torch.int32
    assert lm.logp.dtype == lm.backoff.dtype == torch.float32
    assert [None if w < 0 else lm.words[w] for w in lm.word_map.tolist()] == ref.word_of
    assert lm.words[lm.bos_word] == "<s>"
    rng = np.random.RandomState(order)
    hyps = [[8]] + [[8] + rng.randint(0, len(tokens), size=n).tolist() for n in range(1, order + 3) for _ in range(6)]
    for y in hyps:
        got, want = walk_tables(lm, y), ref.score(y)
        assert np.max(np.abs(got - want)) < 1e-5, (y, got, want)          # fp32 storage of values of magnitude <= 100


def _write(tmp_path, text):
    p = tmp_path / "bad.arpa"
    p.write_text(text)
    return p


GOOD = ("\\data\\\nngram 1=3\nngram 2=2\n\n\\1-grams:\n-1.0\t<s>\t-0.5\n-0.3\ta\t-0.2\n-0.4\t</s>\n\n"
        "\\2-grams:\n-0.1\t<s> a\n-0.2\ta </s>\n\n\\end\\\n")


def test_parser_reads_a_plain_file_and_a_missing_backoff_is_zero(tmp_path):
    lm = _product_lm(_write(tmp_path, GOOD), ["a", "<eos>", "q"])
    assert lm.order == 2 and lm.n_unigrams == 3 and lm.n_nodes == 5
    assert lm.backoff.tolist() == pytest.approx([-0.5, -0.2, 0.0, 0.0, 0.0])
    assert lm.word_map.tolist() == [1, 2, -1] and lm.bos_word == 0
    assert lm.child_begin.tolist() == [3, 4, 5, 5, 5, 5]


@pytest.mark.parametrize("edit,line,what", [
    (lambda s: s.replace("ngram 2=2", "ngram 2=3"), 10, "has 2 lines"),                        # a section against the header
    (lambda s: s.replace("ngram 1=3", "ngram 1=2"), 5, "has 3 lines"),
    (lambda s: s.replace("-0.2\ta </s>", "-0.2\tb </s>"), 12, "prefix"),                       # prefix absent from the previous section
    (lambda s: s.replace("-0.3\ta\t-0.2", "-0.3x\ta\t-0.2"), 7, "non-numeric"),
    (lambda s: s.replace("-0.3\ta\t-0.2", "-0.3\ta\tzero"), 7, "non-numeric"),
    (lambda s: "\\data\\\n\n\\end\\\n", 3, "orders"),                                          # order 0
    (lambda s: s.replace("ngram 1=3", "ngram 0=3"), 2, "order 0"),
    (lambda s: s.replace("-0.1\t<s> a", "-0.1\t<s> zz"), 11, "not among the unigrams"),
    (lambda s: s.replace("\\end\\\n", ""), None, "no \\end\\"),
])
def test_parser_refusals_name_the_line(tmp_path, edit, line, what):
    p = _write(tmp_path, edit(GOOD))
    with pytest.raises(ValueError) as e:
        _product_lm(p, ["a"])
    msg = str(e.value)
    assert what in msg, msg
    if line is not None:
        assert f"{p}:{line}:" in msg, msg


def test_parser_refuses_an_order_above_the_maximum(tmp_path):
    from tavsr import _lib
    from tavsr.lm import ngram
    assert ngram.MAX_ORDER == _lib.ENUMS["TAVSR_NGRAM_MAX_ORDER"] == 8
    n = ngram.MAX_ORDER + 1
    text = "\\data\\\n" + "".join(f"ngram {k}=1\n" for k in range(1, n + 1))
    text += "".join(f"\n\\{k}-grams:\n-1.0\t{' '.join(['a'] * k)}\n" for k in range(1, n + 1)) + "\n\\end\\\n"
    p = _write(tmp_path, text)
    with pytest.raises(ValueError) as e:
        _product_lm(p, ["a"])
    assert "above the maximum of 8" in str(e.value) and f"{p}:{n + 3}:" in str(e.value)
    ok = text.replace(f"ngram {n}=1\n", "").split(f"\n\\{n}-grams:")[0] + "\n\\end\\\n"
    assert _product_lm(_write(tmp_path, ok), ["a"]).order == ngram.MAX_ORDER
