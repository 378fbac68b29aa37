"""CPU: the host side of the device error rates - the token tables ``ErrorCalculator`` builds for ``tavsr_error_counts``, the
separability check that decides whether they may be built, the reference restatements the GPU tests compare against
(tests/error_rates_ref.py), and ``validation()`` on CPU tensors."""
import random

import pytest
import torch

import error_rates_ref as R
from helpers import TOKENS_EN

LISTS = {"en": (TOKENS_EN, "<space>", "<blank>"), "bpe": (R.TOKENS_BPE,) + R.TOKENS_BPE_SYMS,
         "underbar": (R.TOKENS_BPE,) + R.TOKENS_UNDERBAR_SYMS}


def _table_text(tb, x, v):
    """token v of text x, read back from the flat tables as the kernel reads them"""
    V = len(tb["texts"][0])
    s0, s1 = int(tb["span"][x * (V + 1) + v]), int(tb["span"][x * (V + 1) + v + 1])
    return "".join(chr(c) for c in tb["cps"][s0:s1].tolist())


@pytest.mark.parametrize("name", sorted(LISTS))
def test_per_token_texts_joined_equal_the_host_calculators_strings(name):
    from tavsr import ops
    from tavsr.models.espnet_model import ErrorCalculator, error_tables
    assert callable(ops.error_counts) and callable(ops.edit_distance_rows) and isinstance(ops.DEVICE_ERROR_RATES, bool)
    tokens, space, blank = LISTS[name]
    calc = ErrorCalculator(tokens, space, blank, True, True)
    tb = calc.host_tables
    assert tb is not None and tb["tok_max"] == max(len(t) for text in tb["texts"] for t in text)
    V = len(tokens)
    for x in range(3):
        assert [_table_text(tb, x, v) for v in range(V)] == list(tb["texts"][x])
    assert tb["cp_space"].tolist() == [int(chr(c).isspace()) for c in tb["cps"].tolist()]
    assert [v for v in range(V) if tb["drop"][v]] == sorted({tokens.index(blank)} | ({tokens.index(space)} if space in tokens else set()))
    rng = random.Random(5)
    for _ in range(200):
        ids = [rng.randrange(V) for _ in range(rng.randrange(0, 12))]
        joined = "".join(tokens[i] for i in ids)
        assert "".join(tb["texts"][0][i] for i in ids) == joined
        assert "".join(tb["texts"][1][i] for i in ids) == joined.replace(space, " ").replace(blank, "")
        assert "".join(tb["texts"][2][i] for i in ids) == joined.replace(space, " ")


def test_separability_check_rejects_symbols_that_can_form_across_or_inside_tokens():
    from tavsr.models.espnet_model import error_tables
    for tokens, space, blank in LISTS.values():
        assert error_tables(tokens, space, blank) is not None
    assert error_tables(TOKENS_EN + ["<spa", "ce>"], "<space>", "<blank>") is None
    assert "<spa" + "ce>" == "<space>"      # what the joined replace would have found and the per-token replace not
    assert error_tables(TOKENS_EN + ["x<blank>y"], "<space>", "<blank>") is None
    assert error_tables(TOKENS_EN + ["<bl"], "<space>", "<blank>") is None
    assert error_tables(["aba", "b", "c"], "c", "aba") is None      # "aba" + "ba..." : the symbol ends in its own prefix "a"
    assert error_tables(TOKENS_EN + ["<space>x"], "<space>", "<blank>") is None
    assert error_tables(TOKENS_EN + ["x▁y"], "▁", "<blank>") is not None      # a one-character symbol cannot cross a boundary


def test_reference_word_splitter_equals_str_split():
    texts = ["", " ", "a", " a", "a ", "  ab  cd ", "ab\t\ncd e　 f", " x ", "new york  city ", "é \U0010ffff"]
    rng = random.Random(2)
    texts += ["".join(rng.choice("ab \t ") for _ in range(rng.randrange(0, 20))) for _ in range(200)]
    for t in texts:
        got = R.split_words([ord(c) for c in t], [c.isspace() for c in t])
        assert got == [tuple(ord(c) for c in w) for w in t.split()], repr(t)


def test_reference_levenshtein_equals_the_host_levenshtein():
    from tavsr.models.espnet_model import _levenshtein
    rng = random.Random(3)
    for _ in range(300):
        k = rng.choice([2, 3, 30])
        a = [rng.randrange(k) for _ in range(rng.randrange(0, 40))]
        b = [rng.randrange(k) for _ in range(rng.randrange(0, 40))]
        assert R.levenshtein(a, b) == _levenshtein(a, b)
    assert R.levenshtein(["ab", "c"], ["ab", "d", "c"]) == 1 and R.levenshtein("", "abc") == 3 and R.levenshtein("abc", "") == 3


@pytest.mark.parametrize("name", sorted(LISTS))
def test_reference_builders_and_host_counts_equal_the_host_calculator(name):
    """on CPU tensors ``counts`` takes the host route; summed over the batch it gives what ``cer_ctc`` / ``cer`` / ``wer`` divide"""
    from tavsr.models.espnet_model import ErrorCalculator
    tokens, space, blank = LISTS[name]
    calc = ErrorCalculator(tokens, space, blank, True, True)
    g = torch.Generator().manual_seed(4)
    V = len(tokens)
    ys_hat = torch.randint(0, V, (5, 14), generator=g)
    ys_hat[:, 3:6] = ys_hat[:, 3:4]
    ys_pad = torch.randint(0, V, (5, 9), generator=g)
    for b, n in enumerate([9, 6, 3, 1, 7]):
        ys_pad[b, n:] = -1
    want = {"ctc_chars": calc.cer_ctc(ys_hat, ys_pad)}
    want["att_chars"], want["att_words"] = calc(ys_hat[:, :10], ys_pad)
    for mode, rate in want.items():
        hat = ys_hat if mode == "ctc_chars" else ys_hat[:, :10]
        errs, ref_n = calc.counts(hat, ys_pad, mode)
        assert errs.dtype == ref_n.dtype == torch.int32 and not errs.is_cuda
        assert (errs.tolist(), ref_n.tolist()) == R.counts(tokens, space, blank, hat.tolist(), ys_pad.tolist(), mode)
        assert sum(errs.tolist()) / sum(ref_n.tolist()) == rate


def test_validation_on_cpu_tensors_returns_what_it_returned():
    from tavsr.train import validation

    class Toy(torch.nn.Module):
        def forward(self, x, cer):
            return x.square().mean().view(1), {"cer_ctc": cer}, torch.tensor(x.shape[0])

    g = torch.Generator().manual_seed(6)
    cers = [torch.tensor(0.25), 0.125, torch.tensor(1.0 / 3.0, dtype=torch.float64)]
    loader = [dict(x=torch.randn(4, 6, generator=g), cer=c) for c in cers]
    data_loss, data_cer = 0.0, 0.0      # the loop as it stood
    for batch in loader:
        data_loss += float(batch["x"].square().mean())
        data_cer += float(batch["cer"]) * 100.0
    assert validation(Toy(), loader, device="cpu") == (round(data_loss / 3, 3), round(data_cer / 3, 3))
