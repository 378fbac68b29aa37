"""Test-side reference of language-model training: espnet2's ``ESPnetLanguageModel`` (lm/espnet_model.py ``nll`` /
``batchify_nll`` / ``forward``) restated in plain torch over ``oracle.beam_search.TransformerLMOracle``, and ``lm_shift``,
the shifted input / target rows with the per-sentence loop espnet has.

Two things differ from espnet's text, both where espnet cannot run on the reference's batches: rows are delimited by the
lengths (espnet leaves the pad value of ``text`` in ``x``, where ``ignore_id: -1`` would index the embedding), and the target
padding is -1 under ``ignore_index=-1`` (espnet pads the targets with ``ignore_id`` and masks the rows afterwards; the nll rows
are the same).  The oracle masks keys whose id is 0, which is what ``x`` holds behind a sentence."""
import torch
import torch.nn.functional as F


def lm_shift(text, lengths, sos_eos, width=None):
    """text [B][W] ints, lengths [B] -> (x, t [B, width] int64, x_lengths [B] int64, n [B] int32); width defaults to W + 1"""
    B = len(text)
    W = len(text[0]) if B else 0
    width = W + 1 if width is None else width
    x = torch.zeros((B, width), dtype=torch.int64)
    t = torch.full((B, width), -1, dtype=torch.int64)
    for i, l in enumerate(lengths):
        l = int(l)
        x[i, 0] = sos_eos
        for j in range(l):
            x[i, j + 1] = int(text[i][j])
            t[i, j] = int(text[i][j])
        t[i, l] = sos_eos
    x_lengths = torch.as_tensor([int(l) + 1 for l in lengths], dtype=torch.int64)
    return x, t, x_lengths, x_lengths.to(torch.int32)


class LMRef(torch.nn.Module):
    def __init__(self, lm, vocab_size):
        super().__init__()
        self.lm, self.sos, self.eos = lm, vocab_size - 1, vocab_size - 1

    def nll(self, text, text_lengths, max_length=None):
        B = text.size(0)
        text = text[:, : int(text_lengths.max())] if max_length is None else text[:, :max_length]
        x, t, x_lengths, _ = lm_shift(text.tolist(), text_lengths.tolist(), self.eos,
                                      width=None if max_length is None else max_length + 1)
        y, _ = self.lm(x, None)
        nll = F.cross_entropy(y.view(-1, y.shape[-1]), t.view(-1), reduction="none", ignore_index=-1)
        return nll.view(B, -1), x_lengths

    def batchify_nll(self, text, text_lengths, batch_size=100):
        total = text.size(0)
        if total <= batch_size:
            return self.nll(text, text_lengths)
        nlls, lens = [], []
        max_length = int(text_lengths.max())
        for i in range(0, total, batch_size):
            a, b = self.nll(text[i: i + batch_size], text_lengths[i: i + batch_size], max_length=max_length)
            nlls.append(a)
            lens.append(b)
        return torch.cat(nlls), torch.cat(lens)

    def forward(self, text, text_lengths):
        nll, y_lengths = self.nll(text, text_lengths)
        ntokens = y_lengths.sum()
        loss = nll.sum() / ntokens
        return loss, {"loss": loss.detach()}, ntokens
