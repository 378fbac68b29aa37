"""``LMTask.build_model`` - the language-model recipes (configs/lm/*.yaml; the reference's configs/LM/lm-{english,spanish}.yaml
read by lm_main.py:78-95 and by src/inference/avsr_inference.py:141-176 through espnet2's ``LMTask``): ``lm: transformer`` with
``lm_conf`` -> an ``ESPnetLanguageModel``-shaped holder whose ``lm`` is the ``TransformerLM`` the beam search scores with
(``state_dict`` keys ``lm.embed.*``, ``lm.encoder.*``, ``lm.decoder.*`` as espnet2's).  ``ESPnetLanguageModel`` has espnet2's
interface (``nll`` / ``batchify_nll`` / ``forward``) on the HIP path, so the model the decode path scores with is also the one
``tavsr.train.lm_training`` trains (what lm_main.py:22-57 was written to do and cannot do as shipped: SURVEY section 2 #14)."""
from __future__ import annotations

import argparse

import torch

from .. import ops
from ..functional import LabelSmoothingLossFn
from ..lm.transformer_lm import TransformerLM
from ..utils.tokens import load_token_list

lm_choices = {"transformer": TransformerLM}


class ESPnetLanguageModel(torch.nn.Module):
    """espnet2 lm/espnet_model.py ESPnetLanguageModel.  Differences, all of them where espnet reads or loops on the host:
    the shifted rows are built by one launch (``ops.lm_shift``) and delimited by ``text_lengths`` alone, so the pad value of
    ``text`` (``ignore_id`` -1 in the recipes, espnet's default 0, anything else) never reaches the embedding or the loss;
    ``text`` keeps its width W instead of being cut to ``text_lengths.max()`` (all-padding columns are masked rows); the loss
    is sum / count with the count formed on the device.  A forward + backward step is therefore capturable."""

    def __init__(self, lm: torch.nn.Module, vocab_size: int, ignore_id: int = 0):
        super().__init__()
        self.lm, self.sos, self.eos, self.ignore_id = lm, vocab_size - 1, vocab_size - 1, ignore_id

    def _rows(self, text, text_lengths, max_length=None):
        """-> (logits [B, L+1, V], t [B, L+1], x_lengths [B] int64, n [B] int32) with L = W or ``max_length``"""
        text, text_lengths = text.to(torch.int64), text_lengths.to(torch.int64).contiguous()
        if max_length is not None:
            text = text[:, : int(max_length)]
        x, t, x_lengths, n = ops.lm_shift(text, text_lengths, self.eos, width=None if max_length is None else int(max_length) + 1)
        return self.lm(x, None, lengths=x_lengths)[0], t, x_lengths, n

    def nll(self, text, text_lengths, max_length=None):
        """-> (nll [B, L+1] per-token negative log-likelihood, 0 on padded positions; x_lengths [B]).  The rows carry no autograd
        graph: the differentiable quantity is ``forward``'s loss.  ``ops.row_sums(nll)`` gives the per-sentence sums."""
        with torch.no_grad():
            logits, t, x_lengths, _ = self._rows(text, text_lengths, max_length)
            B, L1, V = logits.shape
            row, _, _ = ops.lsm_loss(logits.reshape(B * L1, V), t.view(-1), -1, 0.0)
        return row.view(B, L1), x_lengths

    def batchify_nll(self, text, text_lengths, batch_size: int = 100):
        """``nll`` over slices of ``batch_size`` sentences, every slice at the full width (espnet pads to text_lengths.max())"""
        total = text.size(0)
        if total <= batch_size:
            return self.nll(text, text_lengths)
        nlls, lens = [], []
        for i in range(0, total, batch_size):
            a, b = self.nll(text[i: i + batch_size], text_lengths[i: i + batch_size], max_length=text.size(1))
            nlls.append(a)
            lens.append(b)
        return torch.cat(nlls), torch.cat(lens)

    def forward(self, text, text_lengths, **kwargs):
        """-> (loss = nll.sum() / ntokens, {"loss": loss.detach()}, weight = ntokens); nothing is read on the host."""
        logits, t, x_lengths, n = self._rows(text, text_lengths)
        loss, _ = LabelSmoothingLossFn.apply(logits, t, -1, 0.0, True, n)
        return loss, {"loss": loss.detach()}, x_lengths.sum()


class LMTask:
    @classmethod
    def build_model(cls, args: argparse.Namespace) -> ESPnetLanguageModel:
        token_list = load_token_list(args.token_list)
        args.token_list = list(token_list)
        name = getattr(args, "lm", "transformer")
        if name not in lm_choices:
            raise ValueError(f"--lm must be one of {tuple(lm_choices)}: {name}")
        lm = lm_choices[name](len(token_list), **(getattr(args, "lm_conf", None) or {}))
        return ESPnetLanguageModel(lm, len(token_list), **(getattr(args, "model_conf", None) or {}))
