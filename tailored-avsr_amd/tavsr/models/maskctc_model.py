"""``MaskCTCModel`` / ``MaskCTCInference`` - drop-in for src/models/maskctc_model.py:41-349 (hybrid CTC / masked-LM model,
``model: maskctc`` with ``decoder: mlm``).

Training: the encoder, the CTC branch and the intermediate-CTC mix are the parent's; the decoder branch is the MLM loss
(``mask_uniform``, ``MLMDecoder``, label smoothing over the vocabulary with ``<mask>``).  The masks are drawn on the host from
numpy's generator as the reference draws them (``mask_draw = "host"``, the default), or on the device from the dropout
generator (``mask_draw = "device"``: ``ops.mask_uniform``, no host round trip, capturable with new masks per replay).
Decoding: the token bookkeeping of ``MaskCTCInference.forward`` is two kernels (``ops.maskctc_init`` / ``ops.maskctc_step``), so a batch is
decoded with one host read before the loop and one after it; every utterance follows its own iteration plan, i.e. comes out
as if it were decoded alone."""
from __future__ import annotations

from typing import List, NamedTuple, Tuple, Union

import numpy
import torch

from .. import functional as F_
from .. import ops
from ..ctc.ctc import CTC
from .espnet_model import ErrorCalculator, ESPnetASRModel, _Accuracy


def mask_uniform(ys_pad: torch.Tensor, mask_token: int, eos: int, ignore_id: int):
    """espnet ``maskctc/add_mask_token.py:mask_uniform``: per utterance ``n = randint(1, len + 1)`` positions drawn with
    replacement become ``mask_token`` in ``ys_in``; ``ys_out`` holds the target there and ``ignore_id`` elsewhere; padding is
    ``eos`` / ``ignore_id``.  Drawn on the host from numpy's GLOBAL generator in the reference's call order (one ``randint``,
    one ``choice`` per utterance), so a run seeded like the reference draws the same masks."""
    rows = [[t for t in row if t != ignore_id] for row in ys_pad.tolist()]
    L = max((len(r) for r in rows), default=0)
    ys_in = torch.full((len(rows), L), eos, dtype=torch.int64)
    ys_out = torch.full((len(rows), L), ignore_id, dtype=torch.int64)
    for i, r in enumerate(rows):
        n = numpy.random.randint(1, len(r) + 1)
        idx = torch.from_numpy(numpy.random.choice(len(r), n)).to(torch.int64)
        y = torch.tensor(r, dtype=torch.int64)
        ys_in[i, : len(r)] = y
        ys_in[i, idx] = mask_token
        ys_out[i, idx] = y[idx]
    return ys_in.to(ys_pad.device), ys_out.to(ys_pad.device)


class _MaskCTCMixin:
    """what MaskCTCModel and AVSRMaskCTCModel add to their parents (maskctc_model.py:95-115, :216-241)"""

    def _init_mlm(self, token_list, sym_mask, sym_space, sym_blank, report_cer, report_wer):
        token_list.append(sym_mask)               # (the caller's list grows, as in the reference)
        self.vocab_size += 1
        self.mask_token = self.vocab_size - 1
        self.token_list = list(token_list)
        self.criterion_mlm = F_.LabelSmoothingLossFn      # size = vocab_size with <mask>: the width of the decoder's logits
        self.error_calculator = (ErrorCalculator(self.token_list, sym_space, sym_blank, report_cer, report_wer)
                                 if (report_cer or report_wer) else None)

    # where the MLM masks are drawn: "host" (numpy's global generator in the reference's call order: a run seeded like the
    # reference draws its masks, but every step reads ``text`` on the host) or "device" (ops.mask_uniform: the reference's
    # distribution from the device generator's counter stream - the step makes no host round trip and can be captured, and
    # data-parallel ranks, seeded base + rank, draw different masks as they draw different dropout).  An attribute, not a
    # constructor argument: the constructors keep the reference's signatures.
    mask_draw = "host"
    last_mask_token = None      # introspection: the token of the last device draw (ops.mask_uniform(text, ..., token=) redraws it)

    def _decoder_branch(self, encoder_out, encoder_out_lens, text, text_lengths, ys_in_pad=None, ys_out_pad=None, **kwargs):
        loss_mlm = acc_mlm = None
        if self.ctc_weight != 1.0:
            count = None
            if ys_in_pad is None or ys_out_pad is None:      # (a caller may draw the masks itself, off the critical path)
                if self.mask_draw == "device":
                    ys_in_pad, ys_out_pad, n_target, self.last_mask_token = ops.mask_uniform(
                        text.contiguous(), self.mask_token, self.eos, self.ignore_id)
                    count = n_target if self.length_normalized_loss else None
                elif self.mask_draw == "host":
                    if text.is_cuda and torch.cuda.is_current_stream_capturing():
                        raise NotImplementedError("mask_uniform draws on the host: set mask_draw = \"device\" or pass ys_in_pad / "
                                                  "ys_out_pad to a captured step")
                    ys_in_pad, ys_out_pad = mask_uniform(text, self.mask_token, self.eos, self.ignore_id)
                else:
                    raise ValueError(f"mask_draw must be \"host\" or \"device\", got {self.mask_draw!r}")
            decoder_out, _ = self.decoder(encoder_out, encoder_out_lens, ys_in_pad.to(text.device), text_lengths)
            loss_mlm, correct = self.criterion_mlm.apply(decoder_out, ys_out_pad.to(text.device).to(torch.int64), self.ignore_id,
                                                         self.lsm_weight, self.length_normalized_loss, count)
            acc_mlm = _Accuracy(correct)
        return loss_mlm, {"loss_mlm": loss_mlm.detach() if loss_mlm is not None else None, "acc_mlm": acc_mlm}

    def nll(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens):
        raise NotImplementedError

    def batchify_nll(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, batch_size: int = 100):
        raise NotImplementedError


class MaskCTCModel(_MaskCTCMixin, ESPnetASRModel):
    def __init__(self, vocab_size: int, token_list: Union[Tuple[str, ...], List[str]], frontend, specaug, normalize,
                 preencoder, encoder, postencoder, decoder, ctc: CTC, joint_network=None, ctc_weight: float = 0.5,
                 interctc_weight: float = 0.0, ignore_id: int = -1, lsm_weight: float = 0.0,
                 length_normalized_loss: bool = False, report_cer: bool = True, report_wer: bool = True,
                 sym_space: str = "<space>", sym_blank: str = "<blank>", sym_mask: str = "<mask>",
                 extract_feats_in_collect_stats: bool = True):
        super().__init__(vocab_size=vocab_size, token_list=token_list, frontend=frontend, specaug=specaug, normalize=normalize,
                         preencoder=preencoder, encoder=encoder, postencoder=postencoder, decoder=decoder, ctc=ctc,
                         joint_network=joint_network, ctc_weight=ctc_weight, interctc_weight=interctc_weight,
                         ignore_id=ignore_id, lsm_weight=lsm_weight, length_normalized_loss=length_normalized_loss,
                         report_cer=report_cer, report_wer=report_wer, sym_space=sym_space, sym_blank=sym_blank,
                         extract_feats_in_collect_stats=extract_feats_in_collect_stats)
        self._init_mlm(token_list, sym_mask, sym_space, sym_blank, report_cer, report_wer)


class Hypothesis(NamedTuple):
    """espnet.nets.beam_search.Hypothesis as far as Mask-CTC fills it"""
    yseq: torch.Tensor
    score: float = 0.0
    scores: dict = {}
    states: dict = {}


class MaskCTCInference(torch.nn.Module):
    """maskctc_model.py:263-349.  ``forward(enc_out [T, D])`` is the reference's call (one utterance -> Hypothesis with ``yseq``
    framed by two ``<mask>`` ids); ``decode(enc [B, T, D], enc_lens)`` is the batch form it is built on."""

    def __init__(self, asr_model, n_iterations: int, threshold_probability: float):
        super().__init__()
        self.ctc = asr_model.ctc
        self.mlm = asr_model.decoder
        self.mask_token = asr_model.mask_token
        self.n_iterations = n_iterations
        self.threshold_probability = threshold_probability
        self.token_list = list(asr_model.token_list)

    def ids2text(self, ids: List[int]):
        text = "".join(self.token_list[i] for i in ids)
        return text.replace("<mask>", "_").replace("<space>", " ")

    @torch.no_grad()
    def start(self, enc, enc_lens):
        """-> (y_in, y_hat, tok_prob [B, T], y_len [B], plan [B, 3]) on the device (ops.maskctc_init; blank is id 0, :291)"""
        return ops.maskctc_init(self.ctc._logits(enc).contiguous(), enc_lens.to(torch.int64), 0, self.mask_token,
                                self.threshold_probability, self.n_iterations)

    @torch.no_grad()
    def passes(self, enc, enc_lens, y_in, dec_lens, y_len, plan, n_passes, memory_kv=None, trace=None):
        """``n_passes`` passes of the fill loop on ``y_in`` [B, L] (in place): decoder forward + ops.maskctc_step, nothing read
        back - the launch sequence of a given (B, L, T) is fixed and can be captured.  ``trace``: a list that receives a clone of
        ``y_in`` after every pass (tests)."""
        for it in range(n_passes):
            logits, _ = self.mlm(enc, enc_lens, y_in, dec_lens, memory_kv=memory_kv)
            ops.maskctc_step(logits, y_in, y_len, plan, it, self.mask_token)
            if trace is not None:
                trace.append(y_in.clone())
        return y_in

    @torch.no_grad()
    def decode(self, enc, enc_lens, hoist: bool = True, trace=None) -> List[List[int]]:
        """-> per utterance the framed id list ``[<mask>] + tokens + [<mask>]``."""
        B = enc.shape[0]
        enc = enc.contiguous()
        enc_lens = enc_lens.to(torch.int64)
        y_in, _, _, y_len, plan = self.start(enc, enc_lens)
        host = torch.cat([y_len, plan[:, 1].to(torch.int64)]).tolist()      # the one host read before the loop
        lens, n_passes = host[:B], max(host[B:])
        L = max(lens)
        y = y_in[:, : max(L, 1)].contiguous()
        if trace is not None:
            trace.append(y.clone())
        if n_passes > 0:
            kv = self.mlm.prepare_memory(enc, enc_lens) if hoist else None
            # an utterance without tokens still gives the decoder one (padding) position to attend to
            self.passes(enc, enc_lens, y, y_len.clamp(min=1), y_len, plan, n_passes, memory_kv=kv, trace=trace)
        ids = y.tolist()
        return [[self.mask_token] + ids[b][: lens[b]] + [self.mask_token] for b in range(B)]

    def forward(self, enc_out: torch.Tensor) -> Hypothesis:
        T = enc_out.shape[0]
        lens = torch.full((1,), T, dtype=torch.int64, device=enc_out.device)
        (yseq,) = self.decode(enc_out.unsqueeze(0), lens)
        return Hypothesis(yseq=torch.tensor(yseq, device=enc_out.device))
