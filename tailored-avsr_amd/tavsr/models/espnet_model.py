"""``ESPnetASRModel`` - drop-in for src/models/espnet_model.py:38-593 (hybrid CTC/attention branch).

``forward(speech, speech_lengths, text, text_lengths) -> (loss, stats, weight)`` with the reference's
stats keys; ``encode`` as used by inference.  Host code here is orchestration only (tiny integer
tensor manipulation such as add_sos_eos); every floating-point op runs in libtavsr_hip.so.
"""
from __future__ import annotations

import os
from itertools import groupby
from typing import Dict, List, Optional, Tuple, Union

import weakref

import torch

from .. import functional as F_
from .. import ops
from ..ctc.ctc import CTC
from ..functional_rnnt import RNNTLossFn


def add_sos_eos(ys_pad, ys_lens, sos, eos, ignore_id):
    """espnet add_sos_eos on padded int64 batches without a per-utterance Python loop."""
    B, L = ys_pad.shape
    idx = torch.arange(L + 1, device=ys_pad.device)[None, :]
    lens = ys_lens[:, None]
    body = torch.nn.functional.pad(ys_pad, (1, 0), value=sos)
    ys_in = torch.where(idx <= lens, body, torch.full_like(body, eos))
    ys_in[:, 0] = sos
    tail = torch.nn.functional.pad(ys_pad, (0, 1), value=ignore_id)
    ys_out = torch.where(idx < lens, tail, torch.full_like(tail, ignore_id))
    ys_out = torch.where(idx == lens, torch.full_like(tail, eos), ys_out)
    return ys_in, ys_out


def _levenshtein(a, b) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, cb in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb))
        prev = cur
    return prev[-1]


def _separable(tokens, sym) -> bool:
    """Does ``"".join(tokens of any id sequence).replace(sym, x)`` equal the join of the per-token ``replace``?  A sufficient
    condition: ``sym`` is one character, or no token other than ``sym`` itself contains it and no token (``sym`` included) ends
    in a non-empty proper prefix of it - then no occurrence of ``sym`` in a joined string can cross a token boundary."""
    if not sym:
        return False
    if len(sym) == 1:
        return True
    prefixes = tuple(sym[:k] for k in range(1, len(sym)))
    return not any((sym in t and t != sym) or t.endswith(prefixes) for t in tokens)


def error_tables(char_list, sym_space, sym_blank):
    """The token tables of ``tavsr_error_counts`` (include/tavsr.h) on the host, or None where ``_separable`` does not hold for
    ``sym_space`` on the tokens or for ``sym_blank`` on the tokens after the space replacement.  ``texts``: per token (0) the
    token, (1) what the hypothesis of ``ErrorCalculator.__call__`` makes of it (space -> " ", then blank -> "") and (2) what
    the reference makes of it (space -> " "); ``span`` int32 [3 * (V + 1)], ``cps`` int32 and ``cp_space`` uint8 (``str.isspace``
    of each code point), ``drop`` uint8 [V] (blank / space: left out by ``cer_ctc``), ``tok_max``: the longest text."""
    raw = list(char_list)
    if not _separable(raw, sym_space):
        return None
    ref = [t.replace(sym_space, " ") for t in raw]
    if not _separable(ref, sym_blank):
        return None
    texts = (raw, [t.replace(sym_blank, "") for t in ref], ref)
    span, chars = [], []
    for text in texts:
        for t in text:
            span.append(len(chars))
            chars.extend(t)
        span.append(len(chars))
    chars.append("\0")      # a table of empty tokens still has an address
    return dict(texts=texts, span=torch.tensor(span, dtype=torch.int32), cps=torch.tensor([ord(c) for c in chars], dtype=torch.int32),
                cp_space=torch.tensor([c.isspace() for c in chars], dtype=torch.uint8),
                drop=torch.tensor([t in (sym_blank, sym_space) for t in raw], dtype=torch.uint8),
                tok_max=max(1, max(len(t) for text in texts for t in text)))


class ErrorCalculator:
    """CER/WER of espnet.nets.e2e_asr_common.ErrorCalculator on id sequences (eval only).

    Two routes compute the same integers.  The host route joins the token strings and runs ``_levenshtein`` in Python.  The
    device route (``ops.error_counts``, csrc/editdist.hip) reads nothing on the host; it is taken when the inputs are CUDA
    tensors, ``ops.DEVICE_ERROR_RATES`` is on, the token tables exist and ``ops.error_counts_ok`` takes the shape.  The tables
    hold per-token texts, so they exist only where replacing ``sym_space`` / ``sym_blank`` per token equals the host's replace on
    the joined string: ``_separable`` states the sufficient condition that is checked, and a calculator whose token list fails
    it stays on the host route for good.  An id outside the token list, which the host route raises on (or wraps, when
    negative and not -1), contributes nothing on the device route.

    The host route returns Python floats, ``None`` for ``cer_ctc`` over empty references, and raises ``ZeroDivisionError`` for
    ``cer`` / ``wer`` over empty references.  The device route returns 0-dim float64 device tensors, ``errs.sum() / ref_n.sum()`` in
    double, whose ``float()`` has the bits of the host's division; in the two empty-reference cases it returns NaN."""

    MODES = {"ctc_chars": 1, "att_chars": 2, "att_words": 4}      # the bits of tavsr_error_counts' `modes`

    def __init__(self, char_list, sym_space, sym_blank, report_cer=False, report_wer=False):
        self.char_list, self.space, self.blank = char_list, sym_space, sym_blank
        self.report_cer, self.report_wer = report_cer, report_wer
        self.idx_blank = char_list.index(sym_blank)
        self.idx_space = char_list.index(sym_space) if sym_space in char_list else None
        self.host_tables = error_tables(char_list, sym_space, sym_blank)
        self._device_tables = {}

    def _tables(self, ys_hat, ys_pad, modes):
        """the device route's tables for this call, or None: the host route"""
        if not (ops.DEVICE_ERROR_RATES and ys_hat.is_cuda and ys_pad.is_cuda and self.host_tables is not None):
            return None
        h = self.host_tables
        if not ops.error_counts_ok(modes, ys_hat.shape[0], ys_hat.shape[1], ys_pad.shape[1], h["tok_max"]):
            return None
        tb = self._device_tables.get(ys_hat.device)
        if tb is None:      # once per device
            tb = self._device_tables[ys_hat.device] = ops.ErrorTables(
                *(h[k].to(ys_hat.device) for k in ("span", "cps", "cp_space", "drop")), len(self.char_list), h["tok_max"])
        return tb

    @staticmethod
    def _rate(errs, ref_n):
        e, n = errs.sum().double(), ref_n.sum().double()
        return (e / n).masked_fill(n == 0, float("nan"))

    def counts(self, ys_hat, ys_pad, mode):
        """(errs [B], ref_n [B]) int32 of ``mode`` ("ctc_chars", "att_chars", "att_words"): per utterance the edit count and the
        reference length that ``cer_ctc`` / ``cer`` / ``wer`` sum over the batch, for callers that sum over a corpus.  On the
        device where the device route takes the call, else on the host."""
        tb = self._tables(ys_hat, ys_pad, self.MODES[mode])
        if tb is not None:
            errs, ref_n = ops.error_counts(ys_hat, ys_pad, tb, self.MODES[mode])
            return errs[0], ref_n[0]
        pairs = []
        for y, ref in zip(ys_hat.tolist(), ys_pad.tolist()):
            if mode == "ctc_chars":
                keep = lambda i: i != -1 and i != self.idx_blank and i != self.idx_space
                h = "".join(self.char_list[i] for i, _ in groupby(y) if keep(i))
                r = "".join(self.char_list[i] for i in ref if keep(i))
            else:
                ymax = ref.index(-1) if -1 in ref else len(ref)
                h = "".join(self.char_list[i] for i in y[:ymax]).replace(self.space, " ").replace(self.blank, "")
                r = "".join(self.char_list[i] for i in ref if i != -1).replace(self.space, " ")
                h, r = (h.split(), r.split()) if mode == "att_words" else (h.replace(" ", ""), r.replace(" ", ""))
            pairs.append((_levenshtein(h, r) if (r or mode != "ctc_chars") else 0, len(r)))
        return tuple(torch.tensor(c, dtype=torch.int32) for c in (zip(*pairs) if pairs else ((), ())))

    def cer_ctc(self, ys_hat, ys_pad):
        tb = self._tables(ys_hat, ys_pad, self.MODES["ctc_chars"])
        if tb is not None:
            return self._rate(*ops.error_counts(ys_hat, ys_pad, tb, self.MODES["ctc_chars"]))
        errs, n = 0, 0
        for y, ref in zip(ys_hat.tolist(), ys_pad.tolist()):
            keep = lambda i: i != -1 and i != self.idx_blank and i != self.idx_space
            # the reference joins the token strings and measures the edit distance over CHARACTERS of the joined
            # text, so a multi-character token such as "<unk>" counts as five symbols (espnet ErrorCalculator.calculate_cer_ctc)
            hyp = "".join(self.char_list[i] for i, _ in groupby(y) if keep(i))
            tru = "".join(self.char_list[i] for i in ref if keep(i))
            if tru:
                errs += _levenshtein(hyp, tru)
                n += len(tru)
        return errs / n if n else None

    def __call__(self, ys_hat, ys_pad, is_ctc=False):
        if is_ctc:
            return self.cer_ctc(ys_hat, ys_pad)
        modes = (self.MODES["att_chars"] if self.report_cer else 0) | (self.MODES["att_words"] if self.report_wer else 0)
        tb = self._tables(ys_hat, ys_pad, modes) if modes else None
        if tb is not None:      # cer and wer of the batch in one launch
            errs, ref_n = ops.error_counts(ys_hat, ys_pad, tb, modes)
            rates = [self._rate(errs[k], ref_n[k]) for k in range(errs.shape[0])]
            return (rates.pop(0) if self.report_cer else None), (rates.pop(0) if self.report_wer else None)
        hyps, refs = [], []
        for y, ref in zip(ys_hat.tolist(), ys_pad.tolist()):
            ymax = ref.index(-1) if -1 in ref else len(ref)
            h = "".join(self.char_list[i] for i in y[:ymax]).replace(self.space, " ").replace(self.blank, "")
            r = "".join(self.char_list[i] for i in ref if i != -1).replace(self.space, " ")
            hyps.append(h)
            refs.append(r)
        cer = wer = None
        if self.report_cer:
            d = sum(_levenshtein(list(h.replace(" ", "")), list(r.replace(" ", ""))) for h, r in zip(hyps, refs))
            cer = d / sum(len(r.replace(" ", "")) for r in refs)
        if self.report_wer:
            d = sum(_levenshtein(h.split(), r.split()) for h, r in zip(hyps, refs))
            wer = d / sum(len(r.split()) for r in refs)
        return cer, wer


LOSS_BRANCH = True      # CTC branch beside the attention decoder (TAVSR_SINGLE_STREAM=1 disables every fork)


_MAX_SEEN = {}      # id(lengths tensor) -> (weak reference, tensor version, maximum)


def host_max(lengths: torch.Tensor) -> int:
    """``int(lengths.max())`` without stalling the launch queue where that can be avoided.  Reading a device scalar makes the
    host wait for everything enqueued before it - at the top of a training step that is the previous step's backward pass, so
    the host cannot run ahead across steps and the GPU starves at every step start (2.3 ms of a 17.7 ms audio-only step).
    The collate functions know the lengths on the host and attach the maximum (``_tavsr_max``, utils/avsr_dataloader.py);
    a tensor object that was already asked about (same object, same version counter: a fixed benchmark or validation batch)
    answers from a cache; anything else costs the one sync the reference pays too (espnet_model.py:372)."""
    m = getattr(lengths, "_tavsr_max", None)
    if m is not None:
        # (version counter at the time the maximum was attached, maximum): an in-place edit of the collated tensor (copy_, clamp_,
        # sub_) bumps the version and the hint is dropped for the synced path below
        if isinstance(m, tuple):
            if m[0] == lengths._version:
                return int(m[1])
        else:
            return int(m)
    if not lengths.is_cuda:
        return int(lengths.max())
    key = id(lengths)
    e = _MAX_SEEN.get(key)
    if e is not None and e[0]() is lengths and e[1] == lengths._version:
        return e[2]
    m = int(lengths.max())
    _MAX_SEEN[key] = (weakref.ref(lengths, lambda _r, k=key: _MAX_SEEN.pop(k, None)), lengths._version, m)
    return m


def cut_to_longest(x: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """``x[:, : lengths.max()]`` - the reference's "for data-parallel" cut of an over-padded batch
    (src/models/espnet_model.py:372 / avsr_espnet_model.py:499 ``_extract_feats``, ``forward`` text cut :247).  The
    maximum is a host value (``host_max``); while a hipGraph is being captured no sync is possible and the batch must
    already be tightly padded (a captured step has static shapes anyway)."""
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        return x
    m = host_max(lengths)
    return x if m >= x.shape[1] else x[:, :m].contiguous()


class UtteranceMVN(torch.nn.Module):
    """espnet2 UtteranceMVN(norm_means=True, norm_vars=False) on the HIP path."""

    def __init__(self, norm_means: bool = True, norm_vars: bool = False, eps: float = 1.0e-20):
        super().__init__()
        if not norm_means or norm_vars:
            raise ValueError("HIP path covers norm_means=true, norm_vars=false (all shipped configs)")

    def forward(self, x, ilens):
        return ops.utterance_mvn(x.contiguous(), ilens.to(torch.int64)), ilens


class ESPnetASRModel(torch.nn.Module):
    def __init__(self, vocab_size: int, token_list: Union[Tuple[str, ...], List[str]], frontend, specaug, normalize,
                 preencoder, encoder, postencoder, decoder, ctc: CTC, joint_network=None, aux_ctc: dict = None,
                 ctc_weight: float = 0.5, interctc_weight: float = 0.0, ignore_id: int = -1, lsm_weight: float = 0.0,
                 length_normalized_loss: bool = False, report_cer: bool = True, report_wer: bool = True,
                 sym_space: str = "<space>", sym_blank: str = "<blank>", transducer_multi_blank_durations: List = [],
                 transducer_multi_blank_sigma: float = 0.05, sym_sos: str = "<sos/eos>", sym_eos: str = "<sos/eos>",
                 extract_feats_in_collect_stats: bool = True, lang_token_id: int = -1):
        assert 0.0 <= ctc_weight <= 1.0, ctc_weight
        assert 0.0 <= interctc_weight < 1.0, interctc_weight
        super().__init__()
        if preencoder is not None or postencoder is not None:
            raise ValueError("pre- / post-encoder branches are out of the hot path (no shipped config)")
        self.use_transducer_decoder = joint_network is not None      # espnet_model.py:114-147
        if self.use_transducer_decoder:
            if transducer_multi_blank_durations:
                raise ValueError("transducer_multi_blank_durations: the multi-blank transducer loss is not on the HIP path "
                                 "(leave the list empty: the plain RNN-T loss)")
            if decoder is None:
                raise ValueError("a joint network needs a transducer decoder (decoder: transducer)")
            self.joint_network = joint_network
        self.blank_id = token_list.index(sym_blank) if sym_blank in token_list else 0
        self.sos = token_list.index(sym_sos) if sym_sos in token_list else vocab_size - 1
        self.eos = token_list.index(sym_eos) if sym_eos in token_list else vocab_size - 1
        self.vocab_size, self.ignore_id = vocab_size, ignore_id
        self.ctc_weight, self.interctc_weight, self.aux_ctc = ctc_weight, interctc_weight, aux_ctc
        self.token_list = list(token_list)
        self.frontend, self.specaug, self.normalize, self.encoder = frontend, specaug, normalize, encoder
        if not hasattr(self.encoder, "interctc_use_conditioning"):
            self.encoder.interctc_use_conditioning = False
        if self.encoder.interctc_use_conditioning:       # espnet_model.py:109-112
            self.encoder.conditioning_layer = torch.nn.Linear(vocab_size, self.encoder.output_size())
        self.decoder = decoder if (ctc_weight < 1.0 or self.use_transducer_decoder) else None
        self.lsm_weight, self.length_normalized_loss = lsm_weight, length_normalized_loss
        self.error_calculator = (ErrorCalculator(self.token_list, sym_space, sym_blank, report_cer, report_wer)
                                 if (report_cer or report_wer) else None)
        self.ctc = ctc if ctc_weight != 0.0 else None

    # ---------------------------------------------------------------- espnet_model.py:369-430
    def encode(self, speech: torch.Tensor, speech_lengths: torch.Tensor):
        # espnet_model.py:372: the batch is cut to its longest utterance (the STFT's reflect padding sees the tensor end)
        speech = cut_to_longest(speech, speech_lengths)
        if self.frontend is not None:
            feats, feats_lengths = self.frontend(speech, speech_lengths)
        else:
            feats, feats_lengths = speech, speech_lengths
        if self.specaug is not None and self.training:
            feats, feats_lengths = self.specaug(feats, feats_lengths)
        if self.normalize is not None:
            feats, feats_lengths = self.normalize(feats, feats_lengths)
        if self.encoder.interctc_use_conditioning:       # espnet_model.py:397-402
            encoder_out, encoder_out_lens, _ = self.encoder(feats, feats_lengths, ctc=self.ctc)
        else:
            encoder_out, encoder_out_lens, _ = self.encoder(feats, feats_lengths)
        return encoder_out, encoder_out_lens

    # ---------------------------------------------------------------- espnet_model.py:206-356
    def forward(self, speech, speech_lengths, text, text_lengths, **kwargs):
        assert text_lengths.dim() == 1, text_lengths.shape
        assert speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0], (
            speech.shape, speech_lengths.shape, text.shape, text_lengths.shape)
        batch_size = speech.shape[0]
        ops.rng_step_begin(speech.device)    # fresh dropout masks for this step (a kernel: captured graphs replay it)
        text = cut_to_longest(text.to(torch.int64).masked_fill(text == -1, self.ignore_id), text_lengths)
        encoder_out, encoder_out_lens = self.encode(speech, speech_lengths)
        return self._hybrid_loss(encoder_out, encoder_out_lens, text, text_lengths, batch_size, **kwargs)

    # CTC + attention losses and the stats dict: espnet_model.py:258-356 == avsr_espnet_model.py:253-367
    def _hybrid_loss(self, encoder_out, encoder_out_lens, text, text_lengths, batch_size, **kwargs):
        intermediate_outs = None
        if isinstance(encoder_out, tuple):
            encoder_out, intermediate_outs = encoder_out
        stats: Dict[str, Optional[torch.Tensor]] = dict()
        loss_ctc = loss_att = None
        # training: the CTC branch (projection, loss, their backward) is independent of the attention decoder - it is enqueued on
        # the side queue and runs beside the decoder, forward and (autograd replays a node on its forward queue) backward
        beside = self.ctc_weight != 0.0 if self.use_transducer_decoder else self.ctc_weight not in (0.0, 1.0)
        br = ops.BranchScope(LOSS_BRANCH and self.training and encoder_out.is_cuda and beside)
        with br:
            if self.ctc_weight != 0.0:
                loss_ctc = self.ctc(encoder_out, encoder_out_lens, text, text_lengths)
                cer_ctc = None
                if not self.training and self.error_calculator is not None:
                    ys_hat = self.ctc.argmax(encoder_out).data
                    cer_ctc = self.error_calculator(ys_hat, text, is_ctc=True)
                stats["loss_ctc"], stats["cer_ctc"] = loss_ctc.detach(), cer_ctc
            if self.interctc_weight != 0.0 and intermediate_outs is not None:      # espnet_model.py:260-304
                if self.aux_ctc is not None:
                    raise NotImplementedError("aux_ctc tasks are not used by any shipped recipe")
                loss_interctc = None
                for layer_idx, intermediate_out in intermediate_outs:
                    loss_ic = self.ctc(intermediate_out, encoder_out_lens, text, text_lengths)
                    cer_ic = None
                    if not self.training and self.error_calculator is not None:
                        ys_hat = self.ctc.argmax(intermediate_out).data
                        cer_ic = self.error_calculator(ys_hat, text, is_ctc=True)
                    loss_interctc = loss_ic if loss_interctc is None else F_.WeightedSumFn.apply(loss_interctc, loss_ic, 1.0, 1.0)
                    stats[f"loss_interctc_layer{layer_idx}"] = loss_ic.detach()
                    stats[f"cer_interctc_layer{layer_idx}"] = cer_ic
                n_ic = len(intermediate_outs)
                loss_ctc = F_.WeightedSumFn.apply(loss_ctc, loss_interctc, 1 - self.interctc_weight, self.interctc_weight / n_ic)
        if self.use_transducer_decoder:      # espnet_model.py:306-328: the transducer branch takes the attention decoder's place
            loss_transducer = self._calc_transducer_loss(encoder_out, encoder_out_lens, text, text_lengths)
            br.join()
            loss = loss_transducer if loss_ctc is None else F_.WeightedSumFn.apply(loss_transducer, loss_ctc, 1.0, self.ctc_weight)
            # (espnet's ErrorCalculatorTransducer decodes with a beam search at validation: not computed here)
            stats.update(loss_transducer=loss_transducer.detach(), cer_transducer=None, wer_transducer=None, loss=loss.detach())
            weight = torch.full((1,), batch_size, dtype=torch.long, device=loss.device)
            return loss.view(1), stats, weight
        loss_att, dec_stats = self._decoder_branch(encoder_out, encoder_out_lens, text, text_lengths, **kwargs)
        br.join()
        if self.ctc_weight == 0.0:
            loss = loss_att
        elif self.ctc_weight == 1.0:
            loss = loss_ctc
        else:
            loss = F_.WeightedSumFn.apply(loss_ctc, loss_att, self.ctc_weight, 1 - self.ctc_weight)
        stats.update(dec_stats)
        stats["loss"] = loss.detach()
        weight = torch.full((1,), batch_size, dtype=torch.long, device=loss.device)
        return loss.view(1), stats, weight

    # the decoder's loss and its stats entries (espnet_model.py:306-317, 332-336); the Mask-CTC models put their MLM branch here
    def _decoder_branch(self, encoder_out, encoder_out_lens, text, text_lengths, **kwargs):
        loss_att = acc_att = cer_att = wer_att = None
        if self.ctc_weight != 1.0:
            ys_in, ys_out = add_sos_eos(text, text_lengths, self.sos, self.eos, self.ignore_id)
            decoder_out, _ = self.decoder(encoder_out, encoder_out_lens, ys_in, text_lengths + 1)
            loss_att, correct = F_.LabelSmoothingLossFn.apply(decoder_out, ys_out, self.ignore_id, self.lsm_weight,
                                                             self.length_normalized_loss)
            acc_att = _Accuracy(correct)
            if not self.training and self.error_calculator is not None:
                ids, _, _ = ops.ctc_greedy(decoder_out.detach().contiguous(), None, -1, collapse=False)  # argmax(-1)
                cer_att, wer_att = self.error_calculator(ids, text)
        return loss_att, {"loss_att": loss_att.detach() if loss_att is not None else None, "acc": acc_att, "cer": cer_att,
                          "wer": wer_att}

    # espnet_model.py:595-641 over espnet2 asr_transducer/utils.py get_transducer_task_io: decoder input [blank] + labels padded
    # with blank, int32 targets, t_len, u_len - built on the device (tavsr_lm_shift: x = [blank] + labels, 0 = blank behind them)
    def _calc_transducer_loss(self, encoder_out, encoder_out_lens, text, text_lengths):
        if self.blank_id != 0:
            raise ValueError("the transducer branch takes <blank> at id 0 (the embedding's padding row and the label padding)")
        u_len = text_lengths.to(torch.int64).contiguous()
        decoder_in, target, _, _ = ops.lm_shift(text.contiguous(), u_len, self.blank_id)
        target = target[:, : text.shape[1]].to(torch.int32)
        t_len = encoder_out_lens.to(torch.int64).contiguous()
        self.decoder.set_device(encoder_out.device)
        decoder_out = self.decoder(decoder_in)
        return F_.grad_apply(RNNTLossFn, encoder_out, decoder_out, t_len, u_len, target, dict(blank=self.blank_id),
                             *self.joint_network.params())

    @torch.no_grad()
    def ctc_greedy(self, speech, speech_lengths):
        """-> (ids (B,T), hyp (B,T) padded -1, hyp_len (B)): argmax + collapse, integer exact."""
        enc, olens = self.encode(speech, speech_lengths)
        return self.ctc.greedy(enc, olens, self.blank_id)

    @torch.no_grad()
    def align(self, *batch):
        """(*encode's tensors, text, text_lengths) -> (align (B,T) int64, frame_lp (B,T), span (B,Lmax,2) int32, score (B),
        encoder_out_lens): the CTC forced alignment of every utterance to its transcript (``CTC.forced_align``; frames are the
        encoder's).  ``text`` (B,Lmax) is read up to ``text_lengths``; its padding may hold anything."""
        *inputs, text, text_lengths = batch
        if self.ctc is None:
            raise ValueError("align needs the CTC head: this model was built without one (ctc_weight: 0.0)")
        enc, olens = self.encode(*inputs)
        if isinstance(enc, tuple):
            enc = enc[0]
        return self.ctc.forced_align(enc, olens, text, text_lengths, self.blank_id) + (olens,)


class _Accuracy:
    """Lazy th_accuracy: the reference returns a Python float (a device->host sync, nets_utils.th_accuracy);
    the counters stay on the device until somebody asks."""

    def __init__(self, correct):
        self.correct = correct

    def __float__(self):
        c = self.correct
        return float((c == 1).sum()) / float((c >= 0).sum())
