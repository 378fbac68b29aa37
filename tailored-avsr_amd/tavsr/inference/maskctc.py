"""``Speech2TextMaskCTC`` - src/inference/{asr,avsr}_inference_maskctc.py:Speech2Text for models that are already built:
encode + Mask-CTC decoding, results per utterance as the reference returns them (:130-143):
``[(text, tokens, token ids without the frame and without id 0, hypothesis)]``."""
from __future__ import annotations

import torch

from ..models.maskctc_model import Hypothesis, MaskCTCInference
from .beam_search import CapturedEncode


class Speech2TextMaskCTC:
    def __init__(self, asr_model, maskctc_n_iterations: int = 10, maskctc_threshold_probability: float = 0.99):
        self.asr_model = asr_model.eval()
        self.s2t = MaskCTCInference(asr_model=self.asr_model, n_iterations=maskctc_n_iterations,
                                    threshold_probability=maskctc_threshold_probability)
        self.encode = CapturedEncode(self.asr_model)

    @torch.no_grad()
    def __call__(self, *batch):
        """batch: the tensors of ``asr_model.encode`` (speech, lengths) or (audio, lengths, video, lengths)."""
        enc, enc_lens = self.encode(*batch)
        if isinstance(enc, tuple):
            enc = enc[0]
        results = []
        for yseq in self.s2t.decode(enc, enc_lens):
            token_int = [t for t in yseq[1:-1] if t != 0]
            token = [self.asr_model.token_list[t] for t in token_int]
            hyp = Hypothesis(yseq=torch.tensor(yseq, device=enc.device))
            results.append([(self.s2t.ids2text(token_int), token, token_int, hyp)])
        return results
