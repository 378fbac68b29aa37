"""``AVSRMaskCTCModel`` / ``AVSRMaskCTCInference`` - drop-in for src/models/avsr_maskctc_model.py:44-370: the audio-visual
encoder of ``ESPnetAVSRModel`` with the Mask-CTC decoder branch and decoding of ``maskctc_model.py`` (one implementation)."""
from __future__ import annotations

from typing import List, Tuple, Union

from ..ctc.ctc import CTC
from .avsr_espnet_model import ESPnetAVSRModel
from .maskctc_model import MaskCTCInference, _MaskCTCMixin


class AVSRMaskCTCModel(_MaskCTCMixin, ESPnetAVSRModel):
    def __init__(self, vocab_size: int, token_list: Union[Tuple[str, ...], List[str]], specaug, normalize,
                 acoustic_frontend, visual_frontend, acoustic_preencoder, visual_preencoder, acoustic_embed, visual_embed,
                 encoder, audiovisual_fusion, postencoder, decoder, ctc: CTC, joint_network=None, ctc_weight: float = 0.5,
                 interctc_weight: float = 0.0, ignore_id: int = -1, lsm_weight: float = 0.0,
                 length_normalized_loss: bool = False, report_cer: bool = True, report_wer: bool = True,
                 sym_space: str = "<space>", sym_blank: str = "<blank>", sym_mask: str = "<mask>",
                 extract_feats_in_collect_stats: bool = True):
        super().__init__(vocab_size=vocab_size, token_list=token_list, specaug=specaug, normalize=normalize,
                         acoustic_frontend=acoustic_frontend, visual_frontend=visual_frontend,
                         acoustic_preencoder=acoustic_preencoder, visual_preencoder=visual_preencoder,
                         acoustic_embed=acoustic_embed, visual_embed=visual_embed, encoder=encoder,
                         audiovisual_fusion=audiovisual_fusion, postencoder=postencoder, decoder=decoder, ctc=ctc,
                         joint_network=joint_network, ctc_weight=ctc_weight, interctc_weight=interctc_weight,
                         ignore_id=ignore_id, lsm_weight=lsm_weight, length_normalized_loss=length_normalized_loss,
                         report_cer=report_cer, report_wer=report_wer, sym_space=sym_space, sym_blank=sym_blank,
                         extract_feats_in_collect_stats=extract_feats_in_collect_stats)
        self._init_mlm(token_list, sym_mask, sym_space, sym_blank, report_cer, report_wer)


class AVSRMaskCTCInference(MaskCTCInference):
    """avsr_maskctc_model.py:283-370: the same loop on the fused audio-visual encoder output"""
