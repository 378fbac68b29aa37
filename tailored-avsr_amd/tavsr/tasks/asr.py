"""``ASRTask.build_model`` - drop-in for src/tasks/asr.py:482-619: same YAML keys, string registries
restricted to the classes on the hot path (anything else raises ValueError naming the key)."""
from __future__ import annotations

import argparse

from ..ctc.ctc import CTC
from ..decoder.joint_network import JointNetwork
from ..decoder.mlm_decoder import MLMDecoder
from ..decoder.transducer_decoder import TransducerDecoder
from ..decoder.transformer_decoder import TransformerDecoder
from ..encoder.branchformer.encoder import MyBranchformerEncoder
from ..encoder.conformer.encoder import ConformerEncoder
from ..encoder.e_branchformer.encoder import EBranchformerEncoder
from ..frontend.conv3d_resnet18 import Conv3dResNet18
from ..frontend.default import DefaultFrontend
from ..models.espnet_model import ESPnetASRModel, UtteranceMVN
from ..models.maskctc_model import MaskCTCModel
from ..specaug.specaug import SpecAug
from ..utils.tokens import load_token_list

frontend_choices = {"default": DefaultFrontend, "conv3dresnet18": Conv3dResNet18}      # src/tasks/asr.py:93-103
specaug_choices = {"specaug": SpecAug}
encoder_choices = {"conformer": ConformerEncoder, "branchformer": MyBranchformerEncoder,      # src/tasks/asr.py:148,161-162
                   "e_branchformer": EBranchformerEncoder}
decoder_choices = {"transformer": TransformerDecoder, "mlm": MLMDecoder, "transducer": TransducerDecoder}
normalize_choices = {"utterance_mvn": UtteranceMVN}
model_choices = {"espnet": ESPnetASRModel, "maskctc": MaskCTCModel}


def _pick(table, name, what):
    if name not in table:
        raise ValueError(f"--{what} must be one of {tuple(table)}: {name}")
    return table[name]


def build_decoder(args, choices, vocab_size, encoder, encoder_output_size):
    """-> (decoder, joint_network): src/tasks/asr.py:556-581 == src/tasks/avsr.py:654-680.  ``decoder: transducer`` takes the
    vocabulary size and ``embed_pad=0`` and comes with a joint network built from ``joint_net_conf``."""
    if getattr(args, "decoder", None) is None:
        return None, None
    decoder_class = _pick(choices, args.decoder, "decoder")
    if args.decoder == "transducer":
        decoder = decoder_class(vocab_size, embed_pad=0, **args.decoder_conf)
        joint = JointNetwork(vocab_size, encoder.output_size(), decoder.dunits, **(getattr(args, "joint_net_conf", None) or {}))
        return decoder, joint
    return decoder_class(vocab_size=vocab_size, encoder_output_size=encoder_output_size, **args.decoder_conf), None


class ASRTask:
    @classmethod
    def build_model(cls, args: argparse.Namespace) -> ESPnetASRModel:
        token_list = load_token_list(args.token_list)
        args.token_list = list(token_list)
        vocab_size = len(token_list)
        if args.input_size is None:       # waveform in: the log-mel frontend is part of the model (src/tasks/asr.py:500-512)
            frontend = _pick(frontend_choices, getattr(args, "frontend", "default"), "frontend")(
                **(getattr(args, "frontend_conf", None) or {}))
            input_size = frontend.output_size()
        else:
            frontend, input_size = None, args.input_size
        specaug = None
        if getattr(args, "specaug", None) is not None:
            specaug = _pick(specaug_choices, args.specaug, "specaug")(**(getattr(args, "specaug_conf", None) or {}))
        normalize = None
        if getattr(args, "normalize", None) is not None:
            normalize = _pick(normalize_choices, args.normalize, "normalize")(**(args.normalize_conf or {}))
        encoder = _pick(encoder_choices, args.encoder, "encoder")(input_size=input_size, **args.encoder_conf)
        decoder, joint_network = build_decoder(args, decoder_choices, vocab_size, encoder, encoder.output_size())
        ctc = CTC(odim=vocab_size, encoder_output_size=encoder.output_size(), **args.ctc_conf)
        model_class = model_choices.get(getattr(args, "model", "espnet"), ESPnetASRModel)
        model = model_class(vocab_size=vocab_size, frontend=frontend, specaug=specaug, normalize=normalize,
                            preencoder=None, encoder=encoder, postencoder=None, decoder=decoder, ctc=ctc,
                            joint_network=joint_network, token_list=token_list, **args.model_conf)
        if getattr(args, "init", None) is not None:
            raise NotImplementedError("init: null in every shipped config")
        return model
