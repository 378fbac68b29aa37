"""``build_speech2text`` - the ``config.model`` switch of src/utils/inference.py:6-27 for models that are already built."""
from __future__ import annotations

from ..inference import Speech2Text, Speech2TextMaskCTC


def build_speech2text(config, asr_model, lm=None):
    """``config``: the recipe (namespace or dict) with ``model`` and ``inference_conf``; one front end serves asr / vsr / avsr
    (its call takes the tensors of the model's own ``encode``)."""
    get = config.get if isinstance(config, dict) else lambda k, d=None: getattr(config, k, d)
    model, conf = get("model", "espnet"), dict(get("inference_conf") or {})
    conf.pop("batch_size", None)
    if model == "espnet":
        return Speech2Text(asr_model, lm, **conf)
    if model == "maskctc":
        return Speech2TextMaskCTC(asr_model, **conf)
    raise ValueError(f"unknown model architecture {model}")
