"""Which models the beam search accepts and with which scorers (espnet's BeamSearch drops a scorer that is None or has weight 0;
the reference hands it {decoder, ctc, length_bonus, lm}: src/inference/avsr_inference.py:141-153, 249-286).  Host only: a search object
is built on CPU models, nothing is decoded."""
import argparse

import pytest

from helpers import TOKENS_EN, asr_conf
from tavsr.inference.beam_search import BatchBeamSearch, Speech2Text
from tavsr.lm.transformer_lm import TransformerLM
from tavsr.tasks.asr import ASRTask

LM_KW = dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0)


def _model(model_ctc_weight=None):
    conf = asr_conf(num_blocks=1, dec_blocks=1)
    if model_ctc_weight is not None:
        conf["model_conf"]["ctc_weight"] = model_ctc_weight
    conf["token_list"] = TOKENS_EN
    return ASRTask.build_model(argparse.Namespace(**conf)).eval()


@pytest.fixture(scope="module")
def models():
    return dict(hybrid=_model(), ctc_only=_model(1.0), att_only=_model(0.0), lm=TransformerLM(len(TOKENS_EN), **LM_KW).eval())


def test_models_without_decoder_or_without_ctc_head_get_a_search(models):
    ctc_only, att_only, lm = models["ctc_only"], models["att_only"], models["lm"]
    assert ctc_only.decoder is None and ctc_only.ctc is not None
    assert att_only.ctc is None and att_only.decoder is not None
    s = BatchBeamSearch(ctc_only, None, beam_size=5, ctc_weight=1.0, lm_weight=0.0, penalty=0.5)
    assert s.scorers == ("ctc", "length_bonus") and s.dec_step is None and s.lm_step is None and not s.pre_beam
    s = BatchBeamSearch(ctc_only, lm, beam_size=5, ctc_weight=1.0, lm_weight=0.6, penalty=0.5)
    assert s.scorers == ("ctc", "length_bonus", "lm") and s.dec_step is None and not s.pre_beam
    s = BatchBeamSearch(ctc_only, lm, beam_size=5, ctc_weight=0.4, lm_weight=0.6, penalty=0.5)      # pre-beam on the LM's scores
    assert s.scorers == ("ctc", "length_bonus", "lm") and s.pre_beam and s.C == 7
    s = BatchBeamSearch(att_only, None, beam_size=5, ctc_weight=0.0, lm_weight=0.0, penalty=0.5)
    assert s.scorers == ("decoder", "length_bonus") and s.dec_step is not None and not s.pre_beam
    s = BatchBeamSearch(att_only, lm, beam_size=5, ctc_weight=0.3, lm_weight=0.6, penalty=0.5)      # no CTC head: its weight is moot
    assert s.scorers == ("decoder", "length_bonus", "lm")
    for m, w in ((ctc_only, 1.0), (att_only, 0.0)):
        s2t = Speech2Text(m, None, beam_size=5, ctc_weight=w, lm_weight=0.0, penalty=0.5)
        assert s2t.beam_search.scorers == (("ctc" if w else "decoder"), "length_bonus")


def test_the_two_combinations_without_a_sensible_search_are_refused(models):
    ctc_only, att_only, hybrid, lm = models["ctc_only"], models["att_only"], models["hybrid"], models["lm"]
    # (a) neither decoder nor CTC scorer is left
    with pytest.raises(ValueError, match="ctc_weight to 1.0"):
        BatchBeamSearch(ctc_only, None, 5, ctc_weight=0.0)
    with pytest.raises(ValueError, match="ctc_weight to 0.0"):
        BatchBeamSearch(att_only, lm, 5, ctc_weight=1.0)
    # (b) CTC scorer with a pre-beam, but neither decoder nor LM to rank the candidates
    with pytest.raises(ValueError, match="ctc_weight: 1.0"):
        BatchBeamSearch(ctc_only, None, 5, ctc_weight=0.3)
    with pytest.raises(ValueError, match="ctc_weight: 1.0"):
        BatchBeamSearch(ctc_only, lm, 5, ctc_weight=0.3, lm_weight=0.0)
    with pytest.raises(ValueError, match="ctc_weight: 1.0"):
        BatchBeamSearch(ctc_only, None, 5, ctc_weight=0.9, skip_zero_weight=True)
    # ... not refused: int(1.5 * beam) >= V leaves no pre-beam
    assert not BatchBeamSearch(ctc_only, None, 30, ctc_weight=0.3).pre_beam
    with pytest.raises(ValueError, match="ctc_weight must lie"):
        BatchBeamSearch(ctc_only, None, 5, ctc_weight=1.5)


@pytest.mark.parametrize("ctc_weight", [0.0, 0.3, 1.0])
def test_a_hybrid_model_keeps_its_scorers_unless_asked(models, ctc_weight):
    hybrid, lm = models["hybrid"], models["lm"]
    s = BatchBeamSearch(hybrid, lm, 5, ctc_weight, 0.6, 0.5)
    assert s.scorers == ("decoder", "ctc", "length_bonus", "lm") and s.dec_step is not None
    assert s.C == (len(TOKENS_EN) if ctc_weight == 1.0 else 7)
    assert BatchBeamSearch(hybrid, lm, 5, ctc_weight, 0.0, 0.5).scorers == ("decoder", "ctc", "length_bonus")
    t = BatchBeamSearch(hybrid, lm, 5, ctc_weight, 0.6, 0.5, skip_zero_weight=True)
    want = {0.0: ("decoder", "length_bonus", "lm"), 0.3: ("decoder", "ctc", "length_bonus", "lm"), 1.0: ("ctc", "length_bonus", "lm")}
    assert t.scorers == want[ctc_weight]
    assert (t.dec_step is None) == (ctc_weight == 1.0)
    s2t = Speech2Text(hybrid, lm, 5, ctc_weight, 0.6, 0.5, skip_zero_weight=True)
    assert s2t.beam_search.scorers == want[ctc_weight]
