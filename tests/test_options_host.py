"""CPU: the encoders' ``ffn_activation_type`` over espnet get_activation's whole set (hardtanh, tanh, relu, selu, swish;
src/encoder/branchformer/encoder.py:206, src/encoder/audiovisual/tailored/encoder.py:99) - construction, state_dict keys, the
C enum the Python table passes on, names outside the set, and the oracle against the reference's own layer
(tests/golden/bf_layer_ffn_*.npz, scripts/gen_golden_options.py)."""
import argparse
import os
import re

import pytest
import torch

from helpers import AVSR_CONV_YAML, AVSR_YAML, ROOT, asr_conf, avsr_conf, golden, grad_ok, max_rel, rel_err

NEW_ACTS = ("tanh", "hardtanh", "selu")


def test_act_table_matches_the_c_enum():
    from tavsr._lib import ACT
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"TAVSR_ACT_([A-Z]+) = (\d+)", hdr)}
    assert enum == {"none": 0, "relu": 1, "swish": 2, "gelu": 3, "tanh": 4, "hardtanh": 5, "selu": 6}
    for name, code in enum.items():
        assert ACT[name] == code, name


@pytest.mark.parametrize("act", ["hardtanh", "tanh", "relu", "selu", "swish"])
def test_every_encoder_takes_the_whole_set(act):
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.tasks.asr import ASRTask
    from tavsr.tasks.avsr import AVSRTask
    enc = MyBranchformerEncoder(input_size=80, num_blocks=2, input_layer="conv2d", ffn_activation_type=act)
    assert all(layer.feed_forward.activation == act and layer.feed_forward_macaron.activation == act for layer in enc.encoders)
    ASRTask.build_model(argparse.Namespace(**asr_conf(num_blocks=1, dec_blocks=1, ffn_activation_type=act)))
    m = AVSRTask.build_model(argparse.Namespace(**avsr_conf(AVSR_YAML, num_blocks=1, dec_blocks=1, ffn_activation_type=act)))
    assert m.encoder.encoders[0].feed_forward.activation == act
    conf = avsr_conf(AVSR_CONV_YAML, num_blocks=1, dec_blocks=1)
    for side in ("acoustic_encoder_conf", "visual_encoder_conf"):
        conf["encoder_conf"][side]["ffn_activation_type"] = act
    AVSRTask.build_model(argparse.Namespace(**conf))


@pytest.mark.parametrize("act", ["gelu", "sigmoid", "identity", "Tanh"])
def test_names_outside_the_set_still_raise(act):
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    with pytest.raises((ValueError, KeyError)):
        MyBranchformerEncoder(input_size=256, num_blocks=1, input_layer=None, ffn_activation_type=act)


def test_macaron_false_still_raises():
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    with pytest.raises(ValueError):
        MyBranchformerEncoder(input_size=256, num_blocks=1, input_layer=None, macaron=False)


def test_fusion_ffn_keeps_its_two_activations():
    from tavsr.audiovisual_fusion.adaptive_audiovisual_fusion import AdaptiveAudioVisualFusion
    with pytest.raises(ValueError):
        AdaptiveAudioVisualFusion(256, 256, activation_type="tanh")


@pytest.mark.parametrize("act", NEW_ACTS)
def test_state_dict_keys_equal_the_fixture(act):
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    g = golden(f"bf_layer_ffn_{act}")
    enc = MyBranchformerEncoder(input_size=int(g["D"]), num_blocks=1, input_layer=None, ffn_activation_type=act,
                                merge_method="learned_ave")
    assert sorted(enc.encoders[0].state_dict().keys()) == list(g["keys"])


@pytest.mark.parametrize("act", NEW_ACTS)
def test_oracle_layer_matches_reference(act):
    from oracle import leaves as L
    from oracle.model import BranchformerEncoderOracle, compact, fill_parameters_, synth
    g = golden(f"bf_layer_ffn_{act}")
    B, T, D = int(g["B"]), int(g["T"]), int(g["D"])
    enc = BranchformerEncoderOracle(input_size=D, num_blocks=1, input_layer=None, dropout_rate=0.0, positional_dropout_rate=0.0,
                                    attention_dropout_rate=0.0, ffn_activation_type=act, merge_method="learned_ave")
    layer = enc.encoders[0].train()
    assert sorted(layer.state_dict().keys()) == list(g["keys"])
    fill_parameters_(layer, seed=21)
    lens = torch.from_numpy(g["lens"])
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, None, :]
    x = synth((B, T, D), seed=22).requires_grad_(True)
    xs, pos = L.RelPositionalEncoding(D, 0.0)(x)
    (y, _), _ = layer((xs, pos), mask)
    (y * synth((B, T, D), seed=23)).sum().backward()
    assert max_rel(y, g["y"]) < 2e-5
    assert rel_err(x.grad, g["grad_x"]) < 1e-4
    for n, p in layer.named_parameters():
        if "g_" + n in g.files:
            assert grad_ok(compact(p.grad), g["g_" + n], 1e-4), n
    assert rel_err(layer.weight_global, g["weight_global"]) < 1e-5
