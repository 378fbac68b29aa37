"""Host (no GPU): the Conformer classes' construction, state_dict keys, registry, recipe and refusals, and the restated
GLU + depthwise convolution (tests/conformer_ref.py) against torch.autograd in float64."""
import argparse
import os

import pytest
import torch
import yaml

import conformer_ref as R
from helpers import ROOT

CONFORMER_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "conformer", "asr_conformer_transformer_ctc_english.yaml")


def _expected_keys(D, H, units, K, nb, macaron, conv, in_dim=80):
    """{key: shape}: espnet's names (conformer/encoder_layer.py, conformer/convolution.py) for a conv2d-embedded encoder"""
    f = ((in_dim - 1) // 2 - 1) // 2
    keys = {"embed.conv.0.weight": (D, 1, 3, 3), "embed.conv.0.bias": (D,), "embed.conv.2.weight": (D, D, 3, 3),
            "embed.conv.2.bias": (D,), "embed.out.0.weight": (D, D * f), "embed.out.0.bias": (D,),
            "after_norm.weight": (D,), "after_norm.bias": (D,)}
    for i in range(nb):
        lay = {}
        for c in "qkv":
            lay[f"self_attn.linear_{c}.weight"], lay[f"self_attn.linear_{c}.bias"] = (D, D), (D,)
        lay.update({"self_attn.linear_out.weight": (D, D), "self_attn.linear_out.bias": (D,), "self_attn.linear_pos.weight": (D, D),
                    "self_attn.pos_bias_u": (H, D // H), "self_attn.pos_bias_v": (H, D // H)})
        if conv:
            lay.update({"conv_module.pointwise_conv1.weight": (2 * D, D, 1), "conv_module.pointwise_conv1.bias": (2 * D,),
                        "conv_module.depthwise_conv.weight": (D, 1, K), "conv_module.depthwise_conv.bias": (D,),
                        "conv_module.norm.weight": (D,), "conv_module.norm.bias": (D,), "conv_module.norm.running_mean": (D,),
                        "conv_module.norm.running_var": (D,), "conv_module.norm.num_batches_tracked": (),
                        "conv_module.pointwise_conv2.weight": (D, D, 1), "conv_module.pointwise_conv2.bias": (D,)})
        norms = ["norm_ff", "norm_mha"] + (["norm_ff_macaron"] if macaron else []) + (["norm_conv", "norm_final"] if conv else [])
        for n in norms:
            lay[n + ".weight"], lay[n + ".bias"] = (D,), (D,)
        for ff in ["feed_forward"] + (["feed_forward_macaron"] if macaron else []):
            lay.update({f"{ff}.w_1.weight": (units, D), f"{ff}.w_1.bias": (units,), f"{ff}.w_2.weight": (D, units), f"{ff}.w_2.bias": (D,)})
        keys.update({f"encoders.{i}.{n}": s for n, s in lay.items()})
    return keys


@pytest.mark.parametrize("macaron,conv", [(False, False), (True, False), (False, True), (True, True)])
def test_state_dict_keys_and_shapes(macaron, conv):
    from tavsr import functional_conformer as FC_
    from tavsr.encoder.conformer import ConformerEncoder, ConvolutionModule, EncoderLayer
    kw = dict(input_size=80, output_size=64, attention_heads=2, linear_units=96, num_blocks=2, macaron_style=macaron,
              use_cnn_module=conv, cnn_module_kernel=7, rel_pos_type="latest")
    enc = ConformerEncoder(**kw)
    assert enc.output_size() == 64 and all(isinstance(l, EncoderLayer) for l in enc.encoders)
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == _expected_keys(64, 2, 96, 7, 2, macaron, conv)
    lay = enc.encoders[0]
    assert lay.ff_scale == (0.5 if macaron else 1.0)
    assert hasattr(lay, "norm_conv") == hasattr(lay, "norm_final") == conv and hasattr(lay, "norm_ff_macaron") == macaron
    assert isinstance(lay.conv_module, ConvolutionModule) == conv
    # the layer's own parameter list is complete: every parameter of the module, None only for an absent block
    P = dict(zip(FC_.CONFORMER_PARAM_NAMES, lay._params()))
    assert {n for n, p in P.items() if p is not None} == {n for n, _ in lay.named_parameters()}
    # the reference restatement names its parameters alike: its state_dict loads key for key
    ref = R.ConformerEncoderRef(**kw)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == got
    enc.load_state_dict(ref.state_dict(), strict=True)


def test_branchformer_parameter_lists_are_untouched():
    from tavsr import functional as F_
    assert not any("conv_module" in n or "self_attn" in n for n in F_.EBF_PARAM_NAMES)
    assert F_.EBF_PARAM_NAMES[:len(F_.BF_PARAM_NAMES)] == F_.BF_PARAM_NAMES and len(F_.BF_PARAM_NAMES) == 47


def test_conditioning_layer_key_and_task_registry():
    from helpers import asr_conf
    from tavsr.encoder.conformer import ConformerEncoder
    from tavsr.tasks.asr import ASRTask, encoder_choices
    assert encoder_choices["conformer"] is ConformerEncoder
    conf = asr_conf(num_blocks=2, dec_blocks=1)
    conf["encoder"] = "conformer"
    conf["encoder_conf"] = dict(output_size=64, attention_heads=2, num_blocks=2, macaron_style=True, linear_units=96, cnn_module_kernel=3,
                                rel_pos_type="latest", interctc_layer_idx=[1], interctc_use_conditioning=True)
    conf["model_conf"]["interctc_weight"] = 0.3
    model = ASRTask.build_model(argparse.Namespace(**conf))
    assert isinstance(model.encoder, ConformerEncoder)
    sd = model.state_dict()
    V = sd["ctc.ctc_lo.weight"].shape[0]
    assert tuple(sd["encoder.conditioning_layer.weight"].shape) == (64, V) and "encoder.conditioning_layer.bias" in sd
    enc_keys = {k.split(".")[1] for k in sd if k.startswith("encoder.")}
    assert enc_keys == {"embed", "encoders", "after_norm", "conditioning_layer"}


def test_recipe_loads_and_builds():
    from tavsr.encoder.conformer import ConformerEncoder
    from tavsr.tasks.asr import ASRTask
    conf = yaml.safe_load(open(CONFORMER_YAML))
    base = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_transformer_ctc_english.yaml")))
    assert set(conf) == set(base) and conf["encoder"] == "conformer"
    assert {k: v for k, v in conf.items() if k not in ("encoder", "encoder_conf")} == \
           {k: v for k, v in base.items() if k not in ("encoder", "encoder_conf")}
    ec = conf["encoder_conf"]
    assert (ec["macaron_style"], ec["use_cnn_module"], ec["cnn_module_kernel"], ec["rel_pos_type"], ec["activation_type"],
            ec["num_blocks"], ec["linear_units"]) == (True, True, 31, "latest", "swish", 12, 2048)
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"]["num_blocks"] = 2
    conf["decoder_conf"]["num_blocks"] = 1
    model = ASRTask.build_model(argparse.Namespace(**conf))
    assert isinstance(model.encoder, ConformerEncoder) and len(model.encoder.encoders) == 2
    lay = model.encoder.encoders[0]
    assert tuple(lay.conv_module.depthwise_conv.weight.shape) == (256, 1, 31) and lay.ff_scale == 0.5


REFUSALS = [("rel_pos_type", "legacy"), ("pos_enc_layer_type", "abs_pos"), ("selfattention_layer_type", "selfattn"),
            ("positionwise_layer_type", "conv1d"), ("normalize_before", False), ("concat_after", True),
            ("stochastic_depth_rate", 0.1), ("stochastic_depth_rate", [0.0, 0.1]), ("layer_drop_rate", 0.1), ("zero_triu", True),
            ("input_layer", "conv2d6"), ("cnn_module_kernel", 4), ("cnn_module_kernel", 33)]


@pytest.mark.parametrize("option,value", REFUSALS, ids=[f"{o}={v}" for o, v in REFUSALS])
def test_refusals_name_their_option(option, value):
    from tavsr.encoder.conformer import ConformerEncoder
    kw = dict(input_size=80, output_size=64, attention_heads=2, linear_units=96, num_blocks=2, rel_pos_type="latest")
    kw[option] = value
    with pytest.raises(ValueError, match=option):
        ConformerEncoder(**kw)


def test_default_construction_is_refused_and_names_the_way_out():
    """espnet's default rel_pos_type is 'legacy': it stays the default here and is refused, with the option to set in the message"""
    from tavsr.encoder.conformer import ConformerEncoder
    with pytest.raises(ValueError, match="rel_pos_type: latest"):
        ConformerEncoder(input_size=80)


def test_module_and_layer_refusals_and_cache():
    from tavsr.encoder.conformer import ConformerEncoder, ConvolutionModule, EncoderLayer
    for K in (4, 33):
        with pytest.raises(ValueError, match="cnn_module_kernel"):
            ConvolutionModule(64, K, "swish")
    enc = ConformerEncoder(input_size=80, output_size=64, attention_heads=2, linear_units=96, num_blocks=1, rel_pos_type="latest")
    lay = enc.encoders[0]
    for kw in (dict(normalize_before=False), dict(concat_after=True), dict(stochastic_depth_rate=0.1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            EncoderLayer(64, lay.self_attn, lay.feed_forward, None, None, 0.1, **kw)
    x = (torch.zeros(1, 4, 64), torch.zeros(1, 7, 64))
    with pytest.raises(NotImplementedError):
        lay(x, None, cache=torch.zeros(1))


@pytest.mark.parametrize("K", [1, 3, 31])
def test_restated_glu_dwconv_backward_agrees_with_autograd_in_float64(K):
    torch.manual_seed(K)
    B, T, C = 3, 17, 10
    h = torch.randn(B, T, 2 * C, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, K, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(B, T, C, dtype=torch.float64)
    z = R.glu_dwconv(h, w, b)
    assert torch.allclose(R.glu_dwconv_restated(h, w, b), z, rtol=1e-12, atol=1e-12)
    gh, gw, gb = torch.autograd.grad(z, (h, w, b), dz)
    dh, dw, db = R.glu_dwconv_bwd_restated(dz, h.detach(), w.detach())
    for got, want in ((dh, gh), (dw, gw), (db, gb)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()) + 1e-13
