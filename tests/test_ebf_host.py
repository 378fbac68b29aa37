"""Host (no GPU): the E-Branchformer classes' construction, state_dict keys, registry, recipe and refusals, and the restated
depthwise-add (tests/ebf_ref.py) against torch.autograd in float64."""
import argparse
import os

import pytest
import torch
import yaml

import ebf_ref as R
from helpers import ROOT

EBF_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "e_branchformer", "asr_e_branchformer_transformer_ctc_english.yaml")


def _expected_keys(D, H, cg_units, cg_kernel, units, k, nb, use_ffn, macaron, in_dim=80):
    """{key: shape}: espnet's names (e_branchformer_encoder.py) for a conv2d-embedded encoder"""
    f = ((in_dim - 1) // 2 - 1) // 2
    keys = {"embed.conv.0.weight": (D, 1, 3, 3), "embed.conv.0.bias": (D,), "embed.conv.2.weight": (D, D, 3, 3),
            "embed.conv.2.bias": (D,), "embed.out.0.weight": (D, D * f), "embed.out.0.bias": (D,),
            "after_norm.weight": (D,), "after_norm.bias": (D,)}
    for i in range(nb):
        lay = {}
        for c in "qkv":
            lay[f"attn.linear_{c}.weight"], lay[f"attn.linear_{c}.bias"] = (D, D), (D,)
        lay.update({"attn.linear_out.weight": (D, D), "attn.linear_out.bias": (D,), "attn.linear_pos.weight": (D, D),
                    "attn.pos_bias_u": (H, D // H), "attn.pos_bias_v": (H, D // H),
                    "cgmlp.channel_proj1.0.weight": (cg_units, D), "cgmlp.channel_proj1.0.bias": (cg_units,),
                    "cgmlp.csgu.norm.weight": (cg_units // 2,), "cgmlp.csgu.norm.bias": (cg_units // 2,),
                    "cgmlp.csgu.conv.weight": (cg_units // 2, 1, cg_kernel), "cgmlp.csgu.conv.bias": (cg_units // 2,),
                    "cgmlp.channel_proj2.weight": (D, cg_units // 2), "cgmlp.channel_proj2.bias": (D,),
                    "depthwise_conv_fusion.weight": (2 * D, 1, k), "depthwise_conv_fusion.bias": (2 * D,),
                    "merge_proj.weight": (D, 2 * D), "merge_proj.bias": (D,)})
        norms = ["norm_mha", "norm_mlp", "norm_final"] + (["norm_ff"] if use_ffn else []) + (["norm_ff_macaron"] if macaron else [])
        for n in norms:
            lay[n + ".weight"], lay[n + ".bias"] = (D,), (D,)
        for ff in (["feed_forward"] if use_ffn else []) + (["feed_forward_macaron"] if macaron else []):
            lay.update({f"{ff}.w_1.weight": (units, D), f"{ff}.w_1.bias": (units,), f"{ff}.w_2.weight": (D, units), f"{ff}.w_2.bias": (D,)})
        keys.update({f"encoders.{i}.{n}": s for n, s in lay.items()})
    return keys


@pytest.mark.parametrize("use_ffn,macaron", [(False, False), (True, False), (True, True)])
def test_state_dict_keys_and_shapes(use_ffn, macaron):
    from tavsr.encoder.e_branchformer import EBranchformerEncoder, EBranchformerEncoderLayer
    kw = dict(input_size=80, output_size=64, attention_heads=2, cgmlp_linear_units=128, cgmlp_conv_kernel=7, num_blocks=2,
              use_ffn=use_ffn, macaron_ffn=macaron, linear_units=96, merge_conv_kernel=5)
    enc = EBranchformerEncoder(**kw)
    assert enc.output_size() == 64 and all(isinstance(l, EBranchformerEncoderLayer) for l in enc.encoders)
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == _expected_keys(64, 2, 128, 7, 96, 5, 2, use_ffn, macaron)
    assert enc.encoders[0].ff_scale == (0.5 if macaron else 1.0)
    # the reference restatement names its parameters alike: its state_dict loads key for key
    ref = R.EBranchformerEncoderRef(**kw)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == got
    enc.load_state_dict(ref.state_dict())


def test_conditioning_layer_key_and_task_registry():
    from helpers import asr_conf
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    from tavsr.tasks.asr import ASRTask, encoder_choices
    assert encoder_choices["e_branchformer"] is EBranchformerEncoder
    conf = asr_conf(num_blocks=2, dec_blocks=1)
    conf["encoder"] = "e_branchformer"
    conf["encoder_conf"] = dict(output_size=64, attention_heads=2, cgmlp_linear_units=128, cgmlp_conv_kernel=7, num_blocks=2,
                                use_ffn=True, macaron_ffn=True, linear_units=96, merge_conv_kernel=3, interctc_layer_idx=[1],
                                interctc_use_conditioning=True)
    conf["model_conf"]["interctc_weight"] = 0.3
    model = ASRTask.build_model(argparse.Namespace(**conf))
    assert isinstance(model.encoder, EBranchformerEncoder)
    sd = model.state_dict()
    V = len(conf["token_list"]) if isinstance(conf["token_list"], list) else sd["ctc.ctc_lo.weight"].shape[0]
    assert tuple(sd["encoder.conditioning_layer.weight"].shape) == (64, V) and "encoder.conditioning_layer.bias" in sd
    enc_keys = {k.split(".")[1] for k in sd if k.startswith("encoder.")}
    assert enc_keys == {"embed", "encoders", "after_norm", "conditioning_layer"}


def test_recipe_loads_and_builds():
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    from tavsr.tasks.asr import ASRTask
    conf = yaml.safe_load(open(EBF_YAML))
    base = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_transformer_ctc_english.yaml")))
    assert set(conf) == set(base) and conf["encoder"] == "e_branchformer"
    assert {k: v for k, v in conf.items() if k not in ("encoder", "encoder_conf")} == \
           {k: v for k, v in base.items() if k not in ("encoder", "encoder_conf")}
    ec = conf["encoder_conf"]
    assert (ec["use_ffn"], ec["macaron_ffn"], ec["merge_conv_kernel"], ec["cgmlp_linear_units"], ec["linear_units"], ec["num_blocks"]) == \
           (True, True, 31, 1024, 1024, 12)
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"]["num_blocks"] = 2
    conf["decoder_conf"]["num_blocks"] = 1
    model = ASRTask.build_model(argparse.Namespace(**conf))
    assert isinstance(model.encoder, EBranchformerEncoder) and len(model.encoder.encoders) == 2
    lay = model.encoder.encoders[0]
    assert tuple(lay.depthwise_conv_fusion.weight.shape) == (512, 1, 31) and lay.ff_scale == 0.5


REFUSALS = [("rel_pos_type", "legacy"), ("pos_enc_layer_type", "abs_pos"), ("attention_layer_type", "selfattn"),
            ("positionwise_layer_type", "conv1d"), ("input_layer", "conv2d6"), ("layer_drop_rate", 0.1), ("merge_conv_kernel", 4),
            ("merge_conv_kernel", 33),
            ("use_linear_after_conv", True), ("gate_activation", "swish"), ("zero_triu", True)]


@pytest.mark.parametrize("option,value", REFUSALS, ids=[f"{o}={v}" for o, v in REFUSALS])
def test_refusals_name_their_option(option, value):
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    with pytest.raises(ValueError, match=option):
        EBranchformerEncoder(input_size=80, output_size=64, attention_heads=2, cgmlp_linear_units=128, num_blocks=1, **{option: value})


def test_macaron_without_ffn_and_cache_are_refused():
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    with pytest.raises(ValueError, match="macaron_ffn"):
        EBranchformerEncoder(input_size=80, output_size=64, attention_heads=2, cgmlp_linear_units=128, num_blocks=1, macaron_ffn=True)
    enc = EBranchformerEncoder(input_size=80, output_size=64, attention_heads=2, cgmlp_linear_units=128, num_blocks=1)
    x = (torch.zeros(1, 4, 64), torch.zeros(1, 7, 64))
    with pytest.raises(NotImplementedError):
        enc.encoders[0](x, None, cache=torch.zeros(1))


@pytest.mark.parametrize("K", [1, 3, 31])
def test_restated_depthwise_add_backward_agrees_with_autograd_in_float64(K):
    torch.manual_seed(K)
    B, T, C = 3, 17, 10
    x = torch.randn(B, T, C, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, K, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, dtype=torch.float64, requires_grad=True)
    du = torch.randn(B, T, C, dtype=torch.float64)
    u = R.dwconv_add(x, w, b)
    assert torch.allclose(R.dwconv_add_restated(x, w, b), u, rtol=1e-12, atol=1e-12)
    gx, gw, gb = torch.autograd.grad(u, (x, w, b), du)
    dx, dw, db = R.dwconv_add_bwd_restated(du, x.detach(), w.detach())
    for got, want in ((dx, gx), (dw, gw), (db, gb)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()) + 1e-13


def test_branchformer_layers_keep_a_complete_parameter_list():
    """the C-side layer backward (functional._layer_c_backward) runs only for a parameter list without ``None``: the E-Branchformer
    parameters live in a list of their own (EBF_PARAM_NAMES), so the recipe's Branchformer layer is still gathered complete"""
    from tavsr import functional as F_
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.encoder.e_branchformer import EBranchformerEncoder
    assert not any("depthwise_conv_fusion" in n for n in F_.BF_PARAM_NAMES)
    assert F_.EBF_PARAM_NAMES[:len(F_.BF_PARAM_NAMES)] == F_.BF_PARAM_NAMES
    bf = MyBranchformerEncoder(input_size=64, output_size=64, attention_heads=2, linear_units=96, cgmlp_linear_units=128, num_blocks=1,
                               input_layer=None).encoders[0]
    P = bf._params()
    assert len(P) == len(F_.BF_PARAM_NAMES) and all(p is not None for p in P)
    ebf = EBranchformerEncoder(input_size=64, output_size=64, attention_heads=2, linear_units=96, cgmlp_linear_units=128, num_blocks=1,
                               input_layer=None, use_ffn=True, macaron_ffn=True).encoders[0]
    got = dict(zip(F_.EBF_PARAM_NAMES, ebf._params()))
    assert len(got) == len(F_.EBF_PARAM_NAMES)
    assert {n for n, p in got.items() if p is not None} == {n for n, _ in ebf.named_parameters()}
    assert got["depthwise_conv_fusion.weight"] is ebf.depthwise_conv_fusion.weight
