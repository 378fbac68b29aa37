"""Host (no GPU): the Branchformer encoder's attention_layer_type / pos_enc_layer_type options - construction, state_dict keys,
refusals, the recipe - and properties of the restatement in tests/fastattn_ref.py."""
import argparse
import os

import pytest
import torch
import yaml

import fastattn_ref as R
from helpers import ROOT, TOKENS_EN

FAST_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "branchformer_fast", "asr_branchformer_fast_transformer_ctc_english.yaml")
PAIRS = [("abs_pos", "selfattn"), ("scaled_abs_pos", "selfattn"), ("abs_pos", "fast_selfattn"), ("scaled_abs_pos", "fast_selfattn"),
         ("rel_pos", "rel_selfattn")]


def _kw(input_layer, pos, attn):
    return dict(input_size=80, output_size=64, attention_heads=4, linear_units=96, num_blocks=2, cgmlp_linear_units=128,
                cgmlp_conv_kernel=7, input_layer=input_layer, pos_enc_layer_type=pos, attention_layer_type=attn)


def _attn_keys(attn, D, H):
    if attn == "fast_selfattn":
        keys = {f"attn.{m}.{w}": s for m, n in (("query", D), ("key", D), ("transform", D), ("query_att", H), ("key_att", H))
                for w, s in (("weight", (n, D)), ("bias", (n,)))}
        return keys
    keys = {f"attn.linear_{c}.{w}": s for c in ("q", "k", "v", "out") for w, s in (("weight", (D, D)), ("bias", (D,)))}
    if attn == "rel_selfattn":
        keys.update({"attn.linear_pos.weight": (D, D), "attn.pos_bias_u": (H, D // H), "attn.pos_bias_v": (H, D // H)})
    return keys


@pytest.mark.parametrize("pos,attn", PAIRS)
@pytest.mark.parametrize("input_layer", ["conv2d", "linear", "conv3dresnet18"])
def test_accepted_combinations_build_with_the_reference_keys(input_layer, pos, attn):
    from tavsr import layers
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    D, H = 64, 4
    enc = MyBranchformerEncoder(**_kw(input_layer, pos, attn))
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    a0 = {k[len("encoders.0."):]: s for k, s in got.items() if k.startswith("encoders.0.attn.")}
    assert a0 == _attn_keys(attn, D, H)
    want_cls = {"fast_selfattn": layers.FastSelfAttention, "selfattn": layers.MultiHeadedAttention,
                "rel_selfattn": layers.RelPositionMultiHeadedAttention}[attn]
    assert all(type(l.attn) is want_cls for l in enc.encoders)
    alpha = {"conv2d": "embed.out.1.alpha", "linear": "embed.3.alpha", "conv3dresnet18": "embed.1.alpha"}[input_layer]
    assert [k for k in got if k.endswith(".alpha")] == ([alpha] if pos == "scaled_abs_pos" else [])
    if pos == "scaled_abs_pos":
        assert got[alpha] == () and float(enc.state_dict()[alpha]) == 1.0
    pe = enc.embed.out[1] if input_layer == "conv2d" else enc.embed[-1]
    assert type(pe) is {"abs_pos": layers.PositionalEncoding, "scaled_abs_pos": layers.ScaledPositionalEncoding,
                        "rel_pos": layers.RelPositionalEncoding}[pos]
    # the restatement names its parameters alike: its state_dict loads key for key
    ref = R.BranchformerEncoderRef(**_kw(input_layer, pos, attn))
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == got
    enc.load_state_dict(ref.state_dict(), strict=True)


@pytest.mark.parametrize("pos,attn", [("rel_pos", "selfattn"), ("rel_pos", "fast_selfattn"), ("abs_pos", "rel_selfattn"),
                                      ("scaled_abs_pos", "rel_selfattn"), ("legacy_rel_pos", "legacy_rel_selfattn"),
                                      ("legacy_rel_pos", "rel_selfattn"), ("rel_pos", "legacy_rel_selfattn"), ("abs_pos", "nonsense")])
def test_refused_combinations_name_both_options_and_the_accepted_pairs(pos, attn):
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    with pytest.raises(ValueError) as e:
        MyBranchformerEncoder(**_kw("conv2d", pos, attn))
    msg = str(e.value)
    assert repr(pos) in msg and repr(attn) in msg
    for a, b in PAIRS:
        assert f"({a}, {b})" in msg


def test_legacy_rel_pos_type_and_the_other_encoders_stay_refused():
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    with pytest.raises(ValueError, match="legacy rel_pos is not on the HIP path"):
        MyBranchformerEncoder(rel_pos_type="legacy")
    with pytest.raises(ValueError, match="legacy rel_pos is not on the HIP path"):
        MyBranchformerEncoder(rel_pos_type="legacy", pos_enc_layer_type="abs_pos", attention_layer_type="fast_selfattn")


def test_fast_self_attention_constructor():
    from tavsr import ops
    from tavsr.layers import FastSelfAttention
    with pytest.raises(ValueError, match="not an integer multiple of attention heads"):
        FastSelfAttention(66, 4, 0.0)
    with pytest.raises(ValueError, match="not an integer multiple of attention heads"):
        R.FastSelfAttentionRef(66, 4, 0.0)
    # outside the kernels' range: refused at construction, in the words of the limit
    for size, heads in ((72, 12), (516, 4), (60, 6), (1024, 4)):
        assert not ops.fastattn_ok(size, heads)
        with pytest.raises(ValueError) as e:
            FastSelfAttention(size, heads, 0.0)
        assert ops.FASTATTN_LIMIT in str(e.value) and str(size) in str(e.value)
    for size, heads in ((64, 4), (256, 4), (64, 8), (96, 4), (256, 1), (512, 8)):
        assert ops.fastattn_ok(size, heads)
    m = FastSelfAttention(64, 4, 0.1)
    m.espnet_initialization_fn()
    assert all(float(p.detach().abs().max()) == 0.0 for n, p in m.named_parameters() if n.endswith("bias"))
    assert all(0.01 < float(p.detach().std()) < 0.03 for n, p in m.named_parameters() if n.endswith("weight"))


def test_layer_takes_the_form_its_attention_needs():
    from tavsr import layers as M
    from tavsr.encoder.branchformer.encoder_layer import MyBranchformerEncoderLayer
    ffn = lambda: M.PositionwiseFeedForward(64, 96, 0.0, "swish")
    cg = lambda: M.ConvolutionalGatingMLP(64, 128, 7, 0.0, False, "identity")
    fast = MyBranchformerEncoderLayer(64, M.FastSelfAttention(64, 4, 0.0), cg(), ffn(), ffn(), 0.0, "learned_ave")
    rel = MyBranchformerEncoderLayer(64, M.RelPositionMultiHeadedAttention(4, 64, 0.0), cg(), ffn(), ffn(), 0.0, "learned_ave")
    plain = MyBranchformerEncoderLayer(64, M.MultiHeadedAttention(4, 64, 0.0), cg(), ffn(), ffn(), 0.0, "learned_ave")
    assert (fast._attn_kind(), rel._attn_kind(), plain._attn_kind()) == ("fast_selfattn", "rel_selfattn", "selfattn")
    x = torch.zeros(1, 3, 64)
    with pytest.raises(ValueError, match="tensor x alone"):
        fast((x, x), None)
    with pytest.raises(ValueError, match="x_input = \\(x, pos_emb\\)"):
        rel(x, None)
    from tavsr import functional as F_
    assert len(F_.FAST_PARAM_NAMES) == len(F_.BF_PARAM_NAMES) - 1 and set(F_.FAST_ATTN_PARAMS) <= set(F_.FAST_PARAM_NAMES)
    assert [n for n in fast._params() if n is None] == [] and len(fast._params()) == len(F_.FAST_PARAM_NAMES)
    assert F_.BF_PARAM_NAMES.index("norm_mlp.weight") - F_.BF_PARAM_NAMES.index("norm_mha.bias") == 12      # the C descriptor's list is as it was


# ------------------------------------------------------------------------------------------------ the restatement
def _module(D=64, H=4, seed=0, dt=torch.float64):
    torch.manual_seed(seed)
    m = R.FastSelfAttentionRef(D, H, 0.0).to(dt)
    for p in m.parameters():
        p.data.normal_(0, 0.3)
    return m


def _mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, None, :]


def test_restatement_valid_rows_ignore_padded_input_frames():
    m = _module()
    T, lens = 9, (9, 5, 1)
    x = torch.randn(3, T, 64, dtype=torch.float64)
    x2 = x.clone()
    for b, n in enumerate(lens):
        x2[b, n:] = torch.randn(T - n, 64, dtype=torch.float64) * 7
    y, y2 = m(x, _mask(lens, T)), m(x2, _mask(lens, T))
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :n], y2[b, :n])
        assert n == T or not torch.equal(y[b, n:], y2[b, n:])      # the padded rows are computed from what is there


def test_restatement_no_mask_is_a_full_length_mask():
    m = _module(seed=1)
    x = torch.randn(2, 7, 64, dtype=torch.float64)
    assert torch.equal(m(x, None), m(x, _mask((7, 7), 7)))


def test_restatement_single_frame_is_transform_of_k_q_q():
    m = _module(seed=2)
    x = torch.randn(3, 1, 64, dtype=torch.float64)
    q, k = m.query(x), m.key(x)
    torch.testing.assert_close(m(x, _mask((1, 1, 1), 1)), m.transform(k * q * q) + q, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D,H,T", [(64, 4, 1), (64, 8, 17), (96, 4, 33)])
def test_kernel_formulas_are_the_module(D, H, T):
    """``fast_core`` (what csrc/fastattn.hip computes, by its formulas) between the module's projections is the module"""
    m = _module(D, H, seed=3)
    lens = (T, max(1, T // 2), 1)
    x = torch.randn(3, T, D, dtype=torch.float64)
    q, k = m.query(x), m.key(x)
    wv, alpha, beta, pq, pk = R.fast_core(q, k, m.query_att.weight, m.query_att.bias, m.key_att.weight, m.key_att.bias, torch.tensor(lens), H)
    torch.testing.assert_close(m.transform(wv) + q, m(x, _mask(lens, T)), rtol=1e-10, atol=1e-10)
    for b, n in enumerate(lens):
        assert float(alpha[b, :, n:].abs().sum()) == 0.0 and float(beta[b, :, n:].abs().sum()) == 0.0
        torch.testing.assert_close(alpha[b].sum(-1), torch.ones(H, dtype=torch.float64))


def test_bias_gradients_of_the_scores_are_zero():
    """softmax shift invariance: query_att.bias / key_att.bias never move the output"""
    m = _module(seed=4)
    x = torch.randn(2, 6, 64, dtype=torch.float64)
    (m(x, _mask((6, 3), 6)) * torch.randn(2, 6, 64, dtype=torch.float64)).sum().backward()
    assert float(m.query_att.bias.grad.abs().max()) < 1e-12 and float(m.key_att.bias.grad.abs().max()) < 1e-12
    assert float(m.query_att.weight.grad.abs().max()) > 1e-6


# ------------------------------------------------------------------------------------------------ the recipe
def test_recipe_builds_through_the_task_registry():
    from tavsr.layers import FastSelfAttention, PositionalEncoding
    from tavsr.tasks.asr import ASRTask
    conf = yaml.safe_load(open(FAST_YAML))
    base = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_transformer_ctc_english.yaml")))
    assert set(conf) == set(base)
    diff = {k for k in conf if conf[k] != base[k]}
    assert diff == {"encoder_conf"}
    assert {k: v for k, v in conf["encoder_conf"].items() if base["encoder_conf"][k] != v} == {
        "attention_layer_type": "fast_selfattn", "pos_enc_layer_type": "abs_pos"}
    conf["token_list"] = list(TOKENS_EN)
    model = ASRTask.build_model(argparse.Namespace(**conf))
    assert len(model.encoder.encoders) == 12 and all(isinstance(l.attn, FastSelfAttention) for l in model.encoder.encoders)
    assert type(model.encoder.embed.out[1]) is PositionalEncoding
    vsr = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "vsr_conv3dresnet18_branchformer_transformer_ctc_english.yaml")))
    vsr["encoder_conf"].update(attention_layer_type="fast_selfattn", pos_enc_layer_type="scaled_abs_pos")
    vsr["token_list"] = list(TOKENS_EN)
    vm = ASRTask.build_model(argparse.Namespace(**vsr))
    assert "encoder.embed.1.alpha" in vm.state_dict() or "encoder.embed.3.alpha" in vm.state_dict()
