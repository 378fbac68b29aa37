"""CPU: the Mask-CTC model family on the host (no GPU, no compute calls): registries and recipes, constructor surface,
``mask_uniform``'s draw, the C ABI's two entry points, and ``tests/maskctc_ref.py`` - the restatement the GPU tests compare
against - pinned to the fixtures ``scripts/gen_golden_maskctc.py`` wrote from the reference's own classes."""
import argparse
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import maskctc_ref as R
from helpers import ROOT, TOKENS_EN, avsr_conf, golden
from oracle.model import fill_parameters_, synth

REL = 1e-4      # the project's bar for losses (tests/test_gpu_parity.py)


def _asr_batch(g):
    speech = synth((int(g["B"]), int(g["Tin"]), 80), seed=42)
    return (speech, torch.from_numpy(g["slens"])), torch.from_numpy(g["text"]), torch.from_numpy(g["tlens"])


def _avsr_batch(g, seed=101):
    B, Ta, Tv = int(g["B"]), int(g["Ta"]), int(g["Tv"])
    audio, video = synth((B, Ta, 80), seed=seed + 1), synth((B, Tv, 88, 88), seed=seed + 2)
    return ((audio, torch.from_numpy(g["alens"]), video, torch.from_numpy(g["vlens"])), torch.from_numpy(g["text"]),
            torch.from_numpy(g["tlens"]))


def _avsr_small():
    conf = avsr_conf(R.AVSR_MASKCTC_YAML, num_blocks=2, dec_blocks=1)
    conf["token_list"] = list(TOKENS_EN)
    return conf


def test_tasks_build_the_maskctc_models_from_the_new_recipes():
    from tavsr.decoder.mlm_decoder import MLMDecoder
    from tavsr.models.avsr_maskctc_model import AVSRMaskCTCModel
    from tavsr.models.maskctc_model import MaskCTCModel
    from tavsr.tasks.asr import ASRTask
    from tavsr.tasks.avsr import AVSRTask
    for task, cls, conf, name in ((ASRTask, MaskCTCModel, R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), "maskctc_asr_3L"),
                                  (AVSRTask, AVSRMaskCTCModel, _avsr_small(), "maskctc_avsr_2L")):
        g = golden(name)
        m = task.build_model(argparse.Namespace(**copy.deepcopy(conf)))
        assert type(m) is cls and type(m.decoder) is MLMDecoder
        assert sorted(m.state_dict().keys()) == list(g["keys"])
        assert sum(p.numel() for p in m.parameters()) == int(g["n_params"])
        assert (m.mask_token, m.vocab_size, m.eos) == (int(g["mask_token"]), int(g["vocab_size"]), int(g["eos"])) == (41, 42, 40)
        assert m.token_list[-1] == "<mask>" and len(m.token_list) == 42
        assert m.ctc.ctc_lo.weight.shape[0] == 41 and m.decoder.output_layer.weight.shape[0] == 42
        assert m.decoder.embed[0].weight.shape[0] == 42
        assert hasattr(m, "criterion_mlm") and not hasattr(m, "criterion_att")
        for key in ("sym_sos", "sym_eos", "lang_token_id"):          # the three keys a Mask-CTC recipe drops, refused by name
            bad = copy.deepcopy(conf)
            bad["model_conf"][key] = -1 if key == "lang_token_id" else "<sos/eos>"
            with pytest.raises(TypeError, match=key):
                task.build_model(argparse.Namespace(**bad))
    with pytest.raises(NotImplementedError):
        m.nll(None, None, None, None)


def test_unknown_names_are_treated_as_before():
    """unchanged behaviour by design (this one passes without the feature too): an unknown decoder name still raises, an unknown
    model name still builds the attention model"""
    from tavsr.models.espnet_model import ESPnetASRModel
    from tavsr.tasks.asr import ASRTask
    from helpers import asr_conf
    conf = asr_conf(num_blocks=1, dec_blocks=1)
    conf["decoder"] = "rnn"
    with pytest.raises(ValueError, match="decoder"):
        ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    conf["decoder"], conf["model"] = "transformer", "no_such_model"
    assert type(ASRTask.build_model(argparse.Namespace(**conf))) is ESPnetASRModel


def test_mlm_decoder_refuses_what_the_transformer_decoder_refuses():
    from tavsr.decoder.mlm_decoder import MLMDecoder
    for kw in (dict(input_layer="linear"), dict(normalize_before=False), dict(concat_after=True), dict(use_output_layer=False)):
        with pytest.raises(ValueError):
            MLMDecoder(41, 256, num_blocks=1, **kw)
    with pytest.raises(TypeError):
        MLMDecoder(41, 256, layer_drop_rate=0.1)


@pytest.mark.parametrize("name", ["maskctc_asr_3L", "maskctc_avsr_2L"])
def test_mask_uniform_draws_the_recorded_masks(name):
    from tavsr.models.maskctc_model import mask_uniform
    g = golden(name)
    text = torch.from_numpy(g["text"])
    np.random.seed(int(g["np_seed"]))
    ys_in, ys_out = mask_uniform(text, int(g["mask_token"]), int(g["eos"]), -1)
    assert ys_in.dtype == torch.int64 and torch.equal(ys_in, torch.from_numpy(g["ys_in"]))
    assert torch.equal(ys_out, torch.from_numpy(g["ys_out"]))
    np.random.seed(int(g["np_seed"]))
    a, b = R.mask_uniform_ref(text, int(g["mask_token"]), int(g["eos"]), -1)
    assert torch.equal(a, ys_in) and torch.equal(b, ys_out)


def _check_train(m, g, batch, text, tlens):
    m.train()
    np.random.seed(int(g["np_seed"]))
    loss, stats, ys_in, ys_out = R.maskctc_forward(m, batch, text, tlens)
    assert torch.equal(ys_in, torch.from_numpy(g["ys_in"])) and torch.equal(ys_out, torch.from_numpy(g["ys_out"]))
    assert [k for k in g["stats_keys"]] == list(stats.keys())
    for got, key in ((loss, "loss_train"), (stats["loss_ctc"], "loss_ctc"), (stats["loss_mlm"], "loss_mlm"),
                     (stats["acc_mlm"], "acc_mlm")):
        want, got = float(g[key].reshape(-1)[0]), float(torch.as_tensor(got).detach())
        assert abs(got - want) <= REL * abs(want), (key, got, want)
    loss.backward()
    want = dict(zip(g["gnorm_keys"], g["gnorm_vals"]))
    for n, p in m.named_parameters():
        if p.grad is not None:
            # (analytically zero gradients - linear_k.bias: softmax shift invariance - are rounding noise on both sides, helpers.grad_ok)
            assert abs(float(p.grad.norm()) - want[n]) <= (1e-3 * want[n] if want[n] >= 1e-6 else 1e-5), n
    m.eval()
    with torch.no_grad():
        enc, olens = m.encode(*batch)
        logits, _ = m.decoder(enc, olens, ys_in, tlens)
    ref = torch.from_numpy(g["dec_logits"])
    for b, n in enumerate(tlens.tolist()):
        assert float((logits[b, :n] - ref[b, :n]).abs().max()) <= REL * float(ref[b, :n].abs().max())


def test_restatement_matches_the_reference_training_step_asr():
    g = golden("maskctc_asr_3L")
    m = R.build_asr_ref(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), TOKENS_EN)
    assert sorted(m.state_dict().keys()) == list(g["keys"])
    fill_parameters_(m, seed=41)
    _check_train(m, g, *_asr_batch(g))


def test_restatement_matches_the_reference_training_step_avsr():
    g = golden("maskctc_avsr_2L")
    m = R.build_avsr_ref(_avsr_small(), TOKENS_EN)
    assert sorted(m.state_dict().keys()) == list(g["keys"])
    fill_parameters_(m, seed=101)
    _check_train(m, g, *_avsr_batch(g))


def test_restatement_matches_the_reference_decoding_trace():
    g = golden("maskctc_decode")
    m = R.build_asr_ref(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), TOKENS_EN).eval()
    fill_parameters_(m, seed=41)
    assert int(g["n_utt"]) >= 6
    kinds = set()
    for u in range(int(g["n_utt"])):
        T, K, thr = int(g[f"u{u}_T"]), int(g[f"u{u}_K"]), float(g[f"u{u}_thr"])
        enc = R.synth_encoder_output(T, int(g[f"u{u}_seed"]))
        tr = R.maskctc_infer(m.ctc.ctc_lo, m.decoder, enc, m.mask_token, K, thr)
        assert torch.equal(tr["ctc_ids"], torch.from_numpy(g[f"u{u}_ctc_ids"]))
        assert torch.equal(tr["y_hat"], torch.from_numpy(g[f"u{u}_y_hat"]))
        assert np.allclose(tr["tok_prob"].numpy(), g[f"u{u}_tok_prob"], rtol=1e-6, atol=0)
        assert list(tr["plan"]) == g[f"u{u}_plan"].tolist()
        assert torch.equal(torch.stack(tr["y_in"]), torch.from_numpy(g[f"u{u}_y_in"]))
        assert torch.equal(tr["yseq"], torch.from_numpy(g[f"u{u}_yseq"]))
        mg = g[f"u{u}_margins"]
        assert min(mg[0], mg[2], mg[3]) >= 1e-3 and mg[1] >= 1e-4, (u, mg)       # the generator's acceptance rule
        assert R.margins_ok(tr)
        n, mask_num = len(tr["y_hat"]), tr["plan"][0]
        kinds |= {"few" if 0 < mask_num < K else "", "none" if mask_num == 0 else "", "all" if mask_num == n else "",
                  "T499" if T == 499 else ""}
    assert {"few", "none", "all", "T499"} <= kinds


def test_restatement_in_fp64_agrees_with_fp32():
    g = golden("maskctc_decode")
    m = R.build_asr_ref(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2), TOKENS_EN).eval()
    fill_parameters_(m, seed=41)
    m = m.double()
    for u in (2, 3, 6):
        enc = R.synth_encoder_output(int(g[f"u{u}_T"]), int(g[f"u{u}_seed"])).double()
        tr = R.maskctc_infer(m.ctc.ctc_lo, m.decoder, enc, m.mask_token, int(g[f"u{u}_K"]), float(g[f"u{u}_thr"]))
        assert tr["tok_prob"].dtype == torch.float64 and torch.equal(tr["yseq"], torch.from_numpy(g[f"u{u}_yseq"]))


def test_fill_pass_tie_rule_and_mask_token_winning():
    """a pin of the RESTATEMENT's tie rule and plan arithmetic (test code only, no product code: the kernel is held to the same cases
    on the GPU, test_gpu_maskctc.py::test_maskctc_step_kernel_tie_rule_and_mask_token_winning)"""
    V1, mask = 6, 5
    y = torch.tensor([mask, 2, mask, mask, mask])
    lg = torch.zeros(5, V1)
    lg[0, 1] = lg[2, 3] = lg[3, 4] = 2.0       # three equal maxima: the two lower positions are taken
    lg[4, mask] = 9.0                          # <mask> wins the argmax: chosen first, stays masked
    out, _, _ = R.fill_pass(lg, y, mask, it=0, num_iter=3, per_iter=3)
    assert out.tolist() == [1, 2, 3, mask, mask]
    out, _, _ = R.fill_pass(lg, y, mask, it=2, num_iter=3, per_iter=3)
    assert out.tolist() == [1, 2, 3, 4, mask]
    out, _, _ = R.fill_pass(lg, y, mask, it=3, num_iter=3, per_iter=3)
    assert out.tolist() == y.tolist()
    assert R.plan_of(7, 10) == (7, 7, 1) and R.plan_of(25, 10) == (25, 10, 2) and R.plan_of(5, 0) == (5, 5, 1)
    assert R.plan_of(0, 10) == (0, 0, 0)


def test_product_state_dict_loads_the_restatement_and_ids2text():
    from tavsr.models.maskctc_model import MaskCTCInference
    from tavsr.tasks.asr import ASRTask
    conf = R.asr_maskctc_conf(num_blocks=1, dec_blocks=1)
    ref = R.build_asr_ref(conf, TOKENS_EN)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    model.load_state_dict(ref.state_dict())
    inf = MaskCTCInference(model, n_iterations=10, threshold_probability=0.99)
    assert inf.ids2text([21, 41, 13, 22]) == "H_ I"
    assert inf.mask_token == 41 and inf.mlm is model.decoder and inf.ctc is model.ctc


def test_speech2text_front_ends_and_the_model_switch():
    import tavsr.inference as inference
    from tavsr.tasks.asr import ASRTask
    from tavsr.utils.inference import build_speech2text
    assert inference.__all__ == ["Speech2Text", "Speech2TextMaskCTC"]
    conf = R.asr_maskctc_conf(num_blocks=1, dec_blocks=1)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    s2t = build_speech2text(argparse.Namespace(**conf), model)
    assert type(s2t) is inference.Speech2TextMaskCTC
    assert (s2t.s2t.n_iterations, s2t.s2t.threshold_probability) == (10, 0.99)
    with pytest.raises(ValueError, match="unknown model architecture"):
        build_speech2text(dict(conf, model="transducer"), model)


def test_c_abi_declares_exports_and_validates_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    names = set(re.findall(r"\b(tavsr_[a-z0-9_]+)\s*\(", hdr))
    assert {"tavsr_maskctc_init", "tavsr_maskctc_step"} <= names
    lib = ctypes.CDLL(os.path.join(ROOT, "tailored-avsr_amd", "tavsr", "lib", "libtavsr_hip.so"))
    lib.tavsr_last_error_string.restype = ctypes.c_char_p
    buf = (ctypes.c_int64 * 16)()                 # a host address: the checks return before anything is launched or read
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    i64, i32, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double

    def init(logits=p, y_in=p, plan=p, V=41, T=4, ld_y=4):
        return lib.tavsr_maskctc_init(logits, i64(V), i64(T * V), null, i32(0), i32(41), f64(0.5), i32(10), y_in, p, p, i64(ld_y), p,
                                      plan, i32(1), i32(T), i32(V), null)

    def step(logits=p, y_in=p, plan=p, it=0, V1=42, L=4, mask=41):
        return lib.tavsr_maskctc_step(logits, i64(V1), i64(L * V1), y_in, i64(L), p, plan, i32(it), i32(mask), i32(1), i32(L), i32(V1),
                                      null)

    cases = ((init, dict(logits=null), "null pointer"), (init, dict(y_in=null), "null pointer"), (init, dict(plan=null), "null pointer"),
             (init, dict(V=0), "V >= 1"), (init, dict(ld_y=3), "ld_y"), (step, dict(logits=null), "null pointer"),
             (step, dict(y_in=null), "null pointer"), (step, dict(plan=null), "null pointer"), (step, dict(V1=1, mask=0), "V + 1 >= 2"),
             (step, dict(it=-1), "it < 0"), (step, dict(mask=42), "mask_token"))
    for fn, kw, what in cases:
        rc = fn(**kw)
        assert rc != 0 and what in lib.tavsr_last_error_string().decode(), (kw, rc, lib.tavsr_last_error_string())
