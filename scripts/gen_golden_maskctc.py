"""Golden vectors for Mask-CTC (``model: maskctc``, ``decoder: mlm``) from the REFERENCE's own classes.

Imports the reference's Python over ``oracle._shim`` as ``oracle/gen_golden.py`` does, with four more stand-ins for espnet
names the checkout does not carry, registered into ``_shim._REAL`` before the shim is installed (``oracle/`` is not
edited): ``MLMDecoder`` and ``mask_uniform`` (this project's restatements in ``tests/maskctc_ref.py``), ``Hypothesis`` and
``TokenIDConverter`` (below).  The models are built by the reference's ``ASRTask`` / ``AVSRTask`` and run through the
reference's ``MaskCTCModel`` / ``AVSRMaskCTCModel`` / ``MaskCTCInference``.  Writes under ``tests/golden/``:

* ``maskctc_asr_3L.npz`` - 3-layer encoder, 2-layer MLM decoder, the batch of ``asr_model_3L``: the numpy seed, the masks
  drawn, train-mode loss / stats / picked gradients / all gradient norms, state_dict keys, parameter count, and the
  eval-mode decoder logits on the drawn ``ys_in``;
* ``maskctc_avsr_2L.npz`` - the same for the tailored audio-visual model at the size and batch of ``av_model_tailored_2L``;
* ``maskctc_decode.npz`` - ``MaskCTCInference.forward`` on seven utterances (T = 9 ... 499) with the ASR model's CTC head and
  decoder: per utterance T, the seed of its encoder output, threshold, K, CTC ids, ``y_hat``, token probabilities, ``y_in``
  initially and after every pass, the final ``yseq`` (the reference's own), and the decision margins.  The decode only ever
  sees the encoder OUTPUT, so that is a seeded tensor (``maskctc_ref.synth_encoder_output``: standard-normal frames held for
  runs of 1-7 frames, about T / 4 tokens) and the file stores its seed instead of 0.5 MB of floats for T = 499.  With seeded
  random weights the CTC maxima sit far below 0.99, so the threshold is put in the middle of the widest gap between neighbouring
  token probabilities around their median (about half the positions masked); three utterances take a special threshold: three
  masks (< K), none, all.  An utterance is accepted only if every logit margin is >= 1e-3 and its threshold distance >= 1e-4;
  otherwise the next seed is tried.

Re-running reproduces the files bit for bit (fixed seeds, one thread).

    python scripts/gen_golden_maskctc.py          # needs the reference checkout the shim points at
"""
import argparse
import copy
import math
import os
import sys
from typing import NamedTuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import maskctc_ref as R  # noqa: E402
from oracle import _shim  # noqa: E402
from oracle.gen_golden import AVSR_YAML, TOKENS, _np, _save, asr_conf, avsr_conf  # noqa: E402
from oracle.model import compact, fill_parameters_, synth  # noqa: E402

NP_SEED = 20240
DRAWN = []


class Hypothesis(NamedTuple):
    yseq: torch.Tensor
    score: float = 0.0
    scores: dict = {}
    states: dict = {}


class TokenIDConverter:
    def __init__(self, token_list, unk_symbol="<unk>"):
        self.token_list = list(token_list)

    def ids2tokens(self, ids):
        return [self.token_list[i] for i in ids]


def _mask_uniform(ys_pad, mask_token, eos, ignore_id):
    out = R.mask_uniform_ref(ys_pad, mask_token, eos, ignore_id)
    DRAWN.append(out)
    return out


def install():
    _shim._REAL["espnet2.asr.decoder.mlm_decoder"] = {"MLMDecoder": R.MLMDecoderRef}
    _shim._REAL["espnet.nets.pytorch_backend.maskctc.add_mask_token"] = {"mask_uniform": _mask_uniform}
    _shim._REAL["espnet.nets.beam_search"] = {"Hypothesis": Hypothesis}
    _shim._REAL["espnet2.text.token_id_converter"] = {"TokenIDConverter": TokenIDConverter}
    _shim.install()


def to_maskctc(conf):
    conf = copy.deepcopy(conf)
    conf["model"], conf["decoder"] = "maskctc", "mlm"
    for k in ("sym_sos", "sym_eos", "lang_token_id"):
        conf["model_conf"].pop(k)
    conf["token_list"] = TOKENS
    return conf


def _train_record(model, batch, text, tlens, pick):
    """one train-mode step of the reference's model -> arrays"""
    model.train()
    np.random.seed(NP_SEED)
    DRAWN.clear()
    loss, stats, _ = model(*[t.clone() for t in batch], text.clone(), tlens)
    loss.backward()
    (ys_in, ys_out), = DRAWN
    params = dict(model.named_parameters())
    grads = {"g_" + n: compact(params[n].grad) for n in pick if n in params}
    gnorm = {n: float(p.grad.norm()) for n, p in params.items() if p.grad is not None}
    model.eval()
    with torch.no_grad():
        enc, olens = model.encode(*[t.clone() for t in batch])
        logits, _ = model.decoder(enc, olens, ys_in, tlens)
    return dict(np_seed=NP_SEED, ys_in=_np(ys_in), ys_out=_np(ys_out), loss_train=_np(loss), loss_ctc=_np(stats["loss_ctc"]),
                loss_mlm=_np(stats["loss_mlm"]), acc_mlm=_np(stats["acc_mlm"]), stats_keys=np.array(list(stats.keys())),
                dec_logits=_np(logits), olens=_np(olens), mask_token=model.mask_token, vocab_size=model.vocab_size, eos=model.eos,
                gnorm_keys=np.array(list(gnorm.keys())), gnorm_vals=np.array(list(gnorm.values()), dtype=np.float64),
                n_params=sum(p.numel() for p in model.parameters()), keys=np.array(sorted(model.state_dict().keys())), **grads)


def build_asr():
    from src.tasks.asr import ASRTask
    model = ASRTask.build_model(argparse.Namespace(**to_maskctc(asr_conf(num_blocks=3, dec_blocks=2))))
    assert type(model).__name__ == "MaskCTCModel" and type(model.decoder) is R.MLMDecoderRef
    fill_parameters_(model, seed=41)
    return model


def gen_asr(model):
    B, Tin, Lmax = 3, 120, 12                     # the batch of gen_golden.gen_asr_model
    speech, slens, tlens = synth((B, Tin, 80), seed=42), torch.tensor([120, 96, 64]), torch.tensor([12, 7, 10])
    text = synth((B, Lmax), seed=43, kind="int", lo=1, hi=39)
    for i, l in enumerate(tlens):
        text[i, l:] = -1
    pick = ["encoder.embed.conv.0.weight", "encoder.encoders.0.attn.pos_bias_v", "encoder.encoders.2.feed_forward.w_2.weight",
            "encoder.after_norm.weight", "ctc.ctc_lo.weight", "decoder.embed.0.weight", "decoder.decoders.0.src_attn.linear_k.weight",
            "decoder.decoders.0.self_attn.linear_k.weight", "decoder.decoders.1.self_attn.linear_q.bias", "decoder.output_layer.bias",
            "decoder.output_layer.weight", "decoder.after_norm.bias"]
    _save("maskctc_asr_3L", B=B, Tin=Tin, slens=_np(slens), tlens=_np(tlens), text=_np(text),
          **_train_record(model, (speech, slens), text, tlens, pick))


def gen_avsr():
    from src.tasks.avsr import AVSRTask
    seed = 101                                    # the model and batch of gen_golden._gen_avsr_model("av_model_tailored_2L")
    model = AVSRTask.build_model(argparse.Namespace(**to_maskctc(avsr_conf(AVSR_YAML, num_blocks=2, dec_blocks=1))))
    assert type(model).__name__ == "AVSRMaskCTCModel"
    fill_parameters_(model, seed=seed)
    B, Ta, Tv, Lmax = 2, 40, 9, 6
    audio, video = synth((B, Ta, 80), seed=seed + 1), synth((B, Tv, 88, 88), seed=seed + 2)
    alens, vlens, tlens = torch.tensor([40, 32]), torch.tensor([9, 8]), torch.tensor([6, 4])
    text = synth((B, Lmax), seed=seed + 3, kind="int", lo=1, hi=39)
    for i, l in enumerate(tlens):
        text[i, l:] = -1
    pick = ["visual_frontend.frontend3D.0.weight", "acoustic_embed.embed.conv.0.weight", "visual_embed.embed.0.weight",
            "encoder.modality_encoding.weight", "audiovisual_fusion.audiovisual_layer.w_1.weight", "ctc.ctc_lo.weight",
            "decoder.embed.0.weight", "decoder.decoders.0.self_attn.linear_k.weight", "decoder.output_layer.weight"]
    _save("maskctc_avsr_2L", B=B, Ta=Ta, Tv=Tv, alens=_np(alens), vlens=_np(vlens), tlens=_np(tlens), text=_np(text),
          **_train_record(model, (audio, alens, video, vlens), text, tlens, pick))


def median_gap_threshold(prob):
    """the middle of the widest gap between neighbouring token probabilities among the middle fifth of their ranks"""
    s = np.sort(prob.astype(np.float64))
    lo, hi = int(0.4 * len(s)), max(int(0.6 * len(s)), int(0.4 * len(s)) + 2)
    band = s[lo: min(hi, len(s))]
    i = int(np.argmax(np.diff(band)))
    return float((band[i] + band[i + 1]) / 2)


UTTERANCES = (          # (T, K, kind of threshold)
    (499, 10, "median"), (150, 10, "median"), (97, 10, "median"), (61, 10, "three"), (38, 10, "none"), (23, 10, "all"),
    (9, 4, "median"))


def gen_decode(model):
    from src.models.maskctc_model import MaskCTCInference
    model.eval()
    out = dict(n_utt=len(UTTERANCES))
    for u, (T, K, kind) in enumerate(UTTERANCES):
        for seed in range(700 + 100 * u, 800 + 100 * u):
            enc = R.synth_encoder_output(T, seed)
            with torch.no_grad():
                _, _, prob = R.ctc_tokens(model.ctc.ctc_lo(enc))
            s = np.sort(_np(prob).astype(np.float64))
            thr = {"median": lambda: median_gap_threshold(_np(prob)), "three": lambda: float((s[2] + s[3]) / 2),
                   "none": lambda: float(s[0] / 2), "all": lambda: 0.99}[kind]()
            tr = R.maskctc_infer(model.ctc.ctc_lo, model.decoder, enc, model.mask_token, K, thr)
            if min(tr["m_ctc"], tr["m_fill"], tr["m_cand"]) >= 1e-3 and tr["m_thr"] >= 1e-4:
                break
            print(f"  utterance {u}: seed {seed} falls short (ctc {tr['m_ctc']:.1e} fill {tr['m_fill']:.1e} cand {tr['m_cand']:.1e} "
                  f"thr {tr['m_thr']:.1e}): next seed")
        else:
            raise RuntimeError(f"no seed gives utterance {u} clear margins")
        with torch.no_grad():
            hyp = MaskCTCInference(model, n_iterations=K, threshold_probability=thr)(enc)        # the reference's own loop
        assert torch.equal(hyp.yseq, tr["yseq"]), (u, hyp.yseq, tr["yseq"])
        mask_num, num_iter, per_iter = tr["plan"]
        assert {"three": mask_num == 3, "none": mask_num == 0, "all": mask_num == len(tr["y_hat"])}.get(kind, True), (kind, mask_num)
        print(f"utterance {u}: T {T} seed {seed} tokens {len(tr['y_hat'])} masked {mask_num} passes {num_iter} x {per_iter}; margins "
              f"ctc {tr['m_ctc']:.2e} thr {tr['m_thr']:.2e} fill {tr['m_fill']:.2e} cand {tr['m_cand']:.2e}")
        inf = lambda v: np.float64(v if math.isfinite(v) else np.inf)
        out.update({f"u{u}_T": T, f"u{u}_seed": seed, f"u{u}_K": K, f"u{u}_thr": np.float64(thr), f"u{u}_ctc_ids": _np(tr["ctc_ids"]),
                    f"u{u}_y_hat": _np(tr["y_hat"]), f"u{u}_tok_prob": _np(tr["tok_prob"]), f"u{u}_plan": np.array(tr["plan"]),
                    f"u{u}_y_in": np.stack([_np(y) for y in tr["y_in"]]), f"u{u}_yseq": _np(hyp.yseq),
                    f"u{u}_margins": np.array([inf(tr[k]) for k in ("m_ctc", "m_thr", "m_fill", "m_cand")])})
    _save("maskctc_decode", **out)


def main():
    install()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    model = build_asr()
    gen_asr(model)
    for p in model.parameters():
        p.grad = None
    gen_decode(model)
    gen_avsr()


if __name__ == "__main__":
    main()
