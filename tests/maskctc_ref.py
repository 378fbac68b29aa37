"""CPU restatement of Mask-CTC in plain torch (fp32 or fp64, whatever the model it is handed is): the MLM decoder, the
training loss of ``MaskCTCModel`` / ``AVSRMaskCTCModel`` and the decoding loop of ``MaskCTCInference`` with a trace of
every decision and its margin.  Built on ``oracle.leaves`` / ``oracle.model`` / ``oracle.av`` by import; the GPU tests
compare against it because no reference checkout exists where they run, and ``tests/golden/maskctc_*.npz`` (written by
``scripts/gen_golden_maskctc.py`` from the reference's own classes) pin it (tests/test_maskctc_host.py)."""
import copy
import math
import os

import numpy as np
import torch

from oracle import leaves as L


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASR_MASKCTC_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_maskctc_english.yaml")
AVSR_MASKCTC_YAML = os.path.join(ROOT, "tailored-avsr_amd", "configs", "avsr_tailored_maskctc_english.yaml")


def asr_maskctc_conf(num_blocks=12, dropout=0.0, dec_blocks=6, **enc_over):
    """the edits of ``helpers.asr_conf`` on the Mask-CTC recipe (``helpers.avsr_conf`` takes the AVSR one by path)"""
    import yaml
    conf = yaml.safe_load(open(ASR_MASKCTC_YAML))
    conf.update(input_size=80, specaug=None)
    conf["encoder_conf"]["num_blocks"], conf["decoder_conf"]["num_blocks"] = num_blocks, dec_blocks
    for part, keys in (("encoder_conf", ("dropout_rate", "positional_dropout_rate", "attention_dropout_rate")),
                       ("decoder_conf", ("dropout_rate", "positional_dropout_rate", "self_attention_dropout_rate",
                                         "src_attention_dropout_rate")), ("ctc_conf", ("dropout_rate",))):
        for k in keys:
            conf[part][k] = dropout
    conf["encoder_conf"].update(enc_over)
    return conf


class MLMDecoderRef(L.TransformerDecoder):
    """espnet2 ``MLMDecoder``: the TransformerDecoder stack with one more vocabulary row (<mask>), no layer drop, and a
    self-attention mask that is the padding mask on both axes - not causal."""

    def __init__(self, vocab_size, encoder_output_size, attention_heads=4, linear_units=2048, num_blocks=6, dropout_rate=0.1,
                 positional_dropout_rate=0.1, self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0,
                 input_layer="embed", use_output_layer=True, pos_enc_class=L.PositionalEncoding, normalize_before=True,
                 concat_after=False):
        super().__init__(vocab_size + 1, encoder_output_size, attention_heads, linear_units, num_blocks, dropout_rate,
                         positional_dropout_rate, self_attention_dropout_rate, src_attention_dropout_rate, input_layer,
                         use_output_layer, pos_enc_class, normalize_before, concat_after)

    def forward(self, hs_pad, hlens, ys_in_pad, ys_in_lens):
        valid = (~L.make_pad_mask(ys_in_lens, maxlen=ys_in_pad.size(1))).to(ys_in_pad.device)        # (B, L)
        tgt_mask = valid[:, None, :] & valid[:, :, None]
        memory_mask = (~L.make_pad_mask(hlens, maxlen=hs_pad.size(1)))[:, None, :].to(hs_pad.device)
        x = self.embed(ys_in_pad)
        x, tgt_mask, _, _ = self.decoders(x, tgt_mask, hs_pad, memory_mask)
        x = self.output_layer(self.after_norm(x))
        return x, tgt_mask.sum(1)


def mask_uniform_ref(ys_pad, mask_token, eos, ignore_id):
    """espnet ``mask_uniform``: numpy's global generator, one randint and one choice (with replacement) per utterance"""
    ys = [y[y != ignore_id] for y in ys_pad]
    ys_out = [torch.full_like(y, ignore_id) for y in ys]
    ys_in = [y.clone() for y in ys]
    for i, y in enumerate(ys):
        n = np.random.randint(1, len(y) + 1)
        idx = np.random.choice(len(y), n)
        ys_in[i][idx] = mask_token
        ys_out[i][idx] = y[idx]
    return L.pad_list(ys_in, eos), L.pad_list(ys_out, ignore_id)


def to_maskctc_(oracle, decoder_conf, encoder_output_size=256, lsm_weight=0.0, length_normalized_loss=False):
    """turn an ``ASRModelOracle`` / ``AVSRModelOracle`` (built WITHOUT a decoder) into the Mask-CTC model in place:
    MLM decoder, <mask> appended, criterion_mlm for criterion_att (maskctc_model.py:95-109)"""
    oracle.decoder = MLMDecoderRef(vocab_size=oracle.vocab_size, encoder_output_size=encoder_output_size, **decoder_conf)
    oracle.token_list = list(oracle.token_list) + ["<mask>"]
    oracle.vocab_size += 1
    oracle.mask_token = oracle.vocab_size - 1
    del oracle.criterion_att
    oracle.criterion_mlm = L.LabelSmoothingLoss(oracle.vocab_size, oracle.ignore_id, lsm_weight, length_normalized_loss)
    return oracle


def build_asr_ref(conf, token_list):
    from oracle.model import build_asr_oracle
    c = copy.deepcopy(conf)
    c["decoder"] = None
    m = build_asr_oracle(c, token_list)
    mc = conf["model_conf"]
    return to_maskctc_(m, conf["decoder_conf"], m.encoder.output_size(), mc.get("lsm_weight", 0.0),
                       mc.get("length_normalized_loss", False))


def build_avsr_ref(conf, token_list):
    from oracle.av import build_avsr_oracle
    c = copy.deepcopy(conf)
    c["decoder"] = None
    m = build_avsr_oracle(c, token_list)
    mc = conf["model_conf"]
    return to_maskctc_(m, conf["decoder_conf"], m.audiovisual_fusion.output_size(), mc.get("lsm_weight", 0.0),
                       mc.get("length_normalized_loss", False))


def maskctc_forward(m, inputs, text, text_lengths, ys_in_pad=None, ys_out_pad=None):
    """MaskCTCModel.forward / AVSRMaskCTCModel.forward on a model of ``build_*_ref``: ``inputs`` are the tensors of its
    ``encode``.  -> (loss, stats, ys_in_pad, ys_out_pad)"""
    text = text.clone()
    text[text == -1] = m.ignore_id
    text = text[:, : text_lengths.max()]
    enc, enc_lens = m.encode(*inputs)
    inter = None
    if isinstance(enc, tuple):
        enc, inter = enc
    stats = {}
    loss_ctc = loss_mlm = acc_mlm = None
    if m.ctc_weight != 0.0:
        loss_ctc = m.ctc(enc, enc_lens, text, text_lengths)
        cer_ctc = None
        if not m.training and m.error_calculator is not None:
            cer_ctc = m.error_calculator(m.ctc.argmax(enc).data.cpu(), text.cpu(), is_ctc=True)
        stats["loss_ctc"], stats["cer_ctc"] = loss_ctc.detach(), cer_ctc
    if m.interctc_weight != 0.0 and inter is not None:
        li = 0.0
        for idx, o in inter:
            l_ = m.ctc(o, enc_lens, text, text_lengths)
            stats[f"loss_interctc_layer{idx}"] = l_.detach()
            li = li + l_
        loss_ctc = (1 - m.interctc_weight) * loss_ctc + m.interctc_weight * li / len(inter)
    if m.ctc_weight != 1.0:
        if ys_in_pad is None:
            ys_in_pad, ys_out_pad = mask_uniform_ref(text, m.mask_token, m.eos, m.ignore_id)
        dec_out, _ = m.decoder(enc, enc_lens, ys_in_pad, text_lengths)
        loss_mlm = m.criterion_mlm(dec_out, ys_out_pad)
        acc_mlm = L.th_accuracy(dec_out.view(-1, m.vocab_size), ys_out_pad, ignore_label=m.ignore_id)
    if m.ctc_weight == 0.0:
        loss = loss_mlm
    elif m.ctc_weight == 1.0:
        loss = loss_ctc
    else:
        loss = m.ctc_weight * loss_ctc + (1 - m.ctc_weight) * loss_mlm
    stats.update(loss_mlm=None if loss_mlm is None else loss_mlm.detach(), acc_mlm=acc_mlm, loss=loss.detach())
    return loss, stats, ys_in_pad, ys_out_pad


# ------------------------------------------------------------------------------------------------ decoding
def synth_encoder_output(T, seed, D=256):
    """a seeded stand-in for an encoder output [T, D] (what the decoding fixtures store a seed for): standard-normal frames
    (the scale of a LayerNorm output) held for runs of 1-7 frames, so that the greedy CTC path repeats labels as a real one
    does and an utterance of T frames yields about T / 4 tokens"""
    from oracle.model import synth
    runs = synth((T,), seed=seed + 100000, kind="int", lo=1, hi=8)
    idx = torch.repeat_interleave(torch.arange(T), runs)[:T]
    return synth((T, D), seed=seed)[idx].contiguous()


def _top2_gap(rows):
    """smallest (largest - second largest) over the rows of a 2-D tensor; inf for no rows"""
    if rows.numel() == 0 or rows.shape[-1] < 2:
        return math.inf
    t = rows.topk(2, dim=-1).values
    return float((t[:, 0] - t[:, 1]).min())


def ctc_tokens(logits, blank=0):
    """CTC logits [T, V] of one utterance -> (frame ids [T], y_hat [n], tok_prob [n]): greedy ids, runs of equal ids with the
    maximum posterior over the run, blank runs dropped (maskctc_model.py:289-308).  The posterior of the argmax is
    ``1 / sum exp(x - max)`` in the logits' own precision."""
    ids = logits.argmax(-1)
    p = 1.0 / (logits - logits.max(-1, keepdim=True).values).exp().sum(-1)
    y_hat, prob = [], []
    t, T = 0, logits.shape[0]
    while t < T:
        e = t
        while e < T and int(ids[e]) == int(ids[t]):
            e += 1
        if int(ids[t]) != blank:
            m = p.new_tensor(-1.0)                  # :301-304: starts at -1 and is replaced where strictly smaller (a NaN never is)
            for q in p[t:e]:
                if m < q:
                    m = q
            y_hat.append(int(ids[t]))
            prob.append(m)
        t = e
    prob = torch.stack(prob) if prob else p.new_zeros(0)
    return ids, torch.tensor(y_hat, dtype=torch.int64), prob


def plan_of(mask_num, K):
    num_iter = K if (mask_num >= K and K > 0) else mask_num
    return mask_num, num_iter, (mask_num // num_iter if num_iter else 0)


def fill_pass(logits, y_in, mask_token, it, num_iter, per_iter):
    """one pass of the loop on decoder logits [L, V+1] and y_in [L] (a new tensor is returned) -> (y_in, top-2 gap at the
    filled positions, gap between the last chosen and the first rejected candidate).  Equal maxima: the lower position first."""
    y_in = y_in.clone()
    if it >= num_iter:
        return y_in, math.inf, math.inf
    mask_idx = torch.nonzero(y_in == mask_token).squeeze(-1)
    if mask_idx.numel() == 0:
        return y_in, math.inf, math.inf
    score, pred = logits[mask_idx].max(dim=-1)
    if it == num_iter - 1:
        chosen, cand_gap = torch.arange(mask_idx.numel()), math.inf
    else:
        order = torch.sort(score, descending=True, stable=True).indices
        k = min(per_iter, mask_idx.numel())
        chosen = order[:k]
        cand_gap = float(score[order[k - 1]] - score[order[k]]) if 0 < k < mask_idx.numel() else math.inf
    y_in[mask_idx[chosen]] = pred[chosen]
    return y_in, _top2_gap(logits[mask_idx[chosen]]), cand_gap


@torch.no_grad()
def maskctc_infer(ctc_lo, mlm, enc, mask_token, K, threshold):
    """MaskCTCInference.forward (maskctc_model.py:285-349) on one utterance ``enc`` [T, D] with ``ctc_lo`` the CTC head's
    Linear and ``mlm`` the MLM decoder -> dict: ctc_ids, y_hat, tok_prob, plan, y_in (list: initial, then after every pass),
    yseq, and the decision margins m_ctc / m_thr / m_fill / m_cand (inf where no such decision was taken)."""
    logits = ctc_lo(enc)
    ids, y_hat, prob = ctc_tokens(logits)
    masked = prob.double() < float(threshold)
    y_in = torch.where(masked, torch.full_like(y_hat, mask_token), y_hat)
    mask_num, num_iter, per_iter = plan_of(int(masked.sum()), K)
    out = dict(ctc_ids=ids, y_hat=y_hat, tok_prob=prob, plan=(mask_num, num_iter, per_iter), y_in=[y_in.clone()],
               m_ctc=_top2_gap(logits), m_thr=float((prob.double() - float(threshold)).abs().min()) if prob.numel() else math.inf,
               m_fill=math.inf, m_cand=math.inf)
    T, n = enc.shape[0], y_in.numel()
    for it in range(num_iter):
        dec, _ = mlm(enc[None], [T], y_in[None], [n])
        y_in, g_fill, g_cand = fill_pass(dec[0], y_in, mask_token, it, num_iter, per_iter)
        out["y_in"].append(y_in.clone())
        out["m_fill"], out["m_cand"] = min(out["m_fill"], g_fill), min(out["m_cand"], g_cand)
    out["yseq"] = torch.tensor([mask_token] + y_in.tolist() + [mask_token], dtype=torch.int64)
    return out


def margins_ok(tr, logit_bar=1e-4, thr_bar=1e-5):
    """may the utterance be compared id by id?  every logit margin above ``logit_bar``, the threshold distance above ``thr_bar``"""
    return min(tr["m_ctc"], tr["m_fill"], tr["m_cand"]) > logit_bar and tr["m_thr"] > thr_bar
