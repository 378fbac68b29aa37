"""Batched hybrid CTC/attention beam search with LM scoring on the MI355X (BASELINE config 5).

Same search as the reference's decode path - espnet ``BatchBeamSearch`` with scorers {decoder, CTCPrefixScorer,
LengthBonus, lm}, weights {decoder: 1 - ctc_weight, ctc: ctc_weight, lm: lm_weight, length_bonus: penalty}, pre-beam of
``int(1.5 * beam)`` candidates on the weighted full scores, end detection of ``maxlenratio == 0``
(src/inference/avsr_inference.py:141-153, 249-255, 277-304, 449-518) - but the hypotheses of ALL utterances of a batch
advance together (the reference decodes one utterance at a time on the CPU):

* N = U x beam slots.  One step = one token for every slot: decoder step (6 layers) and LM step (16 layers) as
  [N, d] GEMMs on the MFMA kernel, self-attention over each hypothesis' own history by ``tavsr_tree_attn_step`` (keys
  and values stay where they were written; a hypothesis is an int32 list of ancestor rows), source attention against
  the per-utterance memory keys/values projected once, CTC prefix scores of the pre-beam candidates by
  ``tavsr_ctc_prefix_step``.
* The per-step bookkeeping is index plumbing on [N]-sized tensors: top-k and ancestor-list gathers in the beam-update launches,
  ended-hypothesis lists and end detection on the host (inference/search_host.py).

* An n-gram LM (``ngram=``, tavsr/lm/ngram.py: an ARPA file as tables in device memory) is the fifth scorer: one launch per token
  (``tavsr_ngram_score``) adds its weighted log10 scores to the full scorers' row ("full") or to the pre-beam's candidates ("part").
* The scorer set is espnet's: a scorer that is None or has weight 0 drops out (a model without decoder: CTC prefix beam search, with
  or without LM; a model without CTC head: attention beam search).  Scorers {ctc, length_bonus} without pre-beam are searched in ONE
  launch per batch (``tavsr_ctc_beam_search``: the beam's lattice stays in LDS), the host replaying its bookkeeping over the records.

``decode(enc, enc_lens)`` takes encoder outputs (``model.encode``), returns per utterance the ended hypotheses sorted
by score as (token ids incl. <sos>/<eos>, score).  ``Speech2Text`` wraps model + search like the reference's class.
"""
from __future__ import annotations

import math
import os
import time
from typing import Optional

import torch

from .. import ops
from ..utils.timestamps import timestamp_record
from .search_host import D_END, HostSearch

EPS = 1e-12
LOGZERO = -10000000000.0


def _cat(ws):
    return torch.cat([w.detach() for w in ws], dim=0).contiguous()


class _DerivedWeights:
    """The step objects keep a few DERIVED copies of parameters (q / k / v weights side by side for one launch, the LM's input
    table).  Everything else is read through the parameters' own storage.  ``sync()`` re-derives the copies IN PLACE (captured
    graphs keep reading the same buffers) when a source parameter's version counter has moved since they were made - an
    optimizer step or ``load_state_dict`` after the search object was built or between two decodes (validation while training)."""

    def __init__(self):
        self._derived = []          # (destination, source parameters)
        self._seen = ()             # the sources' versions when the copies were made / last re-derived

    def cat(self, ws):
        dst = _cat(ws)
        self._derived.append((dst, list(ws)))
        self._seen += tuple(w._version for w in ws)
        return dst

    def sync(self) -> bool:
        now = tuple(w._version for _, ws in self._derived for w in ws)
        if now == self._seen:
            return False
        for dst, ws in self._derived:
            torch.cat([w.detach() for w in ws], dim=0, out=dst)
        self._seen = now
        return True


# Route constants: module attributes read at call time (tests and scripts/decode_chain_probe.py flip them in-process); the two that
# name an environment variable take their default from it.
# the scorer step as one hipGraph, captured once per batch shape and replayed per token; False: eager launches, host in the loop
GRAPH_STEP = os.environ.get("TAVSR_DECODE_GRAPH", "1") != "0"
# the decoder's source attention (scores, mask, softmax, context) as one launch (csrc/attn_fused.hip); False: two GEMMs and a softmax
FUSED_STEP = True
SCORERS_PARALLEL = True   # the LM's chain on a side queue beside the decoder's (TAVSR_SINGLE_STREAM=1 disables every fork)
TREE_GROUP = 1            # tree attention: beams of an utterance side by side, in groups of TREE_GROUP * beam rows
# pre-beam top-k on the weighted full scores inside the CTC prefix launch (tavsr_ctc_prefix_step_topk; up to 64 candidates of up to
# 4096 tokens); False: torch.topk, then tavsr_ctc_prefix_step on its candidates
PREBEAM_FUSED = True
# per-token records on a queue of their own (TAVSR_RECORD_QUEUE=1) or on the search queue between two replays (default).  A queue of their
# own needs an event behind every replay that ANOTHER queue waits on - and that wait costs the NEXT replay ~1.5 us per launch it holds
# (scripts/graph_pair_probe.py: 60 launches +90 us, 190 launches +275 us; an event record alone, an eager launch or the 128-byte copy on
# the replaying queue itself: +5 us).  In the search: 633 -> 563 us per token at batch 1, 2359 -> 2188 at batch 64 (same process, alternating).
RECORD_QUEUE = os.environ.get("TAVSR_RECORD_QUEUE", "0") == "1"
LN_IN_EPILOGUE = True     # more than 32 rows: tavsr_gemm_ln at the x + f(x) -> norm(x) seams; False: a LayerNorm launch of its own
# Vocabularies of up to 64 tokens (character models), captured step: the CTC prefix scores of EVERY token are computed beside the LM's
# chain, in front of the decoder's - the recursion over the frames (20 us) leaves the critical path - and the whole beam update behind
# the scorers (LM log-softmax, pre-beam, weighted scores, top-k) is one launch (tavsr_beam_select_topk); False: CTC behind the scorers
CTC_BESIDE_SCORERS = True
# A CTC-only search without LM (scorers {ctc, length_bonus}, no pre-beam) has no neural chain per token: the whole search of an
# utterance is ONE launch, the beam's forward variables resident in LDS (tavsr_ctc_beam_search), where its shape fits
# (ops.ctc_beam_search_ok); False: token by token like every other scorer set
CTC_SEARCH_FUSED = True


class _Normed:
    """rows of the residual stream together with their LayerNorm under one particular (gamma, beta): what the launch that finished
    the rows leaves when it was told which norm follows (``_linear_res(..., ln_next=)``, GEMM path: tavsr_gemm_ln)"""
    __slots__ = ("x", "n", "gamma")

    def __init__(self, x, n, gamma):
        self.x, self.n, self.gamma = x, n, gamma

    @property
    def shape(self):
        return self.x.shape


def _rows(x):
    """the plain [N, d] tensor of a residual stream held as ``ops.RowParts`` / ``_Normed``"""
    if isinstance(x, _Normed):
        return x.x
    if isinstance(x, ops.RowParts):
        return x.t.sum(0)
    return x


def _ln_linear(x, norm, w, b, act=None):
    """act(W LN(x) + b): one launch (ops.rowlin) when the shapes allow, else LayerNorm + GEMM launches (no LayerNorm launch when
    the rows arrive with this norm already taken)."""
    if isinstance(x, _Normed):
        if x.gamma is norm[0]:
            return ops.linear(x.n, w, b, act=act)
        x = x.x
    if ops.rowlin_ok(x, w, ln=True):
        return ops.rowlin(x, w, b, ln=(norm[0], norm[1], EPS), act=act)
    n = ops.layernorm_fwd(_rows(x), *norm, EPS, save=False)[0]
    return ops.linear(n, w, b, act=act)


def _linear_res(x, w, b, res, ksplit=1, ln_next=None):
    """res + W x + b (``ksplit`` > 1: K dealt to that many blocks per column tile, the result an ``ops.RowParts``; a K the one-launch
    kernel only takes in slices - 2048 with more than 16 rows - is dealt to ``ops.ROWLIN_KSPLIT`` blocks whatever the caller asked).
    ``ln_next`` = (gamma, beta) of the LayerNorm the result goes through next: on the GEMM path (more than 32 rows) the launch that
    finishes the rows - the sum of the K-split slabs - also normalises them (``_Normed``)."""
    if isinstance(res, _Normed):
        res = res.x
    if ksplit == 1 and not ops.rowlin_ok(x, w) and ops.rowlin_ok(x, w, ksplit=max(2, ops.ROWLIN_KSPLIT)):
        ksplit = max(2, ops.ROWLIN_KSPLIT)
    if ksplit > 1 and ops.rowlin_ok(x, w, ksplit=ksplit):
        return ops.rowlin(x, w, b, res=res, ksplit=ksplit)
    if ops.rowlin_ok(x, w):
        return ops.rowlin(x, w, b, res=res)
    res = _rows(res)
    if ln_next is not None and LN_IN_EPILOGUE and w.shape[0] % 4 == 0 and w.shape[0] <= 2048:
        y, n = ops.linear(x, w, b, res=res, ln=(ln_next[0], ln_next[1], EPS))
        return _Normed(y, n, ln_next[0])
    return ops.linear(x, w, b, res=res)


def _ffn_step(x, norm, L, ln_next=None):
    """x + W2 relu(W1 LN(x) + b1) + b2 of one decoder / LM layer for the current token rows.  Hidden size 2048: the closing
    projection deals its K to ops.ROWLIN_KSPLIT blocks per column tile and the result stays a sum of that many tensors
    (``ops.RowParts``) until the next launches of the chain add them while they load their operands."""
    if not isinstance(x, _Normed) and ops.rowlin_ok(x, L["w1"], ln=True):
        t = ops.rowlin(x, L["w1"], L["b1"], ln=(norm[0], norm[1], EPS), act="relu")
        return _linear_res(t, L["w2"], L["b2"], x, ops.ROWLIN_KSPLIT if t.shape[1] == 2048 else 1)
    t = _ln_linear(x, norm, L["w1"], L["b1"], act="relu")
    return _linear_res(t, L["w2"], L["b2"], x, ln_next=ln_next)


class _DecoderStep:
    """espnet2 TransformerDecoder.forward_one_step with K/V kept per token instead of per-layer output caches."""

    def __init__(self, dec):
        self.dec = dec
        self.weights = _DerivedWeights()
        _cat = self.weights.cat
        self.D = dec.after_norm.weight.numel()
        self.H = dec.heads
        self.dk = self.D // self.H
        self.layers = []
        for l in dec.decoders:
            sa, ca, ff = l.self_attn, l.src_attn, l.feed_forward
            self.layers.append(dict(
                n1=(l.norm1.weight, l.norm1.bias), n2=(l.norm2.weight, l.norm2.bias), n3=(l.norm3.weight, l.norm3.bias),
                wqkv=_cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight]),
                bqkv=_cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias]),
                wo=sa.linear_out.weight, bo=sa.linear_out.bias,
                wq2=ca.linear_q.weight, bq2=ca.linear_q.bias,
                wkv2=_cat([ca.linear_k.weight, ca.linear_v.weight]), bkv2=_cat([ca.linear_k.bias, ca.linear_v.bias]),
                wo2=ca.linear_out.weight, bo2=ca.linear_out.bias,
                w1=ff.w_1.weight, b1=ff.w_1.bias, w2=ff.w_2.weight, b2=ff.w_2.bias))

    def start(self, enc, enc_lens, N, K, max_steps):
        U, T, D = enc.shape
        self.U, self.T, self.N, self.K = U, T, N, K
        self.enc_lens = enc_lens
        mem2 = enc.reshape(U * T, D)
        self.memkv = [ops.linear(mem2, L["wkv2"], L["bkv2"]) for L in self.layers]          # [U*T, 2D] per layer
        self.kpool = [ops.empty(max_steps * N, D, like=enc) for _ in self.layers]
        self.vpool = [ops.empty(max_steps * N, D, like=enc) for _ in self.layers]
        self.pe = self.dec.embed[1].table(max_steps, enc.device)
        self.emb = self.dec.embed[0].weight
        self.xscale = math.sqrt(D)

    def refill(self, enc):
        """a new batch of the same shape into the buffers a captured step reads (the source-attention keys / values)"""
        U, T, D = enc.shape
        mem2 = enc.reshape(U * T, D)
        for L, kv in zip(self.layers, self.memkv):
            ops.linear(mem2, L["wkv2"], L["bkv2"], out=kv, ldc=kv.stride(0))

    def step(self, i, tok, anc, dyn=None, rows=None, **score):
        """tok [N] last tokens, anc int32 [N, >= i+1] (column i already points at this step's rows) -> logp [N, V].
        ``dyn`` = (step_dev,): the step index - and with it the positional row - is read from a device buffer (``i`` is then the
        pool capacity in steps), so the launches can be captured once and replayed for every step.
        ``rows`` = (nkeys_row, pos_row, max_keys), int32 [N] each: rows at DIFFERENT depths (the time-synchronous search) - row n embeds
        position pos_row[n] and attends to its own nkeys_row[n] ancestors; a row with 0 keys does no attention and its result is not
        meant to be read (``i`` / ``dyn`` are not used)."""
        N, D, H, dk, U, T, K = self.N, self.D, self.H, self.dk, self.U, self.T, self.K
        if rows is not None:
            x = ops.embed_pe_rows(tok, self.emb, self.pe, self.xscale, rows[1])
        elif dyn is None:
            x = ops.embed_pe(tok.view(N, 1), self.emb, self.pe[i:i + 1].contiguous(), self.xscale).view(N, D)
        else:      # the positional row of the device-side step counter: read by the embedding launch itself
            x = ops.embed_pe(tok.view(N, 1), self.emb, self.pe, self.xscale, step_dev=dyn[0]).view(N, D)
        after = (self.dec.after_norm.weight, self.dec.after_norm.bias)
        for li, L in enumerate(self.layers):
            qkv = _ln_linear(x, L["n1"], L["wqkv"], L["bqkv"])
            # this step's keys / values are the last key of every hypothesis: the attention launch appends them to the pools
            if rows is not None:
                a = ops.tree_attn_rows(qkv[:, :D], self.kpool[li], self.vpool[li], anc, rows[0], rows[2], H, dk, qkv[:, D:2 * D],
                                       qkv[:, 2 * D:])
            else:
                a = ops.tree_attn_step(qkv[:, :D], self.kpool[li], self.vpool[li], anc, i + 1 if dyn is None else i, H, dk,
                                       step_dev=None if dyn is None else dyn[0], k_new=qkv[:, D:2 * D], v_new=qkv[:, 2 * D:],
                                       group=TREE_GROUP * self.K)
            x = _linear_res(a, L["wo"], L["bo"], x, ln_next=L["n2"])
            q2 = _ln_linear(x, L["n2"], L["wq2"], L["bq2"])
            # source attention: the K slots of an utterance are K query rows against that utterance's memory
            kv = self.memkv[li]
            if FUSED_STEP and dk == 64:      # scores, mask, softmax and context in one launch (csrc/attn_fused.hip)
                c2 = ops.attn_fwd(q2, 0, kv, 0, kv, D, U, K, T, H, dk, klens=self.enc_lens)[0]
            else:
                S = ops.pad4(T)
                sc = ops.empty(H, U, K, S, like=x)
                ops.gemm(K, T, dk, q2, D, kv, 2 * D, sc, S, nb1=U, nb2=H, sA=(K * D, dk), sB=(T * 2 * D, dk),
                         sC=(K * S, U * K * S))
                att = ops.softmax_fwd(sc, None, self.enc_lens, 1.0 / math.sqrt(dk), T2=T)
                c2 = ops.empty(N, D, like=x)
                ops.gemm(K, dk, T, att, S, kv, 2 * D, c2, D, b_off=D, b_kmajor=True, nb1=U, nb2=H, sA=(K * S, U * K * S),
                         sB=(T * 2 * D, dk), sC=(K * D, dk))
            x = _linear_res(c2, L["wo2"], L["bo2"], x, ln_next=L["n3"])
            x = _ffn_step(x, L["n3"], L, ln_next=self.layers[li + 1]["n1"] if li + 1 < len(self.layers) else after)
        z = _ln_linear(x, after, self.dec.output_layer.weight, self.dec.output_layer.bias)
        return ops.log_softmax_rows(z, **score)


class _LMStep:
    """espnet2 TransformerLM.batch_score (encoder.forward_one_step) with per-token K/V."""

    def __init__(self, lm):
        self.lm = lm
        self.weights = _DerivedWeights()
        _cat = self.weights.cat
        self.D, self.H = lm.att_unit, lm.heads
        self.dk = self.D // self.H
        self.layers = []
        for l in lm.encoder.encoders:
            a, ff = l.self_attn, l.feed_forward
            self.layers.append(dict(
                n1=(l.norm1.weight, l.norm1.bias), n2=(l.norm2.weight, l.norm2.bias),
                wqkv=_cat([a.linear_q.weight, a.linear_k.weight, a.linear_v.weight]),
                bqkv=_cat([a.linear_q.bias, a.linear_k.bias, a.linear_v.bias]),
                wo=a.linear_out.weight, bo=a.linear_out.bias,
                w1=ff.w_1.weight, b1=ff.w_1.bias, w2=ff.w_2.weight, b2=ff.w_2.bias))

    def start(self, like, N, max_steps, K=1):
        self.N, self.K = N, K
        # the LM's input layer (embedding -> Linear -> LayerNorm -> ReLU; espnet TransformerLM with pos_enc: null) depends on the token
        # alone: one [V, d] table per search instead of three launches per token
        self.in_table = self._input_table()
        emb = self.lm.encoder.embed
        self._table_ver = tuple(w._version for w in (self.lm.embed.weight, emb[0].weight, emb[0].bias, emb[1].weight, emb[1].bias))
        self.kpool = [ops.empty(max_steps * N, self.D, like=like) for _ in self.layers]
        self.vpool = [ops.empty(max_steps * N, self.D, like=like) for _ in self.layers]

    def _input_table(self):
        lm = self.lm
        emb = lm.encoder.embed
        t = ops.linear(lm.embed.weight.contiguous(), emb[0].weight, emb[0].bias)
        t = ops.layernorm_fwd(t, emb[1].weight, emb[1].bias, EPS, save=False)[0]
        return ops.act_(t, "relu")

    def sync_weights(self):
        """derived copies after a change of the LM's parameters: the q / k / v concatenations and - into the buffer a captured step
        gathers from - the input table (one small GEMM, a LayerNorm, a ReLU)"""
        lm = self.lm
        emb = lm.encoder.embed
        src = (lm.embed.weight, emb[0].weight, emb[0].bias, emb[1].weight, emb[1].bias)
        ver = tuple(w._version for w in src)
        changed = self.weights.sync()
        if getattr(self, "in_table", None) is not None and (changed or ver != self._table_ver):
            self.in_table.copy_(self._input_table())
        self._table_ver = ver

    def step(self, i, tok, anc, dyn=None, logits_only=False, rows=None, **score):
        """``rows``: as ``_DecoderStep.step`` (the LM embeds no position: its key counts alone are used)"""
        N, D, H, dk = self.N, self.D, self.H, self.dk
        lm = self.lm
        # the token's row of the input table is gathered by the first layer's launches themselves where the one-launch Linear
        # runs (its ``gather`` / ``res_gather`` operands): no gather launch at the head of the LM's chain
        after = (lm.encoder.after_norm.weight, lm.encoder.after_norm.bias)
        fold = ops.rowlin_ok(self.in_table, self.layers[0]["wqkv"], n_rows=N, ln=True)
        h = None if fold else self.in_table.index_select(0, tok)
        for li, L in enumerate(self.layers):
            if li == 0 and fold:
                qkv = ops.rowlin(self.in_table, L["wqkv"], L["bqkv"], ln=(L["n1"][0], L["n1"][1], EPS), gather=tok)
            else:
                qkv = _ln_linear(h, L["n1"], L["wqkv"], L["bqkv"])
            # this step's keys / values are the last key of every hypothesis: the attention launch appends them to the pools
            if rows is not None:
                a = ops.tree_attn_rows(qkv[:, :D], self.kpool[li], self.vpool[li], anc, rows[0], rows[2], H, dk, qkv[:, D:2 * D],
                                       qkv[:, 2 * D:])
            else:
                a = ops.tree_attn_step(qkv[:, :D], self.kpool[li], self.vpool[li], anc, i + 1 if dyn is None else i, H, dk,
                                       step_dev=None if dyn is None else dyn[0], k_new=qkv[:, D:2 * D], v_new=qkv[:, 2 * D:],
                                       group=TREE_GROUP * self.K)
            if li == 0 and fold:
                h = ops.rowlin(a, L["wo"], L["bo"], res=self.in_table, res_gather=tok)
            else:
                h = _linear_res(a, L["wo"], L["bo"], h, ln_next=L["n2"])
            h = _ffn_step(h, L["n2"], L, ln_next=self.layers[li + 1]["n1"] if li + 1 < len(self.layers) else after)
        z = _ln_linear(h, after, lm.decoder.weight, lm.decoder.bias)
        return z if logits_only else ops.log_softmax_rows(z, **score)


class BatchBeamSearch:
    def __init__(self, model, lm=None, beam_size: int = 10, ctc_weight: float = 0.1, lm_weight: float = 0.6,
                 penalty: float = 0.5, maxlenratio: float = 0.0, minlenratio: float = 0.0, skip_zero_weight: bool = False,
                 ngram=None, ngram_weight: float = 0.9, ngram_scorer: str = "full"):
        if not (0.0 <= ctc_weight <= 1.0):
            raise ValueError(f"ctc_weight must lie in [0, 1]: {ctc_weight}")
        # The scorer set is espnet's (BeamSearch.__init__ drops a scorer that is None or has weight 0; avsr_inference.py:141-153):
        # a model without decoder (ctc_weight 1.0 in its model_conf) or without CTC head (0.0) is searched with what it has.  A model
        # that has BOTH modules keeps every launch it had whatever ctc_weight says - a scorer of weight 0 still runs and enters the sums
        # with weight 0 (finite log-probabilities), which selects the same hypotheses - unless ``skip_zero_weight`` asks for espnet's set.
        hybrid = model.decoder is not None and model.ctc is not None
        drop = skip_zero_weight or not hybrid
        self.has_dec = model.decoder is not None and not (drop and 1.0 - ctc_weight == 0.0)
        self.has_ctc = model.ctc is not None and not (drop and ctc_weight == 0.0)
        self.has_lm = lm is not None and lm_weight != 0.0
        # the n-gram scorer (tavsr/lm/ngram.py:NgramLM; avsr_inference.py:166-178): "full" - its weighted row joins the full scorers' row
        # in front of the pre-beam; "part" - it is added to the pre-beam's candidates only, behind the pre-beam (espnet's partial scorers
        # score part_ids alone).  None or weight 0 drops it, as every scorer.
        if ngram_scorer not in ("full", "part"):
            raise ValueError(f"ngram_scorer must be 'full' or 'part': {ngram_scorer!r}")
        self.ngram, self.w_ngram, self.ngram_scorer = ngram, float(ngram_weight), ngram_scorer
        if ngram is not None and ngram.word_map.numel() != len(model.token_list):
            raise ValueError(f"the n-gram's word map has {ngram.word_map.numel()} tokens, the model's token list {len(model.token_list)}: "
                             "build it with NgramLM.from_arpa(path, model.token_list, device)")
        if not self.has_dec and not self.has_ctc:
            raise ValueError(f"no scorer is left to search with: the model has {'no' if model.decoder is None else 'a'} decoder and "
                             f"{'no' if model.ctc is None else 'a'} CTC head, and ctc_weight = {ctc_weight} gives the one it has weight 0. "
                             f"Set ctc_weight to {1.0 if model.decoder is None else 0.0}")
        # espnet BeamSearch.forward: maxlenratio == 0 -> up to T tokens with end detection; > 0 -> max(1, int(ratio * T)) tokens,
        # < 0 -> -int(ratio) tokens, both without end detection; minlenratio is accepted and (as in espnet 202402) only logged
        self.maxlenratio, self.minlenratio = float(maxlenratio), float(minlenratio)
        self.model, self.lm = model, lm
        self.K = beam_size
        self.V = len(model.token_list)
        self.sos, self.eos = model.sos, model.eos
        self.w_dec, self.w_ctc = 1.0 - ctc_weight, ctc_weight
        self.w_lm = lm_weight if lm is not None else 0.0
        self.w_len = penalty
        # avsr_inference.py:298: pre_beam_score_key = None when ctc_weight == 1 -> the CTC prefix scorer sees every token
        self.C = self.V if ctc_weight == 1.0 else min(int(1.5 * beam_size), self.V)
        # espnet's do_pre_beam: a partial scorer is present, ctc_weight != 1 (pre_beam_score_key = None there) and fewer candidates than tokens
        self.pre_beam = self.has_ctc and ctc_weight != 1.0 and int(1.5 * beam_size) < self.V
        if self.pre_beam and not self.has_dec and not self.has_lm and not (self.has_ngram and not self._ngram_part):
            raise ValueError(f"ctc_weight = {ctc_weight} on a model without decoder and without LM: the pre-beam of the CTC prefix scorer "
                             "would rank the length bonus alone, a constant - which candidates it keeps is not defined.  Set "
                             "ctc_weight: 1.0 (CTC prefix beam search over every token), or add an LM or a full n-gram scorer")
        self._pinned = None
        self._copy_q = None        # the queue the per-token records leave on (created with the first captured search)
        self._captured = None      # the captured step of the last batch shape (buffers + hipGraph), re-used while the shape repeats
        self.n_steps = None        # tokens searched per utterance in the last decode()
        self.dec_step = _DecoderStep(model.decoder) if self.has_dec else None
        self.lm_step = _LMStep(lm) if self.has_lm else None

    @property
    def scorers(self):
        """names of the scorers the search runs (espnet's keys)"""
        return tuple(k for k, on in (("decoder", self.has_dec), ("ctc", self.has_ctc), ("length_bonus", True), ("lm", self.has_lm),
                                     ("ngram", self.has_ngram)) if on)

    @property
    def has_ngram(self):
        return self.ngram is not None and self.w_ngram != 0.0

    @property
    def _ngram_part(self):
        """the n-gram behind the pre-beam, on its candidates alone; without pre-beam "part" is "full" (every token is a candidate)"""
        return self.has_ngram and self.ngram_scorer == "part" and self.pre_beam

    @property
    def _ctc_all_tokens(self):
        """The one real difference between a hybrid model's step and the step with the decoder absent, where there is NO pre-beam:
        without decoder the CTC launch gets no candidate list (``cand=None``) and scores every token with explicit fma sums, bit-equal
        to the one-launch search.  A hybrid model without pre-beam (ctc_weight 1.0 without ``skip_zero_weight``, or int(1.5 beam) >= V)
        keeps handing the launch a candidate list - every token, or its top-C row - whose sums are the source-expression form.
        Unifying the two would move bits for hybrid models."""
        return self.has_ctc and not self.has_dec and not self.pre_beam

    def _ctc_logp(self, enc, out=None):
        """log-softmax of the CTC head over every frame [U, T, V] (``out``: into a captured step's buffer)"""
        U, T, D = enc.shape
        ctc = self.model.ctc
        z = ops.linear(enc.reshape(U * T, D), ctc.ctc_lo.weight, ctc.ctc_lo.bias)
        return ops.log_softmax_rows(z, out=None if out is None else out.view(U * T, self.V)).view(U, T, self.V)

    @torch.no_grad()
    def decode(self, enc: torch.Tensor, enc_lens: torch.Tensor, nbest: Optional[int] = None):
        """enc [U, T, D] encoder outputs, enc_lens [U] -> per utterance [(yseq list incl. sos/eos, score), ...] sorted."""
        U, T, D = enc.shape
        dev = enc.device
        enc = enc.contiguous().float()
        enc_lens = enc_lens.to(dev).to(torch.int64)
        lens_h = [int(v) for v in enc_lens.cpu()]
        host = HostSearch(self.maxlenratio, lens_h, self.K, self.sos, self.eos)
        if self.has_ctc and any(m > t for m, t in zip(host.maxl, lens_h)):
            # espnet's CTCPrefixScoreTH indexes its forward variables by output length: a hypothesis longer than the number
            # of frames raises IndexError there; refused up front here
            raise ValueError(f"maxlenratio {self.maxlenratio} asks for more tokens than encoder frames {lens_h}: "
                             "the CTC prefix scorer cannot score a prefix longer than its input")
        # derived weight copies follow the parameters (an optimizer step / load_state_dict since they were made): ADVICE rounds 4, 5
        if self.has_dec:
            self.dec_step.weights.sync()
        if self.has_lm:
            self.lm_step.sync_weights()
        if self.has_ngram and self.ngram.device != dev:
            raise ValueError(f"the n-gram's tables are on {self.ngram.device}, the encoder outputs on {dev}: move them with NgramLM.to(device)")
        # scorers {ctc, length_bonus} without pre-beam: the whole search is one launch where the beam's lattice fits a workgroup's LDS
        if self._ctc_all_tokens and not self.has_lm and not self.has_ngram and CTC_SEARCH_FUSED and ops.ctc_beam_search_ok(self.K, self.V, T):
            self._search_one_launch(enc, enc_lens, host)
        else:
            # A captured step is tied to its buffers, not to a batch: while the shape (utterances, frames, token budget) repeats -
            # a stream of 4 s clips - the buffers are refilled in place and the hipGraph of the previous call is replayed; capture
            # and warm-up were 8-10 ms of a 95 ms batch-1 search.
            key = (U, T, D, host.steps, str(dev), self.scorers, self._ngram_part)
            cap = self._captured
            if GRAPH_STEP and cap is not None and cap.key == key:
                self._refill(cap, enc, enc_lens, host)
            else:
                self._captured = None
                beam = self._start(enc, enc_lens, host.steps)
                cap = self._captured = self._capture(key, beam, host) if GRAPH_STEP else None
            if cap is not None:
                self._search_replayed(cap, host)
            else:
                self._search_eager(beam, host)
        self.n_steps = host.n_host.tolist()
        return host.nbest(nbest)

    def _search_one_launch(self, enc, enc_lens, host):
        """One launch searches every utterance to its end (tavsr_ctc_beam_search: records, retiring and end detection on the device);
        the host then replays its own per-token processing over the records of the tokens the device searched."""
        U, T, D = enc.shape
        key = ("ctc_search", U, T, D, host.steps, str(enc.device))
        cap = self._captured
        if cap is None or cap.key != key:
            cap = self._captured = _Captured(key, None, _OneLaunchBuffers(enc, self.K, self.V, host.steps))
        b = cap.bufs
        b.enc_lens.copy_(enc_lens)
        b.maxl.copy_(torch.tensor(host.maxl, dtype=torch.int32))
        self._ctc_logp(enc, out=b.logp_ctc)
        ops.ctc_beam_search(b.logp_ctc, b.enc_lens, b.maxl, b.hist, b.n_steps, self.K, self.sos, self.eos, self.w_ctc, self.w_len,
                            self.maxlenratio == 0.0, D_END)
        n_dev = b.n_steps.cpu()
        rec = b.hist[:int(n_dev.max())].cpu()
        for i in range(rec.shape[0]):
            host.step_from_records(rec, i)
        if bool(host.active.any()) or not torch.equal(host.n_host, n_dev):
            raise RuntimeError(f"tavsr_ctc_beam_search stopped after {n_dev.tolist()} tokens per utterance, the host's end detection "
                               f"over its records after {host.n_host.tolist()} (still searching: {host.active.tolist()})")

    def _start(self, enc, enc_lens, steps):
        """a batch of a new shape: CTC log-probabilities, the scorers' per-search buffers, the beam's running state"""
        U, T, _ = enc.shape
        enc_lens = enc_lens.clone()
        logp_ctc = self._ctc_logp(enc) if self.has_ctc else None
        if self.has_dec:
            self.dec_step.start(enc, enc_lens, U * self.K, self.K, steps)
        if self.has_lm:
            self.lm_step.start(enc, U * self.K, steps, self.K)
        return _Beam(self, logp_ctc, enc_lens, T, steps)

    def _refill(self, cap, enc, enc_lens, host):
        """the next batch of a captured step's shape into the buffers its graph reads"""
        beam = cap.bufs
        beam.enc_lens.copy_(enc_lens)
        if self.has_ctc:
            self._ctc_logp(enc, out=beam.logp_ctc)
        if self.has_dec:
            self.dec_step.refill(enc)
        beam.reset()
        cap.dyn.reset()
        cap.dyn.maxl.copy_(torch.tensor(host.maxl, dtype=torch.int32))

    def _capture(self, key, beam, host):
        """One token costs ~300 scorer launches plus ~90 small ones for the beam update, all on [N, d]-sized operands.
        The whole device side of a step is captured once per batch shape - the step index, the positional row, tokens,
        ancestor lists, CTC state and scores live in fixed device buffers updated in place - and replayed per token;
        the device also retires ended hypotheses itself and records (token, back-pointer, score) per slot and token, so
        the host neither uploads anything nor sits on the critical path: it reads the records one token behind the
        device (end detection, collecting ended hypotheses by back-tracking) while the next step already runs.
        The step is bound by its chain of dependent small kernels (5-6 us each), not by the host: what shortens it is
        fewer launches - the K/V append rides in the attention launch, the scorer weights in the log-softmax
        launches, the beam update is three launches (beam_combine, top-k, beam_reorder) plus one commit."""
        dyn = _StepCounters(beam, host.maxl, host.steps, self.V)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._device_step(beam, host.steps, dyn)            # warm-up outside the capture; the state is reset below
            beam.reset()
            dyn.reset()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._device_step(beam, host.steps, dyn)
        return _Captured(key, graph, beam, dyn)

    def _device_step(self, b, i, dyn=None, cand_all=None):
        """everything the device does for one token: the scorers, the pre-beam, CTC prefix scores of the candidates, the beam update
        and the re-ordering of the running state ``b``.  ``dyn`` = None: eager launches with the host's step index i (``cand_all``:
        every token as a candidate list, where ``_ctc_all_tokens``).  ``dyn`` = device counters: every buffer is updated IN PLACE and the
        step index is read from device memory, so the whole step is one captured hipGraph (i is then the pool capacity in steps;
        hypotheses that ended with the previous token have left the beam and column `step` of the ancestor lists is filled: the
        previous step's re-ordering launch did both, ``reset()`` for step 0)."""
        has_dec, has_ctc, has_lm = self.has_dec, self.has_ctc, self.has_lm
        if dyn is None:
            b.anc[:, i] = b.slot_ids + i * b.tok.numel()
            sd = sdyn = None
        else:
            sd, sdyn, cand_all = dyn.step, (dyn.step,), dyn.cand_all
        # the CTC scores of every token beside the scorers and the beam update behind them in one launch (CTC_BESIDE_SCORERS)
        # (an n-gram behind the pre-beam needs the candidates before the weighted sum: the launches behind the scorers one by one)
        spec = (dyn is not None and CTC_BESIDE_SCORERS and ops.beam_select_topk_ok(self.K, self.V) and self.C <= self.V
                and not self._ngram_part)
        z_lm = None
        if has_lm:                   # the two scorers are independent chains of small launches: the LM runs beside the decoder
            with ops.BranchScope(enabled=SCORERS_PARALLEL) as br:
                z_lm = self.lm_step.step(i, b.tok, b.anc, sdyn, logits_only=True)
        ctc = (None,) * 6
        if spec and has_ctc:
            # on the decoder's queue, in front of its chain: the decoder has ~100 us of slack behind the LM (a third queue for it
            # made the whole step 45 us SLOWER: profiles/r05_notes.md)
            ctc = self._ctc_prefix(b, i, sd, cand_all)
        # full = w_dec * decoder + w_lm * lm + w_len (LengthBonus: 1 per token), summed by the scorers' last launches
        dec = self.dec_step.step(i, b.tok, b.anc, sdyn, alpha=self.w_dec, add=0.0 if has_lm else self.w_len) if has_dec else None
        if self.has_ngram and not self._ngram_part:
            # the n-gram's weighted row lands on the decoder's (behind its chain, on its queue); without decoder it opens the row and
            # carries the length bonus where no LM launch follows to carry it
            dec = ops.ngram_score(self.ngram, b.yseq, i, out=dec, alpha=self.w_ngram, add=0.0 if (has_dec or has_lm) else self.w_len,
                                  accumulate=has_dec, step_dev=sd)
        if has_lm:
            br.join()
        if spec:
            cand, r_new, psi, psi_abs, eos_s, eos_abs = ctc
            top = ops.beam_select_topk(dec, z_lm, self.w_lm, self.w_len if (has_lm or dec is None) else 0.0, psi, psi_abs, eos_s, eos_abs,
                                       b.s_prev, b.score, self.eos, self.w_ctc, self.K, self.C)
            return self._commit(b, dyn, top, cand, r_new, psi_abs)
        full = self._full_row(b, dec, z_lm)
        if has_ctc:
            ctc = self._ctc_prefix(b, i, sd, cand_all, full)
        if self._ngram_part:             # behind the pre-beam: onto its candidates alone (the refusal above: ``full`` is a row of this step)
            ops.ngram_score(self.ngram, b.yseq, i, out=full, alpha=self.w_ngram, accumulate=True, step_dev=sd, cand=ctc[0])
        if dyn is not None:
            return self._beam_update_captured(b, dyn, full, *ctc)
        return self._beam_update_eager(b, i, full, *ctc)

    def _full_row(self, b, dec, z_lm):
        """the full scorers' weighted row [N, V] behind their chains: the LM's log-softmax lands on the decoder's row (``dec``: the
        decoder's and / or the full n-gram's); no decoder, no n-gram and no LM: the length bonus alone"""
        if dec is None:
            return b.full_const if z_lm is None else ops.log_softmax_rows(z_lm, alpha=self.w_lm, add=self.w_len)
        if z_lm is not None:
            ops.log_softmax_rows(z_lm, out=dec, alpha=self.w_lm, add=self.w_len, accumulate=True)
        return dec

    def _ctc_prefix(self, b, i, sd, cand_all, full=None):
        """CTC prefix scores -> (cand, r_new, psi, psi_abs, eos_s, eos_abs), in one of three forms: of every token (``full`` None: in
        front of the scorers; or ``_ctc_all_tokens``), of the pre-beam's candidates with the top-k in the launch, or behind torch.topk"""
        state = (b.logp_ctc, b.enc_lens, b.r_prev, b.s_prev, b.tok)
        if full is None or self._ctc_all_tokens:
            return (cand_all,) + tuple(ops.ctc_prefix_step(*state, None if self._ctc_all_tokens else cand_all, self.K, i, step_dev=sd))
        if PREBEAM_FUSED and self.C <= 64 and self.V <= 4096:            # pre-beam on the weighted full scores inside the CTC launch
            return ops.ctc_prefix_step_topk(*state, full, self.C, self.K, i, step_dev=sd)
        cand = torch.topk(full, self.C, dim=-1)[1]
        return (cand,) + tuple(ops.ctc_prefix_step(*state, cand, self.K, i, step_dev=sd))

    def _beam_update_captured(self, b, dyn, full, cand, r_new, psi, psi_abs, eos_s, eos_abs):
        """weighted scores and top-k of a captured step (one launch where K * V fits, else two); same arithmetic as the torch ops
        of ``_beam_update_eager``"""
        if ops.beam_combine_topk_ok(self.K, self.V):
            top = ops.beam_combine_topk(full, cand, psi, psi_abs, eos_s, eos_abs, b.s_prev, b.score, self.eos, self.w_ctc, self.K)
        else:
            weighted = ops.beam_combine(full, cand, psi, psi_abs, eos_s, eos_abs, b.s_prev, b.score, self.eos, self.w_ctc)
            top = torch.topk(weighted.view(b.U, self.K * self.V), self.K, dim=-1)
        return self._commit(b, dyn, top, cand, r_new, psi_abs)

    def _commit(self, b, dyn, top, cand, r_new, psi_abs):
        """gather of the extended slots' state into the shadow buffers (+ the records, retiring, the next step's ancestor column), then
        one multi-buffer commit that also counts the step"""
        top_s, top_i = top
        ops.beam_reorder(top_i, top_s, cand, r_new, psi_abs, b.yseq, b.anc, dyn.shadow, self.K, self.V, dyn.step, hist=dyn.hist,
                         maxlen=dyn.maxl, eos=self.eos)
        ops.multi_copy_(b.live(), [t for t in dyn.shadow if t is not None], inc=dyn.ctr)

    def _beam_update_eager(self, b, i, full, cand, r_new, psi, psi_abs, eos_s, eos_abs):
        """the beam update in torch ops; the running state is rebound to the gathered tensors"""
        N, V, score = b.tok.numel(), self.V, b.score
        if self.has_ctc:
            is_eos_c = cand == self.eos
            psi = torch.where(is_eos_c, eos_s.unsqueeze(1), psi)
            psi_abs = torch.where(is_eos_c, eos_abs.unsqueeze(1), psi_abs)
            ctc_full = torch.full((N, V), LOGZERO, device=score.device) - b.s_prev.unsqueeze(1)
            ctc_full[:, self.eos] = eos_s
            ctc_full.scatter_(1, cand, psi)
            weighted = full + self.w_ctc * ctc_full + score.unsqueeze(1)
        else:
            weighted = full + score.unsqueeze(1)
        top_s, top_i = torch.topk(weighted.view(b.U, self.K * V), self.K, dim=-1)
        prev = (top_i // V + b.utt_base).view(N)                # slot the new hypothesis extends
        new_tok = (top_i % V).view(N)
        if self.has_ctc:                                        # CTC state of the chosen candidate
            cidx = (cand[prev] == new_tok.unsqueeze(1)).float().argmax(dim=1)
            b.r_prev, b.s_prev = r_new[prev, :, :, cidx], psi_abs[prev, cidx]
        yseq = b.yseq[prev]
        yseq[:, i + 1] = new_tok
        b.yseq, b.score, b.anc, b.tok = yseq, top_s.view(N), b.anc[prev], new_tok

    def _search_eager(self, b, host):
        """token by token with the host in the loop: eager launches, the host's step index"""
        dev, N = b.tok.device, b.tok.numel()
        cand_all = torch.arange(self.V, dtype=torch.int64, device=dev).repeat(N, 1) if self._ctc_all_tokens else None
        for i in range(host.steps):
            self._device_step(b, i, None, cand_all)
            yseq, score = b.yseq, b.score
            kill = host.step(i, b.tok.cpu(), score.cpu(), lambda idx: yseq[idx.to(dev)].cpu().tolist())
            if bool(kill.any()):
                b.score = torch.where(kill.to(dev), torch.full_like(score, -float("inf")), score)
            if not bool(host.active.any()):
                break

    def _search_replayed(self, cap, host):
        """one graph replay per token; the host processes the records one token behind the device"""
        graph, hist = cap.graph, cap.dyn.hist
        steps, _, N = hist.shape
        need = steps * 3 * N                                    # page-locked landing zone of the records: ONE buffer that
        if self._pinned is None or self._pinned.numel() < need:   # grows to the largest search seen
            self._pinned = torch.empty(max(need, 1 << 16), dtype=torch.int32, pin_memory=True)
        pin = self._pinned[:need].view(steps, 3, N)             # pin[token][0 / 1 / 2][slot]
        events, done = [], 0
        timing = os.environ.get("TAVSR_DECODE_TIMING") == "1"   # host-side cost of a token: replay call / record processing
        t_replay = t_host = t_wait = 0.0
        # the record of token i leaves behind step i on the search queue itself (see RECORD_QUEUE for the queue of their own the
        # records had, and what the event it needs costs the next replay)
        main_q = torch.cuda.current_stream()
        if self._copy_q is None:
            self._copy_q = torch.cuda.Stream() if RECORD_QUEUE else main_q
        copy_q = self._copy_q
        copy_q.wait_stream(main_q)
        for i in range(steps):
            t0 = time.perf_counter()
            graph.replay()
            if copy_q is not main_q:
                stepped = torch.cuda.Event()
                stepped.record(main_q)
                copy_q.wait_event(stepped)
            with torch.cuda.stream(copy_q):
                pin[i].copy_(hist[i], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_q)
            events.append(ev)
            t1 = time.perf_counter()
            while done < i and bool(host.active.any()):         # the host works one token behind the device
                events[done].synchronize()
                t2 = time.perf_counter()
                host.step_from_records(pin, done)
                done += 1
                t_wait += t2 - t1
                t_host += time.perf_counter() - t2
            t_replay += t1 - t0
            if not bool(host.active.any()):
                break
        if timing:
            n_ = max(1, len(events))
            print(f"decode timing (host, per token, N = {N}): replay + copy + event {1e6 * t_replay / n_:.0f} us, waiting for the "
                  f"device {1e6 * t_wait / n_:.0f} us, record processing {1e6 * t_host / n_:.0f} us", flush=True)
        while done < len(events) and bool(host.active.any()):
            events[done].synchronize()
            host.step_from_records(pin, done)
            done += 1
        main_q.wait_stream(copy_q)
        main_q.synchronize()                                    # a step the device ran ahead may still be in flight


class _Beam:
    """the running state of a token-by-token search in device buffers: a captured step updates them in place (and ``reset()`` starts
    the next search in them), the eager route rebinds them step by step"""

    def __init__(self, search, logp_ctc, enc_lens, T, steps):
        K, V, dev = search.K, search.V, enc_lens.device
        U = enc_lens.numel()
        N = U * K
        self.U, self.K, self.sos, self.eos = U, K, search.sos, search.eos
        self.logp_ctc, self.enc_lens = logp_ctc, enc_lens
        self.tok = torch.full((N,), self.sos, dtype=torch.int64, device=dev)
        self.yseq = torch.full((N, steps + 2), self.eos, dtype=torch.int64, device=dev)
        self.yseq[:, 0] = self.sos
        score = torch.full((U, K), -float("inf"), device=dev)
        score[:, 0] = 0.0                                          # one <sos> hypothesis per utterance
        self.score = score.view(N)
        self.anc = torch.zeros(N, steps, dtype=torch.int32, device=dev)       # per hypothesis the key / value rows of its history
        self.slot_ids = torch.arange(N, dtype=torch.int32, device=dev)
        self.r_prev = torch.zeros(N, T, 2, device=dev) if search.has_ctc else None
        self.s_prev = torch.zeros(N, device=dev) if search.has_ctc else None
        self.utt_base = (torch.arange(U, device=dev) * K).view(U, 1)
        # no decoder and no LM: the full scorers' row is the length bonus alone
        self.full_const = torch.full((N, V), search.w_len, device=dev) if not search.has_dec and not search.has_lm else None

    def live(self):
        """the buffers a step's commit overwrites, in the order of ``_StepCounters.shadow``"""
        return [t for t in (self.r_prev, self.s_prev) if t is not None] + [self.yseq, self.anc, self.tok, self.score]

    def reset(self):
        self.tok.fill_(self.sos)
        self.yseq.fill_(self.eos)
        self.yseq[:, 0] = self.sos
        self.score.fill_(-float("inf"))
        self.score.view(self.U, self.K)[:, 0] = 0.0
        self.anc.zero_()
        self.anc[:, 0] = self.slot_ids                            # step 0's own key / value rows
        if self.r_prev is not None:
            self.r_prev.zero_()
            self.s_prev.zero_()


class _StepCounters:
    """what a captured step reads and writes beside the beam: the device-side step counter, the token budgets, the per-token records
    (token, back-pointer, score bits), every token as a candidate list of the CTC scorer, the shadow buffers of the beam update"""

    def __init__(self, beam, maxl, steps, V):
        dev, N = beam.tok.device, beam.tok.numel()
        self.ctr = torch.tensor([0, 1], dtype=torch.int64, device=dev)          # (i, i + 1), counted by the commit launch
        self.step = self.ctr.view(torch.int32)[0:1]                             # the kernels read i as int32 (low word: little endian)
        self.maxl = torch.tensor(maxl, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(steps, 3, N, dtype=torch.int32, device=dev)
        self.cand_all = torch.arange(V, dtype=torch.int64, device=dev).repeat(N, 1) if beam.r_prev is not None else None
        self.shadow = tuple(None if t is None else torch.empty_like(t)
                            for t in (beam.r_prev, beam.s_prev, beam.yseq, beam.anc, beam.tok, beam.score))

    def reset(self):
        self.ctr.copy_(torch.tensor([0, 1], dtype=torch.int64))


class _OneLaunchBuffers:
    """operands and results of the one-launch CTC search (tavsr_ctc_beam_search), re-used while the shape repeats"""

    def __init__(self, enc, K, V, steps):
        U, T, _ = enc.shape
        dev = enc.device
        self.logp_ctc = ops.empty(U, T, V, like=enc)
        self.enc_lens = torch.empty(U, dtype=torch.int64, device=dev)
        self.maxl = torch.empty(U, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(steps, 3, U * K, dtype=torch.int32, device=dev)
        self.n_steps = torch.zeros(U, dtype=torch.int32, device=dev)


class _Captured:
    """what a decode() keeps for the next batch of the same shape: the captured step (``graph``; None on the one-launch route), the
    buffers it reads and writes (``bufs``: ``_Beam`` / ``_OneLaunchBuffers``) and its device counters (``dyn``)"""

    def __init__(self, key, graph, bufs, dyn=None):
        self.key, self.graph, self.bufs, self.dyn = key, graph, bufs, dyn

    def __getitem__(self, name):
        """the keyed view of the same objects that earlier callers read: ``["graph"]``, ``["logp_ctc"]``, ``["bufs"][5]`` (r_prev)"""
        if name == "bufs":
            b = self.bufs
            return (b.tok, b.yseq, b.score, b.anc, b.slot_ids, b.r_prev, b.s_prev, b.utt_base)
        for o in (self, self.bufs, self.dyn):
            if hasattr(o, name):
                return getattr(o, name)
        raise KeyError(name)


class CapturedEncode:
    """``model.encode`` of an eval-mode model as a replayed hipGraph while the input shapes repeat (a stream of equally long clips):
    at batch 1 the encoder is ~600 launches of a few microseconds each, i.e. host-bound when enqueued one by one.  Inputs are
    copied into the capture's buffers, outputs are the capture's buffers (valid until the next call).  Lengths are device data the
    kernels read, so utterances of different lengths inside one padded shape replay the same graph; another shape captures anew.
    (The reference encodes eagerly, avsr_inference.py:449-470; results are the same launches' results.)"""

    def __init__(self, model, max_batch: int = 8):
        self.model, self.max_batch = model, max_batch      # (larger batches keep the GPU busy without a graph)
        self._cap = None

    @torch.no_grad()
    def __call__(self, *batch):
        if self.model.training or batch[0].shape[0] > self.max_batch or not all(t.is_cuda for t in batch):
            return self.model.encode(*batch)
        key = tuple((tuple(t.shape), t.dtype) for t in batch)
        cap = self._cap
        if cap is None or cap["key"] != key:
            static = [t.clone() for t in batch]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.model.encode(*static)                 # warm-up outside the capture (lazy buffers, allocator pools)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self.model.encode(*static)
            cap = self._cap = dict(key=key, static=static, graph=graph, out=out)
        else:
            for s_, t in zip(cap["static"], batch):
                s_.copy_(t)
        cap["graph"].replay()
        return cap["out"]


class Speech2Text:
    """src/inference/avsr_inference.py:Speech2Text for models that are already built: encode + beam search, results as
    the reference returns them (:492-518): (text, tokens, token ids without sos/eos/blank, (yseq, score))."""

    def __init__(self, asr_model, lm=None, beam_size: int = 20, ctc_weight: float = 0.5, lm_weight: float = 1.0,
                 penalty: float = 0.0, nbest: int = 1, maxlenratio: float = 0.0, minlenratio: float = 0.0,
                 skip_zero_weight: bool = False, timestamps: bool = False, frame_seconds: float = 0.04,
                 ngram_file: Optional[str] = None, ngram_scorer: str = "full", ngram_weight: float = 0.9, time_sync: bool = False,
                 transducer_conf: Optional[dict] = None):
        # timestamps: every returned hypothesis is aligned to its utterance's CTC posteriors after the search (one launch of
        # tavsr_ctc_align for the whole batch) and its result tuple gains a fifth element, the record of utils/timestamps.py.
        # frame_seconds: one encoder frame - 10 ms hop x 4 subsampling for audio, 25 fps for video: 0.04 s in every shipped recipe.
        if timestamps and asr_model.ctc is None:
            raise ValueError("timestamps need the CTC head: this model was built without one (ctc_weight: 0.0)")
        if timestamps and not frame_seconds > 0.0:
            raise ValueError(f"frame_seconds must be positive: {frame_seconds}")
        self.timestamps, self.frame_seconds = bool(timestamps), float(frame_seconds)
        self.asr_model = asr_model.eval()
        self.lm = None if lm is None else lm.eval()
        self.nbest = nbest
        self.encode = CapturedEncode(self.asr_model)
        # a transducer model is searched by BeamSearchTransducer(beam_size=beam_size, **transducer_conf) (avsr_inference.py:181-207):
        # greedy with beam_size=1, ALSD or TSD with transducer_conf={"search_type": "alsd" / "tsd"} (inference/transducer.py);
        # transducer_conf is ignored for every other model, as in the reference
        self.beam_search_transducer = None
        if getattr(asr_model, "use_transducer_decoder", False):
            from .transducer import BeamSearchTransducer
            if lm is not None or ngram_file is not None or time_sync:
                raise ValueError("the transducer searches (greedy, ALSD, TSD) take no LM, n-gram file or time_sync")
            conf = dict(transducer_conf or {})
            conf.setdefault("nbest", nbest)
            self.beam_search_transducer = BeamSearchTransducer(asr_model.decoder, asr_model.joint_network, beam_size,
                                                               token_list=asr_model.token_list, **conf)
            self.beam_search = self.beam_search_transducer
            return
        # time_sync: espnet's BeamSearchTimeSync in place of the label-synchronous search (avsr_inference.py:257-275;
        # inference/timesync.py); results, nbest and timestamps as for the other search
        if time_sync:
            from .timesync import BeamSearchTimeSync
            self.beam_search = BeamSearchTimeSync(asr_model, lm, beam_size, ctc_weight, lm_weight, penalty, maxlenratio=maxlenratio,
                                                  minlenratio=minlenratio, ngram=ngram_file if ngram_weight != 0.0 else None)
            return
        # ngram_file: an ARPA text file (a KenLM binary is not read); its tables go to the model's device once, here
        ngram = None
        if ngram_file is not None and ngram_weight != 0.0:
            from ..lm.ngram import NgramLM
            ngram = NgramLM.from_arpa(ngram_file, asr_model.token_list, next(asr_model.parameters()).device)
        self.beam_search = BatchBeamSearch(asr_model, lm, beam_size, ctc_weight, lm_weight, penalty, maxlenratio, minlenratio,
                                           skip_zero_weight=skip_zero_weight, ngram=ngram, ngram_weight=ngram_weight,
                                           ngram_scorer=ngram_scorer)

    @torch.no_grad()
    def __call__(self, *batch):
        """batch: the tensors of ``asr_model.encode`` (speech, lengths) or (audio, lengths, video, lengths)."""
        enc, enc_lens = self.encode(*batch)
        return self._results(enc, enc_lens)

    def _results(self, enc, enc_lens):
        if isinstance(enc, tuple):
            enc = enc[0]
        results = []
        last = None if self.beam_search_transducer is not None else -1      # a transducer hypothesis has no <eos> (avsr_inference.py:497)
        for hyps in self.beam_search.decode(enc, enc_lens, nbest=self.nbest):
            res = []
            for ys, sc in hyps:
                token_int = [t for t in ys[1:last] if t != 0]
                token = [self.asr_model.token_list[t] for t in token_int]
                text = "".join(token).replace("<space>", " ")
                res.append((text, token, token_int, (ys, sc)))
            results.append(res)
        return self._with_timestamps(results, enc, enc_lens) if self.timestamps else results

    def _with_timestamps(self, results, enc, enc_lens):
        """align every hypothesis of every utterance in one launch (``rows``: hypothesis -> utterance), read the alignments back
        in one copy and append the timestamp record (None for a hypothesis CTC cannot emit) to every result tuple"""
        flat = [(u, r) for u, res in enumerate(results) for r in res]
        if not flat:
            return results
        N, Lmax = len(flat), max(len(r[2]) for _, r in flat)
        ys = torch.zeros((N, Lmax), dtype=torch.int64)
        for n, (_, r) in enumerate(flat):
            ys[n, : len(r[2])] = torch.tensor(r[2], dtype=torch.int64)
        dev = enc.device
        ys_lens = torch.tensor([len(r[2]) for _, r in flat], dtype=torch.int64).to(dev)
        rows = torch.tensor([u for u, _ in flat], dtype=torch.int32).to(dev)
        _, frame_lp, span, score = self.asr_model.ctc.forced_align(enc.contiguous().float(), enc_lens.to(dev), ys.to(dev), ys_lens,
                                                                   self.asr_model.blank_id, rows=rows)
        T = frame_lp.shape[1]
        packed = torch.cat([frame_lp, score.view(N, 1), span.view(N, 2 * Lmax).view(torch.float32)], dim=1).cpu()
        frame_lp, score = packed[:, :T].tolist(), packed[:, T].tolist()
        span = packed[:, T + 1:].contiguous().view(torch.int32).view(N, Lmax, 2).tolist()
        out = [[] for _ in results]
        for n, (u, r) in enumerate(flat):
            out[u].append(r + (timestamp_record(r[1], span[n], frame_lp[n], score[n], self.frame_seconds),))
        return out
