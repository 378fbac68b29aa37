"""Time-synchronous beam search on the MI355X: the reference's ``Speech2Text(time_sync=True)`` (src/inference/avsr_inference.py:94,
257-275), which swaps the label-synchronous ``BeamSearch`` for espnet's ``BeamSearchTimeSync`` - a CTC prefix beam search walked frame
by frame, every prefix that enters the beam rescored by the attention decoder and the LM with weights {ctc: ctc_weight, decoder:
1 - ctc_weight, lm: lm_weight, length_bonus: penalty}.

The reference is one Python loop over the frames of ONE utterance (batching raises NotImplementedError there), dictionaries keyed by
token tuples, every score read to the host, one un-batched decoder call per new prefix.  Here a batch of utterances, ragged lengths
included, advances together:

* one workgroup per utterance does a frame's bookkeeping (``tavsr_timesync_step``: candidates, expansion, the merge of equal prefixes,
  joint score, top-K); prefixes are nodes of a per-utterance trie in device memory, a prefix has one node for the whole utterance;
* between two frames the decoder and the LM score the slots that are NEW, all of them in one pass of fixed launch shape (U x beam rows)
  whatever their depths (``tavsr_tree_attn_rows``, ``tavsr_embed_pe_rows``): keys / values live in pools addressed by node;
* frame step + scorer pass are captured once per batch shape and replayed per frame from a device-side frame counter;
* without decoder and LM the whole frame loop is ONE launch (``tavsr_timesync_search``).

The host reads the lengths before the frame loop and the beams + tries after it; nothing in between.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .. import ops

GRAPH_STEP = True         # frame step + scorer pass as one hipGraph, captured once per batch shape; False: eager launches
ONE_LAUNCH = True         # no decoder and no LM: the whole frame loop in one launch; False: frame by frame with NULL scorer rows
SCORERS_PARALLEL = True   # the LM's chain on a side queue beside the decoder's (TAVSR_SINGLE_STREAM=1 disables every fork)


class ScorerRows:
    """what a frame leaves for the scorers, in device buffers a captured pass reads in place: per slot (row n = utterance * beam + slot)
    the last token ``tok`` int64 [N], its position ``pos`` = the prefix' depth int32 [N], the keys ``nkeys`` int32 [N] (depth + 1 for a
    slot that is new, 0 for every other: such a row needs no result) and the key / value pool rows of its ancestors ``anc`` int32
    [N, T + 1] (the own row last: utterance * (1 + beam * T) + node)."""

    def __init__(self, U, K, T, device):
        N = U * K
        self.tok = torch.zeros(N, dtype=torch.int64, device=device)
        self.pos = torch.zeros(N, dtype=torch.int32, device=device)
        self.nkeys = torch.zeros(N, dtype=torch.int32, device=device)
        self.anc = torch.zeros(N, T + 1, dtype=torch.int32, device=device)
        self.anc_tmp = torch.zeros(N, T + 1, dtype=torch.int32, device=device)
        self.max_keys = T + 1

    def operands(self):
        return (self.tok, self.pos, self.nkeys, self.anc)


class _Buffers:
    def __init__(self, U, T, V, K, C, device, with_dec, with_lm):
        self.words, self.off = ops.timesync_ws(K, V, T, C)
        self.ws = torch.zeros(U, self.words, dtype=torch.int32, device=device)
        self.lpz = torch.zeros(U, T, V, dtype=torch.float32, device=device)
        self.lens = torch.zeros(U, dtype=torch.int64, device=device)
        self.frame = torch.zeros(1, dtype=torch.int32, device=device)
        scored = with_dec or with_lm
        self.rows = ScorerRows(U, K, T, device) if scored else None
        self.dec = tuple(torch.zeros(U * K, V, dtype=torch.float32, device=device) for _ in range(2)) if with_dec else None
        self.lm = tuple(torch.zeros(U * K, V, dtype=torch.float32, device=device) for _ in range(2)) if with_lm else None
        self.graph = None


class TimeSyncSearch:
    """The search over given CTC log-probabilities.  ``dec_fn`` / ``lm_fn``: (ScorerRows, out) -> [U * beam, V] log-probabilities of the
    next token for (at least) the rows whose ``nkeys`` is not 0 - written to ``out`` and returned, or another tensor that is then
    copied - computed on the device without a host read (the calls are captured)."""

    def __init__(self, V: int, sos: int, beam_size: int, w_ctc: float, w_dec: float = 0.0, w_lm: float = 0.0, penalty: float = 0.0,
                 pre_beam_ratio: float = 1.5, dec_fn: Optional[Callable] = None, lm_fn: Optional[Callable] = None, blank: int = 0):
        self.V, self.sos, self.K, self.blank = V, sos, int(beam_size), blank
        self.C = int(pre_beam_ratio * beam_size)
        if self.C > V:
            raise ValueError(f"the pre-beam keeps int({pre_beam_ratio} * beam_size) = {self.C} tokens of a vocabulary of {V}: "
                             f"lower beam_size to {int(V / pre_beam_ratio)} or less, or pre_beam_ratio")
        if self.C < 1:
            raise ValueError(f"beam_size {beam_size} with pre_beam_ratio {pre_beam_ratio} keeps no candidate")
        self.w_ctc, self.w_dec, self.w_lm, self.pen = float(w_ctc), float(w_dec), float(w_lm), float(penalty)
        self.dec_fn = dec_fn if w_dec != 0.0 else None      # a term whose weight is 0 or whose module is absent is skipped
        self.lm_fn = lm_fn if w_lm != 0.0 else None
        self._bufs = None
        self._key = None
        self.replayed = False      # did the last search() re-use the previous one's captured frame?
        self.route = None          # "one_launch" / "graph" / "eager"
        self.on_new_shape = None   # hook: called with the buffers of a batch shape seen for the first time (scorers' own buffers)

    @property
    def scored(self):
        return self.dec_fn is not None or self.lm_fn is not None

    def check_frames(self, T):
        """with decoder or LM a prefix may grow by one token per frame and attends to all of itself: more frames than the scorers'
        attention takes keys are refused here, before any launch"""
        if self.scored and T + 1 > ops.TREE_ROWS_MAX_KEYS:
            raise ValueError(f"time-synchronous search with decoder or LM: {T} frames allow prefixes of {T + 1} keys, the scorers' "
                             f"attention (tavsr_tree_attn_rows) takes {ops.TREE_ROWS_MAX_KEYS}: cut the input to at most "
                             f"{ops.TREE_ROWS_MAX_KEYS - 1} encoder frames (about 40 s at 25 frames per second), or search with the CTC "
                             "term alone (ctc_weight 1.0, no LM)")

    def _frame(self, b):
        """one frame: the step, the counter, the scorers' rows of the slots that are new"""
        ops.timesync_step(b.lpz, b.lens, b.ws, b.frame, self.K, self.C, self.sos, self.w_ctc, self.w_dec, self.w_lm, self.pen,
                          dec=b.dec, lm=b.lm, scorer=None if b.rows is None else b.rows.operands(),
                          anc_tmp=None if b.rows is None else b.rows.anc_tmp, blank=self.blank)
        b.frame.add_(1)
        self._score(b)

    def _score(self, b):
        """the scorers' rows of the slots that are new, into the buffers the next frame takes them from; the LM's chain of small
        launches runs beside the decoder's (two independent chains, as in the label-synchronous step)"""
        def run(fn, out):
            r = fn(b.rows, out)
            if r is not out:
                out.copy_(r)

        if self.lm_fn is not None:
            with ops.BranchScope(enabled=SCORERS_PARALLEL and self.dec_fn is not None) as br:
                run(self.lm_fn, b.lm[0])
        if self.dec_fn is not None:
            run(self.dec_fn, b.dec[0])
        if self.lm_fn is not None:
            br.join()

    def _init(self, b):
        U, T, V = b.lpz.shape
        ops.timesync_init(b.ws, U, self.K, V, T, self.C, self.sos, self.blank, scorer=None if b.rows is None else b.rows.operands(),
                          frame_dev=b.frame)

    @torch.no_grad()
    def search(self, lpz: torch.Tensor, lens: torch.Tensor, nbest: Optional[int] = None, fill=None):
        """lpz [U, T, V] fp32 log-softmax of the CTC head, lens [U] -> per utterance [(tokens incl. the two <sos>, score), ...] best
        first.  ``fill`` (optional): called with the search's buffers before the frame loop (the scorers' per-batch operands)."""
        U, T, V = lpz.shape
        assert V == self.V
        self.check_frames(T)
        dev = lpz.device
        lens_host = [int(v) for v in lens.cpu()]                       # the one host read in front of the frame loop
        frames = min(T, max(lens_host)) if lens_host else 0
        key = (U, T, V, str(dev))
        self.replayed = self._bufs is not None and self._key == key
        if not self.replayed:
            self._bufs = _Buffers(U, T, V, self.K, self.C, dev, self.dec_fn is not None, self.lm_fn is not None)
            self._key = key
            if self.on_new_shape is not None:
                self.on_new_shape(self._bufs)
        b = self._bufs
        b.lpz.copy_(lpz)
        b.lens.copy_(lens.to(dev).to(torch.int64))
        if fill is not None:
            fill(b)
        self._init(b)
        if not self.scored and ONE_LAUNCH:
            self.route = "one_launch"
            ops.timesync_search(b.lpz, b.lens, b.ws, self.K, self.C, self.sos, self.w_ctc, self.pen, blank=self.blank)
        else:
            self._score(b)                                              # (<sos>,) is scored once, before frame 0
            if GRAPH_STEP:
                self.route = "graph"
                if b.graph is None:
                    self._capture(b)
                for _ in range(frames):
                    b.graph.replay()
            else:
                self.route = "eager"
                for _ in range(frames):
                    self._frame(b)
        return self._read(b, nbest)

    def _capture(self, b):
        """warm-up on a side queue (lazy allocations happen outside the capture), the state put back, then the capture"""
        saved = (b.ws.clone(), b.frame.clone()) + (() if b.rows is None else tuple(t.clone() for t in b.rows.operands()))
        saved_rows = tuple(t.clone() for pair in (b.dec, b.lm) if pair is not None for t in pair)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._frame(b)
        torch.cuda.current_stream().wait_stream(side)
        live = (b.ws, b.frame) + (() if b.rows is None else b.rows.operands())
        for dst, src in zip(live, saved):
            dst.copy_(src)
        for dst, src in zip([t for pair in (b.dec, b.lm) if pair is not None for t in pair], saved_rows):
            dst.copy_(src)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._frame(b)
        b.graph = graph

    def _read(self, b, nbest):
        """the one host read behind the frame loop: beams, scores and tries of every utterance"""
        o = b.off
        NN = o["nodes"]
        host = b.ws[:, : o["token"] + NN].cpu()
        K = self.K
        head = host[:, : o["misc"] + 8]
        order = head[:, o["order"]: o["order"] + K].tolist()
        nodes = head[:, o["node"]: o["node"] + K].tolist()
        scores = head[:, o["score"]: o["score"] + K].view(torch.float32).tolist()
        over = torch.nonzero(head[:, o["misc"] + 2]).flatten().tolist()
        parent, token = host[:, o["parent"]: o["parent"] + NN].numpy(), host[:, o["token"]: o["token"] + NN].numpy()
        out = []
        for u in range(host.shape[0]):
            par, tk, hyps = parent[u], token[u], []
            for r in range(K if nbest is None else min(K, nbest)):
                slot = order[u][r]
                if slot < 0:
                    continue
                node, toks = nodes[u][slot], []
                while node >= 0:
                    toks.append(int(tk[node]))
                    node = int(par[node])
                hyps.append((toks[::-1] + [self.sos], scores[u][slot]))
            out.append(hyps)
        if over:
            raise RuntimeError(f"time-synchronous search: in utterances {over} more than {o['cand_cap']} tokens of one frame tie at the "
                               f"pre-beam's threshold (pre-beam {self.C}): the candidate list holds min(V, 2 * pre-beam) tokens and none "
                               "is dropped silently.  Such a frame is degenerate (equal log-probabilities); raise beam_size or check the "
                               "CTC head's outputs")
        return out


class BeamSearchTimeSync:
    """espnet ``BeamSearchTimeSync`` for a built model: ``decode(enc, enc_lens)`` has the return shape of ``BatchBeamSearch.decode`` and
    takes a batch of utterances.  ``maxlenratio`` / ``minlenratio`` are accepted and unused, as in the reference's class."""

    def __init__(self, model, lm=None, beam_size: int = 10, ctc_weight: float = 0.5, lm_weight: float = 1.0, penalty: float = 0.0,
                 pre_beam_ratio: float = 1.5, maxlenratio: float = 0.0, minlenratio: float = 0.0, ngram=None):
        from .beam_search import _DecoderStep, _LMStep
        if ngram is not None:
            raise ValueError("an n-gram LM together with time_sync: the reference's BeamSearchTimeSync is handed the scorer and never "
                             "reads it - its results are those without n-gram.  Drop ngram_file, or search label-synchronously "
                             "(time_sync=False), where the n-gram is a scorer")
        if model.ctc is None:
            raise ValueError("the time-synchronous search walks the CTC posteriors frame by frame: this model was built without a CTC "
                             "head (model_conf ctc_weight: 0.0).  Search it label-synchronously (time_sync=False)")
        if not (0.0 <= ctc_weight <= 1.0):
            raise ValueError(f"ctc_weight must lie in [0, 1]: {ctc_weight}")
        self.model, self.lm = model, lm
        self.V = len(model.token_list)
        self.K = int(beam_size)
        self.sos = model.sos
        self.has_dec = model.decoder is not None and 1.0 - ctc_weight != 0.0
        self.has_lm = lm is not None and lm_weight != 0.0
        self.dec_step = _DecoderStep(model.decoder) if self.has_dec else None
        self.lm_step = _LMStep(lm) if self.has_lm else None
        self.search = TimeSyncSearch(self.V, self.sos, beam_size, ctc_weight, 1.0 - ctc_weight if self.has_dec else 0.0,
                                     lm_weight if self.has_lm else 0.0, penalty, pre_beam_ratio,
                                     dec_fn=self._dec_rows if self.has_dec else None, lm_fn=self._lm_rows if self.has_lm else None,
                                     blank=getattr(model, "blank_id", 0))
        self.search.on_new_shape = self._new_shape
        self._enc = None

    @property
    def route(self):
        return self.search.route

    def _dec_rows(self, rows, out):
        return self.dec_step.step(0, rows.tok, rows.anc, rows=(rows.nkeys, rows.pos, rows.max_keys), out=out)

    def _lm_rows(self, rows, out):
        return self.lm_step.step(0, rows.tok, rows.anc, rows=(rows.nkeys, rows.pos, rows.max_keys), out=out)

    def _new_shape(self, b):
        """the scorers' buffers of a batch shape: key / value pools with one row per trie node (U (1 + beam T) <= (T + 1) U beam rows),
        the decoder's source-attention keys / values (filled per batch by ``_fill``)"""
        enc, U, T = self._enc, b.lpz.shape[0], b.lpz.shape[1]
        if self.has_dec:
            self.dec_step.start(enc, b.lens, U * self.K, self.K, T + 1)      # (b.lens: the buffer every batch's lengths are copied to)
        if self.has_lm:
            self.lm_step.start(enc, U * self.K, T + 1, self.K)

    def _fill(self, b):
        if self.has_dec:
            self.dec_step.refill(self._enc)

    @torch.no_grad()
    def decode(self, enc: torch.Tensor, enc_lens: torch.Tensor, nbest: Optional[int] = None):
        """enc [U, T, D] encoder outputs, enc_lens [U] -> per utterance [(yseq list incl. the two <sos>, score), ...] best first"""
        U, T, D = enc.shape
        self.search.check_frames(T)
        enc = enc.contiguous().float()
        if self.has_dec:
            self.dec_step.weights.sync()
        if self.has_lm:
            self.lm_step.sync_weights()
        ctc = self.model.ctc
        z = ops.linear(enc.reshape(U * T, D), ctc.ctc_lo.weight, ctc.ctc_lo.bias)
        lpz = ops.log_softmax_rows(z).view(U, T, self.V)
        self._enc = enc
        try:
            return self.search.search(lpz, enc_lens, nbest, fill=self._fill)
        finally:
            self._enc = None
