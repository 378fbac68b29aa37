"""Transducer searches on the MI355X - espnet2 asr/transducer/beam_search_transducer.py BeamSearchTransducer (built by
src/inference/avsr_inference.py:181-207 as ``BeamSearchTransducer(beam_size=beam_size, **transducer_conf)``), for a whole ragged
batch at once.  Blank is id 0.

* ``beam_size <= 1``: its ``greedy_search``.  Per encoder frame the joint row of every utterance, a log-softmax and an argmax;
  where the argmax is not blank it is appended, its log-probability added to the score and ONE prediction-network step committed
  (``tavsr_lstm_step`` with a commit mask) - at most one symbol per frame, as espnet's loop does.
* ``search_type="alsd"``: ``align_length_sync_decoding``.  ``T + min(u_max, T - 1)`` steps; a step extends every hypothesis of the
  beam whose frame ``i - labels`` is still inside the utterance by blank and by its ``beam`` best labels, keeps the ``beam`` best,
  merges equal prefixes with ``logaddexp``, and collects the blank extensions at the last frame as the results.
* ``search_type="tsd"``: ``time_sync_decoding``.  Per frame ``max_sym_exp`` expansions; every expansion adds the blank extensions
  to the frame's list A (merging equal prefixes) and, but for the last, replaces the working set by its ``beam`` best label
  extensions; the beam of the next frame is the ``beam`` best of A.

The beam searches keep ``K = beam`` rows per utterance.  One step (one ``i`` of ALSD, one frame of TSD) is a fixed chain of
launches (csrc/rnnt_search.hip): ``lin_dec`` of the rows' states, the joint row at each row's own frame, ``lin_out``, one reduce
per row (log-softmax, blank, the K best labels), the per-utterance bookkeeping (one workgroup per utterance; prefixes are nodes
of a trie, so equal prefixes are found exactly), the gather of the states by parent row and one LSTM step for the rows that took
a label.  The step is captured once per shape and replayed; the counters, beams, tries and states live in device buffers.  The host
reads the lengths before the loop and the beams, ``final`` and the tries after it.

The default (``beam_size > 1``), NSC and mAES searches and LM fusion are not on the HIP path."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import torch

from .. import _lib as L
from .. import ops

BUILT_BEAM_SEARCHES = ("alsd", "tsd")


@dataclass
class Hypothesis:
    """espnet2.asr.transducer.beam_search_transducer.Hypothesis"""
    score: float
    yseq: List[int]
    dec_state: Any = None
    lm_state: Any = None


def sort_nbest(hyps, score_norm: bool, nbest: int):
    """espnet's sort_nbest on [(yseq, score)]: descending by score / len(yseq) or by score, stable; scores stay un-normalised"""
    return sorted(hyps, key=lambda h: h[1] / len(h[0]) if score_norm else h[1], reverse=True)[:nbest]


class BeamSearchTransducer:
    def __init__(self, decoder, joint_network, beam_size: int, lm=None, lm_weight: float = 0.1, search_type: str = "default",
                 max_sym_exp: int = 2, u_max: int = 50, nstep: int = 1, prefix_alpha: int = 1, expansion_gamma: float = 2.3,
                 expansion_beta: int = 2, score_norm: bool = True, nbest: int = 1, token_list: Optional[List[str]] = None,
                 use_graph: bool = True):
        if search_type not in ("default", "alsd", "tsd", "nsc", "maes"):
            raise ValueError(f"unknown transducer search_type: {search_type!r}")
        if beam_size > 1 and search_type not in BUILT_BEAM_SEARCHES:
            raise ValueError(f"the transducer beam searches on the HIP path are search_type='alsd' and 'tsd': search_type={search_type!r} "
                             f"runs as the greedy search only, set beam_size=1 (got beam_size={beam_size}; the default, NSC and mAES "
                             "beam searches are not built)")
        if lm is not None:
            raise ValueError("LM fusion is not part of the transducer searches on the HIP path (lm must be None)")
        if u_max < 0 or max_sym_exp < 1:
            raise ValueError(f"u_max must be >= 0 and max_sym_exp >= 1 (got u_max={u_max}, max_sym_exp={max_sym_exp})")
        self.decoder, self.joint_network = decoder, joint_network
        self.beam_size, self.nbest = beam_size, nbest
        self.blank_id = decoder.blank_id
        self.vocab_size = decoder.odim
        self.use_graph = use_graph
        self.search_type = search_type
        self.u_max, self.max_sym_exp, self.score_norm = int(u_max), int(max_sym_exp), bool(score_norm)
        self._cap = None                                        # the buffers and the captured step of the last shape searched
        if beam_size <= 1:
            self.search_algorithm = self.greedy_search
        elif search_type == "alsd":
            self.search_algorithm = self.align_length_sync_decoding
        else:
            self.search_algorithm = self.time_sync_decoding

    # ---------------------------------------------------------------- espnet's interface: one utterance
    @torch.no_grad()
    def __call__(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, D) -> [Hypothesis]"""
        return self.search_algorithm(enc_out)

    def _one(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        lens = torch.full((1,), enc_out.shape[0], dtype=torch.int64, device=enc_out.device)
        return [Hypothesis(score=score, yseq=ys) for ys, score in self.decode(enc_out[None], lens)[0]]

    def greedy_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        return self._one(enc_out)

    def align_length_sync_decoding(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        if self.beam_size <= 1 or self.search_type != "alsd":
            raise ValueError("align_length_sync_decoding needs search_type='alsd' and beam_size > 1")
        return self._one(enc_out)

    def time_sync_decoding(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        if self.beam_size <= 1 or self.search_type != "tsd":
            raise ValueError("time_sync_decoding needs search_type='tsd' and beam_size > 1")
        return self._one(enc_out)

    # ---------------------------------------------------------------- the batch
    @torch.no_grad()
    def decode(self, enc: torch.Tensor, enc_lens: torch.Tensor, nbest: Optional[int] = None):
        """enc (B, T, D), enc_lens (B) -> per utterance [(token ids with the leading blank, score)], at most ``nbest`` (None: the
        constructor's), best first"""
        if self.beam_size > 1:
            return self.beam_search_batch(enc, enc_lens, self.nbest if nbest is None else nbest)
        hyp, hyp_len, score = self.greedy_search_batch(enc, enc_lens)
        hyp, hyp_len, score = hyp.tolist(), hyp_len.tolist(), score.tolist()
        return [[([self.blank_id] + hyp[b][: hyp_len[b]], score[b])] for b in range(len(hyp_len))]

    def greedy_search_batch(self, enc: torch.Tensor, enc_lens: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (hyp (B, T) int64, hyp_len (B) int32, score (B) fp32) on the host"""
        dec, jn = self.decoder, self.joint_network
        B, T, D = enc.shape
        dev = enc.device
        t_len = enc_lens.to(device=dev, dtype=torch.int64).contiguous()
        frames = min(T, int(enc_lens.max())) if B else 0        # the one host read in front of the loop
        e = ops.linear(enc.reshape(B * T, D).contiguous().float(), jn.lin_enc.weight, jn.lin_enc.bias).view(B, T, -1)
        wts = dec.step_weights()
        state = dec.init_state(B)
        tok = torch.full((B,), self.blank_id, dtype=torch.int64, device=dev)
        commit = torch.zeros((B,), dtype=torch.uint8, device=dev)
        frame = torch.zeros((1,), dtype=torch.int32, device=dev)
        hyp = torch.zeros((B, max(T, 1)), dtype=torch.int64, device=dev)
        hyp_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        score = torch.zeros((B,), dtype=torch.float32, device=dev)
        bufs = (state[0], state[1], tok, commit, frame, hyp, hyp_len, score)

        def one_frame():
            d = ops.linear(state[0][-1], jn.lin_dec.weight)
            z = ops.rnnt_frame_z(e, d, frame)
            logits = ops.linear(z, jn.lin_out.weight, jn.lin_out.bias)
            ops.rnnt_greedy_pick(logits, t_len, self.blank_id, frame, tok, commit, hyp, hyp_len, score)
            dec.step(tok, state, commit, wts)

        dec.step(tok, state, None, wts)                         # espnet: the first decoder step takes the blank from a zero state
        if frames > 0 and self.use_graph:
            keep = [t.clone() for t in bufs]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                one_frame()                                     # warm-up outside the capture; the buffers are put back below
            torch.cuda.current_stream().wait_stream(side)
            for t, k in zip(bufs, keep):
                t.copy_(k)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                one_frame()                                     # (a capture runs nothing: the buffers still hold the start state)
            for _ in range(frames):
                graph.replay()
        else:
            for _ in range(frames):
                one_frame()
        return hyp.cpu(), hyp_len.cpu(), score.cpu()

    # ---------------------------------------------------------------- ALSD and TSD
    def _buffers(self, U: int, T: int, D: int, dev) -> dict:
        """every device buffer of a search of this shape (and, once captured, its step graph): kept until another shape comes"""
        dec, jn = self.decoder, self.joint_network
        kind, K, V, M = self.search_type, min(self.beam_size, self.vocab_size), self.vocab_size, self.max_sym_exp
        key = (kind, U, T, D, K, self.u_max, M, str(dev), L.param_ptrs(list(dec.parameters()) + list(jn.parameters())))
        if self._cap is not None and self._cap["key"] == key:
            return self._cap
        words, off = ops.rnnt_search_ws(kind, K, V, T, self.u_max, M)      # ValueError before any launch where the shape is not taken
        N, J, H, nl = U * K, jn.lin_out.weight.shape[1], dec.dunits, dec.dlayers
        f = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        b = dict(key=key, graph=None, words=words, off=off, U=U, T=T, K=K, N=N,
                 e=ops.empty(U, T, J, like=jn.lin_out.weight), t_len=torch.zeros(U, dtype=torch.int64, device=dev),
                 ws=torch.empty((U, words), **i32), row_t=torch.empty(N, **i32), parent=torch.empty(N, **i32),
                 tok=torch.empty(N, dtype=torch.int64, device=dev), commit=torch.empty(N, dtype=torch.uint8, device=dev),
                 state=(torch.empty((nl, N, H), **f), torch.empty((nl, N, H), **f)),
                 moved=(torch.empty((nl, N, H), **f), torch.empty((nl, N, H), **f)),
                 d=torch.empty((N, J), **f), z=torch.empty((N, J), **f),
                 reduce=(torch.empty(N, **f), torch.empty((N, K), **f), torch.empty((N, K), **i32)),
                 wts=[torch.empty((H, 4 * H), **f) for _ in range(nl)])
        if kind == "tsd":
            b.update(a_src=torch.empty(N * M, **i32), b_sel=torch.empty(N, **i32),
                     a_state=(torch.empty((nl, N * M, H), **f), torch.empty((nl, N * M, H), **f)))
        self._cap = b
        return b

    def _reset(self, b: dict, enc: torch.Tensor, enc_lens: torch.Tensor) -> None:
        """the state before the first step, written into the kept buffers (launches and device copies only)"""
        dec, jn = self.decoder, self.joint_network
        U, T, D = enc.shape
        b["t_len"].copy_(enc_lens.to(device=enc.device, dtype=torch.int64))
        b["e"].copy_(ops.linear(enc.reshape(U * T, D).contiguous().float(), jn.lin_enc.weight, jn.lin_enc.bias).view(U, T, -1))
        for w, layer in zip(b["wts"], dec.decoder):
            w.copy_(ops.lstm_wt(layer.weight_hh_l0))
        ops.rnnt_search_init(self.search_type, b["ws"], b["t_len"], b["row_t"], b["K"], self.vocab_size, T, self.u_max, self.max_sym_exp)
        b["state"][0].zero_()
        b["state"][1].zero_()
        b["tok"].fill_(self.blank_id)
        dec.step(b["tok"], b["state"], None, b["wts"])          # every row starts as (blank,): the first step from the zero state

    def _joint_rows(self, b: dict) -> None:
        jn = self.joint_network
        ops.linear(b["state"][0][-1], jn.lin_dec.weight, out=b["d"], ldc=b["d"].shape[1])
        ops.rnnt_search_z(b["e"], b["d"], b["row_t"], b["K"], out=b["z"])
        logits = ops.linear(b["z"], jn.lin_out.weight, jn.lin_out.bias)
        ops.rnnt_row_topk(logits, b["K"], b["row_t"], out=b["reduce"])

    def _extend(self, b: dict) -> None:
        """the new rows take their parents' states; the rows that took a label run one prediction-network step"""
        dec = self.decoder
        ops.rnnt_gather_state(b["state"], b["parent"], b["moved"])
        x = dec.embed.weight[b["tok"]]
        for li, layer in enumerate(dec.decoder):
            xg = ops.linear(x, layer.weight_ih_l0)
            ops.lstm_step(xg, b["wts"][li], layer.bias_ih_l0, layer.bias_hh_l0, b["moved"][0][li], b["moved"][1][li], b["commit"],
                          h_out=b["state"][0][li], c_out=b["state"][1][li])
            x = b["state"][0][li]

    def _step(self, b: dict) -> None:
        V, T = self.vocab_size, b["T"]
        if self.search_type == "alsd":
            self._joint_rows(b)
            ops.rnnt_alsd_step(b["ws"], b["t_len"], *b["reduce"], b["row_t"], b["parent"], b["tok"], b["commit"], V, T, self.u_max)
            self._extend(b)
            return
        M = self.max_sym_exp
        for v in range(M):
            self._joint_rows(b)
            ops.rnnt_tsd_step(b["ws"], b["t_len"], *b["reduce"], b["row_t"], b["parent"], b["tok"], b["commit"], b["a_src"], b["b_sel"],
                              v, V, T, M)
            ops.rnnt_gather_state(b["state"], b["a_src"], b["a_state"])      # an entry of A keeps the state of the row that made it
            if v < M - 1:
                self._extend(b)
            else:
                ops.rnnt_gather_state(b["a_state"], b["b_sel"], b["state"])

    def beam_search_batch(self, enc: torch.Tensor, enc_lens: torch.Tensor, nbest: int):
        U, T, D = enc.shape
        if U == 0:
            return []
        lens = [min(T, max(0, int(t))) for t in enc_lens.tolist()]           # the one host read in front of the loop
        if T == 0 or max(lens) == 0:
            return [[([self.blank_id], 0.0)] for _ in lens]
        if self.search_type == "alsd":
            steps = max(t + min(self.u_max, t - 1) if t > 0 else 0 for t in lens)
        else:
            steps = max(lens)
        b = self._buffers(U, T, D, enc.device)
        self._reset(b, enc, enc_lens)
        if self.use_graph:
            if b["graph"] is None:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._step(b)                               # warm-up outside the capture; the start state is written again below
                torch.cuda.current_stream().wait_stream(side)
                self._reset(b, enc, enc_lens)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._step(b)                               # (a capture runs nothing: the buffers still hold the start state)
                b["graph"] = graph
            for _ in range(steps):
                b["graph"].replay()
        else:
            for _ in range(steps):
                self._step(b)
        return self._results(b["ws"].cpu(), b["off"], b["K"], nbest)

    def _results(self, ws: torch.Tensor, off: dict, K: int, nbest: int):
        """the one host read behind the loop: per utterance the beam, the list and the trie -> [(yseq, score)] best first"""
        out = []
        fl = ws.view(torch.float32)
        for u in range(ws.shape[0]):
            blk, fblk = ws[u].tolist(), fl[u]
            if blk[4]:
                raise L.TavsrError("transducer beam search: a table of the search overflowed its bound (include/tavsr.h)")
            n_slots, n_list = blk[1], blk[3]
            par, tk = off["parent"], off["token"]

            def yseq(node):
                ys = []
                while node > 0:
                    ys.append(blk[tk + node])
                    node = blk[par + node]
                return [self.blank_id] + ys[::-1]

            if self.search_type == "alsd" and n_list > 0:       # final
                nodes = blk[off["list_node"]: off["list_node"] + n_list]
                scores = fblk[off["list_score"]: off["list_score"] + n_list].tolist()
                out.append(sort_nbest([(yseq(n), s) for n, s in zip(nodes, scores)], self.score_norm, nbest))
                continue
            nodes = blk[off["node"]: off["node"] + n_slots]
            scores = fblk[off["score"]: off["score"] + n_slots].tolist()
            hyps = [(yseq(n), s) for n, s in zip(nodes, scores)]
            out.append(hyps[:nbest] if self.search_type == "alsd" else sort_nbest(hyps, self.score_norm, nbest))
        return out
