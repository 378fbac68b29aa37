"""Greedy transducer search on the MI355X - espnet2 asr/transducer/beam_search_transducer.py BeamSearchTransducer with
``beam_size <= 1`` (its ``greedy_search``; built by src/inference/avsr_inference.py:181-207), for a whole ragged batch at once.

Per encoder frame: the joint row of every utterance, a log-softmax and an argmax; where the argmax is not blank it is appended,
its log-probability added to the score and ONE prediction-network step committed (``tavsr_lstm_step`` with a commit mask) - at
most one symbol per frame, as espnet's loop does.  A frame is one replayed graph of launches: the frame counter, the tokens,
the commit mask, the states, the hypotheses and the scores live in device buffers updated in place.  The host reads the
lengths before the loop and the hypotheses after it.

The default, ALSD, NSC and mAES beam searches and LM fusion are not on the HIP path: ``beam_size > 1`` raises."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import torch

from .. import ops


@dataclass
class Hypothesis:
    """espnet2.asr.transducer.beam_search_transducer.Hypothesis"""
    score: float
    yseq: List[int]
    dec_state: Any = None
    lm_state: Any = None


class BeamSearchTransducer:
    def __init__(self, decoder, joint_network, beam_size: int, lm=None, lm_weight: float = 0.1, search_type: str = "default",
                 max_sym_exp: int = 2, u_max: int = 50, nstep: int = 1, prefix_alpha: int = 1, expansion_gamma: float = 2.3,
                 expansion_beta: int = 2, score_norm: bool = True, nbest: int = 1, token_list: Optional[List[str]] = None,
                 use_graph: bool = True):
        if beam_size > 1:
            raise ValueError(f"the transducer search on the HIP path is the greedy search: set beam_size=1 (got beam_size={beam_size}; "
                             "the default, ALSD, NSC and mAES beam searches are not built)")
        if lm is not None:
            raise ValueError("LM fusion is not part of the greedy transducer search (lm must be None)")
        self.decoder, self.joint_network = decoder, joint_network
        self.beam_size, self.nbest = beam_size, nbest
        self.blank_id = decoder.blank_id
        self.vocab_size = decoder.odim
        self.use_graph = use_graph
        self.search_algorithm = self.greedy_search

    # ---------------------------------------------------------------- espnet's interface: one utterance
    @torch.no_grad()
    def __call__(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, D) -> [Hypothesis]"""
        return self.greedy_search(enc_out)

    def greedy_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        lens = torch.full((1,), enc_out.shape[0], dtype=torch.int64, device=enc_out.device)
        (ys, score), = self.decode(enc_out[None], lens)[0]
        return [Hypothesis(score=score, yseq=ys)]

    # ---------------------------------------------------------------- the batch
    @torch.no_grad()
    def decode(self, enc: torch.Tensor, enc_lens: torch.Tensor, nbest: Optional[int] = None):
        """enc (B, T, D), enc_lens (B) -> per utterance [(token ids with the leading blank, score)] (one hypothesis)"""
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
