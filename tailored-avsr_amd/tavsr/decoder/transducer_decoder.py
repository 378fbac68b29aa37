"""``TransducerDecoder`` - counterpart of espnet2.asr.decoder.transducer_decoder.TransducerDecoder, the prediction network of
a transducer model (registered as ``decoder: transducer``, src/tasks/avsr.py:191, 658-663): an embedding with a padding row, a
dropout, and ``num_layers`` one-layer LSTMs with a dropout behind each.  Same constructor arguments, members and ``state_dict``
keys (``embed.weight``, ``decoder.{l}.weight_ih_l0`` ...: the keys of ``torch.nn.Embedding`` and ``torch.nn.LSTM``).

``forward`` is one autograd node (``functional_rnnt.TransducerDecoderFn``); the search's one-token steps (``score``,
``batch_score``, ``step``) run ``tavsr_lstm_step`` per layer.  ``rnn_type: gru`` is refused."""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

from .. import functional as F_
from .. import ops
from ..functional_rnnt import LSTM_LAYER_PARAM_NAMES, TransducerDecoderFn


class _LSTMLayer(torch.nn.Module):
    """the parameters of ``torch.nn.LSTM(input_size, hidden_size, 1, batch_first=True)`` under its names, with its initialisation"""

    def __init__(self, input_size: int, hidden_size: int):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.weight_ih_l0 = torch.nn.Parameter(torch.empty(4 * hidden_size, input_size))
        self.weight_hh_l0 = torch.nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
        self.bias_ih_l0 = torch.nn.Parameter(torch.empty(4 * hidden_size))
        self.bias_hh_l0 = torch.nn.Parameter(torch.empty(4 * hidden_size))
        k = 1.0 / math.sqrt(hidden_size)
        for p in self.parameters():
            torch.nn.init.uniform_(p, -k, k)


class TransducerDecoder(torch.nn.Module):
    def __init__(self, vocab_size: int, rnn_type: str = "lstm", num_layers: int = 1, hidden_size: int = 320, dropout: float = 0.0,
                 dropout_embed: float = 0.0, embed_pad: int = 0):
        super().__init__()
        if rnn_type not in ("lstm", "gru"):
            raise ValueError(f"Not supported: rnn_type={rnn_type}")
        if rnn_type == "gru":
            raise ValueError("rnn_type: gru is not on the HIP path: the transducer's prediction network is an LSTM here (rnn_type: lstm)")
        self.embed = torch.nn.Embedding(vocab_size, hidden_size, padding_idx=embed_pad)
        self.decoder = torch.nn.ModuleList([_LSTMLayer(hidden_size, hidden_size) for _ in range(num_layers)])
        self._rates = (float(dropout), float(dropout_embed))
        self.dlayers, self.dunits, self.dtype, self.odim = num_layers, hidden_size, rnn_type, vocab_size
        self.ignore_id, self.blank_id = -1, embed_pad
        self.device = next(self.parameters()).device

    def set_device(self, device: torch.device):
        self.device = device

    def _params(self):
        cached = self.__dict__.get("_tavsr_pcache")
        if cached is None:
            cached = self.__dict__["_tavsr_pcache"] = [self.embed.weight] + [getattr(layer, n) for layer in self.decoder
                                                                              for n in LSTM_LAYER_PARAM_NAMES]
        return cached

    def init_state(self, batch_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.embed.weight.device
        return (torch.zeros(self.dlayers, batch_size, self.dunits, device=dev), torch.zeros(self.dlayers, batch_size, self.dunits, device=dev))

    def forward(self, labels: torch.Tensor) -> torch.Tensor:
        """labels (B, U+1) int64, blank first -> dec_out (B, U+1, dunits); the states start at zero, the full length is run"""
        cfg = dict(layers=self.dlayers, pad=self.embed.padding_idx)
        if self.training:
            cfg.update(p=self._rates[0], p_embed=self._rates[1])
        return F_.grad_apply(TransducerDecoderFn, labels.to(torch.int64), cfg, *self._params())

    # ---------------------------------------------------------------- the search's one-token steps (eval mode: no dropout)
    def step_weights(self) -> List[torch.Tensor]:
        """the transposed recurrent weights ``tavsr_lstm_step`` streams, one per layer: built once per search"""
        return [ops.lstm_wt(layer.weight_hh_l0) for layer in self.decoder]

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, state: Tuple[torch.Tensor, torch.Tensor], commit: Optional[torch.Tensor] = None,
             wts: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """tokens (N) int64, state (h, c) each (dlayers, N, dunits), updated IN PLACE for the rows ``commit`` (uint8 (N); None: all)
        lets through -> dec_out (N, dunits), the last layer's h (a view of the state).  Launches only: capturable."""
        wts = self.step_weights() if wts is None else wts
        x = self.embed.weight[tokens]                               # embedding row gather (index plumbing)
        h, c = state
        for li, layer in enumerate(self.decoder):
            xg = ops.linear(x, layer.weight_ih_l0)
            ops.lstm_step(xg, wts[li], layer.bias_ih_l0, layer.bias_hh_l0, h[li], c[li], commit)
            x = h[li]
        return x

    def score(self, hyp, cache: Dict[str, Any]):
        """espnet's one-hypothesis step: -> (dec_out (dunits), (h, c) each (dlayers, 1, dunits), label (1))"""
        label = torch.full((1,), hyp.yseq[-1], dtype=torch.long, device=self.embed.weight.device)
        key = "_".join(map(str, hyp.yseq))
        if key in cache:
            dec_out, dec_state = cache[key]
        else:
            dec_state = (hyp.dec_state[0].clone(), hyp.dec_state[1].clone())
            dec_out = self.step(label, dec_state).clone()
            cache[key] = (dec_out, dec_state)
        return dec_out[0], dec_state, label

    def batch_score(self, hyps, dec_states=None, cache: Optional[Dict[str, Any]] = None, use_lm: bool = False):
        """espnet's batched step over a list of hypotheses: -> (dec_out (N, dunits), (h, c) each (dlayers, N, dunits), labels (N))"""
        dev = self.embed.weight.device
        labels = torch.tensor([h.yseq[-1] for h in hyps], dtype=torch.long, device=dev)
        state = (torch.cat([h.dec_state[0] for h in hyps], dim=1).contiguous(), torch.cat([h.dec_state[1] for h in hyps], dim=1).contiguous())
        dec_out = self.step(labels, state).clone()
        return dec_out, state, labels

    def select_state(self, states: Tuple[torch.Tensor, torch.Tensor], idx: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return (states[0][:, idx: idx + 1, :], states[1][:, idx: idx + 1, :])

    def create_batch_states(self, states, new_states, check_list=None):
        return (torch.cat([s[0] for s in new_states], dim=1), torch.cat([s[1] for s in new_states], dim=1))
