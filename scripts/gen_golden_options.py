"""Golden vectors for the encoder options beyond the shipped recipes, from the REFERENCE's own modules.

Imports the reference's Python over ``oracle._shim`` exactly as ``oracle/gen_golden.py`` does (same leaf stand-ins, same
seeded parameter fill and inputs), and writes ``tests/golden/bf_layer_ffn_{tanh,hardtanh,selu}.npz``: one
MyBranchformerEncoderLayer.forward (encoder_layer.py:153-321, learned-average merge, ragged lengths) per member of espnet
get_activation's set that the recipes do not use, as ``ffn_activation_type`` (encoder.py:206).  Same contents as
``bf_layer_learned.npz`` plus the fraction of feed-forward pre-activations on each side of the activation's kinks.
Re-running reproduces the files bit for bit (fixed seeds, one thread).

    python scripts/gen_golden_options.py          # needs the reference checkout the shim points at
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _shim  # noqa: E402
from oracle.gen_golden import _np, _save  # noqa: E402
from oracle.model import compact, fill_parameters_, synth  # noqa: E402

FFN_ACTS = ("tanh", "hardtanh", "selu")
GRADS = ("pos_bias_u", "linear_pos.weight", "conv.weight", "pooling_proj1.weight", "weight_proj2.weight", "norm_mlp.weight",
         "merge_proj.bias", "feed_forward_macaron.w_1.weight", "feed_forward_macaron.w_1.bias", "feed_forward.w_1.weight",
         "feed_forward.w_2.weight", "csgu.norm.bias", "linear_k.bias")


def gen_ffn_layers():
    from espnet.nets.pytorch_backend.transformer.embedding import RelPositionalEncoding
    from src.encoder.branchformer.encoder import MyBranchformerEncoder

    B, T, D = 3, 23, 256
    lens = torch.tensor([23, 17, 9])
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, None, :]
    pe = RelPositionalEncoding(D, 0.0)
    for act in FFN_ACTS:
        enc = MyBranchformerEncoder(input_size=D, num_blocks=1, input_layer=None, dropout_rate=0.0,
                                    positional_dropout_rate=0.0, attention_dropout_rate=0.0, ffn_activation_type=act,
                                    merge_method="learned_ave")
        layer = enc.encoders[0].train()
        fill_parameters_(layer, seed=21)
        zs = []
        hooks = [m.w_1.register_forward_hook(lambda _m, _i, o: zs.append(o.detach()))
                 for m in (layer.feed_forward_macaron, layer.feed_forward)]
        x = synth((B, T, D), seed=22).requires_grad_(True)
        xs, pos = pe(x)
        (y, _), _ = layer((xs, pos), mask)
        (y * synth((B, T, D), seed=23)).sum().backward()
        for h in hooks:
            h.remove()
        z = torch.cat([t.flatten() for t in zs])
        grads = {"g_" + n: compact(p.grad) for n, p in layer.named_parameters() if n.endswith(GRADS)}
        _save(f"bf_layer_ffn_{act}", B=B, T=T, D=D, lens=_np(lens), y=_np(y), grad_x=_np(x.grad),
              keys=np.array(sorted(layer.state_dict().keys())), weight_global=_np(layer.weight_global),
              z_frac=np.array([float((z.abs() < 0.25).double().mean()), float((z.abs() >= 1).double().mean())]), **grads)


def main():
    _shim.install()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_ffn_layers()


if __name__ == "__main__":
    main()
