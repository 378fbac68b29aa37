"""``JointNetwork`` - counterpart of espnet2.asr_transducer.joint_network.JointNetwork (built by the task beside a transducer
decoder, src/tasks/avsr.py:665-670): ``lin_out(tanh(lin_enc(enc) + lin_dec(dec)))`` with ``lin_dec`` bias-free.  Same
constructor arguments and ``state_dict`` keys.  ``forward`` serves the search's single rows; training never calls it: the loss
node (``functional_rnnt.RNNTLossFn``) takes the three Linears' parameters and walks the lattice in chunks."""
from __future__ import annotations

import torch

from .. import ops


class JointNetwork(torch.nn.Module):
    def __init__(self, output_size: int, encoder_size: int, decoder_size: int, joint_space_size: int = 256,
                 joint_activation_type: str = "tanh", **activation_parameters):
        super().__init__()
        if joint_activation_type != "tanh":
            raise ValueError(f"joint_activation_type: {joint_activation_type} is not on the HIP path: the joint kernels apply tanh")
        self.lin_enc = torch.nn.Linear(encoder_size, joint_space_size)
        self.lin_dec = torch.nn.Linear(decoder_size, joint_space_size, bias=False)
        self.lin_out = torch.nn.Linear(joint_space_size, output_size)
        self.joint_space_size, self.output_size = joint_space_size, output_size

    def params(self):
        return (self.lin_enc.weight, self.lin_enc.bias, self.lin_dec.weight, self.lin_out.weight, self.lin_out.bias)

    @torch.no_grad()
    def forward(self, enc_out: torch.Tensor, dec_out: torch.Tensor) -> torch.Tensor:
        """enc_out (..., encoder_size), dec_out (..., decoder_size) with equal leading shapes -> logits (..., output_size)"""
        lead = enc_out.shape[:-1]
        e = ops.linear(enc_out.reshape(-1, enc_out.shape[-1]).contiguous(), self.lin_enc.weight, self.lin_enc.bias)
        d = ops.linear(dec_out.reshape(-1, dec_out.shape[-1]).contiguous(), self.lin_dec.weight)
        frame = torch.zeros(1, dtype=torch.int32, device=e.device)
        z = ops.rnnt_frame_z(e.view(e.shape[0], 1, -1), d, frame)
        return ops.linear(z, self.lin_out.weight, self.lin_out.bias).view(*lead, -1)
