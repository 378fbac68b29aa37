"""What every family starts from: the allocation helper, the address hook and the small operand tables."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib as L
from .._lib import ACT, AttnDesc, GemmDesc, check, lib, ptr, require_cuda, stream  # noqa: F401

# (the imports are part of the surface - the tree reaches ``ops.lib``, ``ops.ACT`` and ``ops.require_cuda`` -: tests/golden/ops_public_names.txt)
__all__ = ["C", "L", "torch", "Sequence", "ACT", "AttnDesc", "GemmDesc", "check", "lib", "ptr", "require_cuda", "stream",
           "f32", "empty", "_addr", "_zero_page", "_ptr_array", "_i32"]


f32 = torch.float32


def empty(*shape, like: Optional[torch.Tensor] = None, dtype=f32, device=None):
    dev = like.device if like is not None else (device if device is not None else "cuda")
    return torch.empty(shape, dtype=dtype, device=dev)


_addr = L.addr      # tensor (+ element offset) -> integer address; the stream-safety hook lives there (_lib.py)


_ZERO = {}


def _zero_page(device) -> torch.Tensor:
    z = _ZERO.get(device)
    if z is None:
        z = _ZERO[device] = torch.zeros(64, dtype=f32, device=device)
    return z


def _ptr_array(ts: Sequence[torch.Tensor]):
    require_cuda(*ts)
    return (C.c_void_p * len(ts))(*[_addr(t) for t in ts])


def _i32(*tensors):
    require_cuda(*tensors)
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in tensors)
