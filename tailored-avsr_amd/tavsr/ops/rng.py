"""The device generator of the dropout masks and the stand-alone dropout launches."""
from __future__ import annotations

import torch

from .._lib import ACT, check, lib, ptr, require_cuda, stream

__all__ = ["rng_state", "manual_seed", "rng_step_begin", "step_seed", "_new_token", "dropout", "dropout_add", "dropout_act_bwd"]


# ---------------------------------------------------------------------------------------------- dropout
# The generator state is ONE uint64 per device, resident in HBM.  ``rng_step_begin`` advances it with a kernel (so a
# captured step graph draws new masks at every replay), writes the advanced value into a fresh one-element tensor that
# belongs to THIS forward pass, and rewinds the per-step site counter, which hands every dropout call of the pass its own,
# reproducible counter range.  A dropout call returns the token (p, offset, step seed tensor) that regenerates its mask
# in the backward pass: the token owns the seed it was drawn with, so a second forward pass (micro-batches, a validation
# pass, another model) before the first backward cannot change the masks that backward regenerates.
_RNG = {}
_STEP_SEED = {}
_SITE = [0]


def _dev_index(device=None) -> int:
    return torch.cuda.current_device() if device is None or device.index is None else device.index


def rng_state(device=None) -> torch.Tensor:
    dev = _dev_index(device)
    t = _RNG.get(dev)
    if t is None:
        t = _RNG[dev] = torch.full((1,), 0x5EED5EED, dtype=torch.int64, device=f"cuda:{dev}")
    return t


def manual_seed(seed: int, device=None):
    """the seeding hook of the device generator (dropout masks); data-parallel ranks seed with base + rank (dp.init_from_env)."""
    rng_state(device).fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
    _STEP_SEED.pop(_dev_index(device), None)
    _SITE[0] = 0


def rng_step_begin(device=None):
    """call once per forward pass (before its first dropout site)."""
    dev = _dev_index(device)
    step = torch.empty(1, dtype=torch.int64, device=f"cuda:{dev}")     # inside a graph capture: lives in the graph's pool
    check(lib().tavsr_rng_step(ptr(rng_state(device)), ptr(step), stream()), "tavsr_rng_step")
    _STEP_SEED[dev] = step
    _SITE[0] = 0


def step_seed(device=None) -> torch.Tensor:
    """the seed tensor new dropout sites draw from: the current pass's copy (the live state before any rng_step_begin)."""
    t = _STEP_SEED.get(_dev_index(device))
    return rng_state(device) if t is None else t


def _new_token(p, n, device):
    tok = (float(p), _SITE[0], step_seed(device))
    _SITE[0] += (n + 3) // 4 * 4
    return tok


def dropout(x, p: float, out=None, token=None):
    """y = dropout(x, p); returns (y, token).  ``token`` from a previous call reproduces that call's mask."""
    require_cuda(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    n = x.numel()
    if token is None:
        token = _new_token(p, n, x.device)
    check(lib().tavsr_dropout(ptr(x), ptr(out), n, token[0], ptr(token[2]), token[1], stream()), "tavsr_dropout")
    return out, token


def dropout_add(a, t, p: float, alpha: float = 1.0, out=None):
    """y = a + alpha * dropout(t, p) in one pass; returns (y, token) - the token is the one ``dropout(t)`` would give."""
    require_cuda(a, t)
    assert a.is_contiguous() and t.is_contiguous() and a.numel() == t.numel()
    if out is None:
        out = torch.empty_like(a)
    n = t.numel()
    token = _new_token(p, n, a.device)
    check(lib().tavsr_dropout_add(ptr(a), ptr(t), ptr(out), n, p, alpha, ptr(token[2]), token[1], stream()), "tavsr_dropout_add")
    return out, token


def dropout_act_bwd(dh, z, act, token, out=None):
    """dz = dropout_mask(dh) * act'(z) with the mask of ``token`` (the site that dropped act(z) in the forward pass)."""
    require_cuda(dh, z)
    assert dh.is_contiguous() and z.is_contiguous() and dh.numel() == z.numel()
    if out is None:
        out = torch.empty_like(dh)
    check(lib().tavsr_dropout_act_bwd(ptr(dh), ptr(z), ptr(out), dh.numel(), token[0], ACT[act], ptr(token[2]), token[1], stream()),
          "tavsr_dropout_act_bwd")
    return out
