"""Float64 restatement of gradient clipping as espnet's trainer applies it around Adam: ``torch.nn.utils.clip_grad_norm_``'s
total norm and coefficient, "a step whose norm is NaN or Inf is not taken", and step counts (bias corrections, the learning-rate
schedule) that advance on taken steps only.  The Adam arithmetic is torch's single-tensor Adam / AdamW, operation by operation,
as the harness tests use it (tests/test_train_harness.py)."""
import math

import torch


def total_norm(grads, norm_type=2.0):
    """norm over every gradient that is not None, as one vector; NaN propagates for both norm types (torch.norm does)"""
    flat = [g.detach().to(torch.float64).reshape(-1) for g in grads if g is not None]
    if not flat:
        return 0.0
    v = torch.cat(flat)
    if bool(torch.isnan(v).any()):
        return math.nan
    if norm_type == math.inf:
        return float(v.abs().max())
    assert norm_type == 2.0, norm_type
    return math.sqrt(float((v * v).sum()))


def clip_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def adam_clip_steps(params, grads_per_step, max_norm, norm_type=2.0, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.0):
    """``params``: tensors (copied to float64).  ``grads_per_step``: one list per step with a tensor or None per parameter.
    ``lr``: a number, or a function of the 1-based count of the step being taken (Noam's ``_step``, a scheduler's position + 1).
    ``max_norm`` None or <= 0: no clipping and no skipping.  A parameter without a gradient is left alone and keeps its own step
    count, as torch.optim.Adam does.  Returns (parameters, log); log[k] = dict(norm, coef, skipped, clipped, count, lr) of step
    k + 1, ``count`` being the number of steps taken including this one if it is taken."""
    b1, b2 = betas
    p = [x.detach().to(torch.float64).clone() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    steps, taken, log = [0] * len(p), 0, []
    for grads in grads_per_step:
        gs = [None if g is None else g.detach().to(torch.float64) for g in grads]
        clipping = max_norm is not None and max_norm > 0
        norm = total_norm(gs, norm_type) if clipping else None
        rate = lr(taken + 1) if callable(lr) else lr
        if clipping and not math.isfinite(norm):
            log.append(dict(norm=norm, coef=0.0, skipped=True, clipped=False, count=taken, lr=rate))
            continue
        coef = clip_coef(norm, max_norm) if clipping else 1.0
        taken += 1
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g * coef
            steps[i] += 1
            m[i] = m[i] + (g - m[i]) * (1 - b1)
            v[i] = v[i] * b2 + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** steps[i], 1 - b2 ** steps[i]
            denom = v[i].sqrt() / math.sqrt(bc2) + eps
            p[i] = p[i] * (1 - rate * weight_decay) - (rate / bc1) * (m[i] / denom)
        log.append(dict(norm=norm, coef=coef, skipped=False, clipped=coef < 1.0, count=taken, lr=rate))
    return p, log
