"""GPU: the fused attention core (csrc/attn_fused.hip: forward, backward pass 0 = dQu / dQv, pass 1 = dK / dV / ds_skew) at its
loop bounds - key tiles of 32, online-softmax blocks of 128 keys, workgroups of four query tiles -, under the causal tile
cut-off, with T1 far from T2, with a running maximum that moves between key blocks, beside an utterance without keys, with other
head counts, and under dropout with the mask PREDICTED on the host from the Philox counters (tests/mask_draw_ref.py).  Sections
1 - 3 hold the fallback route (``_SelfAttnCore`` on the csrc/attn.hip kernels) to the same float64 reference at the same shapes;
section 8 runs that route at the head sizes only it takes (dk = 32 / 128).

Every float64 case: outputs pre-filled with NaN must come back finite, ``ctx`` within 2e-5 and every gradient within 5e-5 of the
reference in max |a - b| / max |b| (the figures of test_gpu_attn.py), and a second identical call is bit-equal (no atomics).

Where a reference gradient is identically zero - every query row has ONE live key, so the softmax Jacobian vanishes (T2 = 1,
T = 1) - the measure has no denominator.  The kernel computes dS = p (dPd - D) scale there with dPd and D two float32 dot
products of the same 64 terms in different orders, so its dS is rounding noise of the size of those terms, not 0: such a gradient
is held to 5e-5 of the largest value of the same gradient with the subtraction left out (dS+ = p dPd scale, ``_uncancelled``) -
the same relative accuracy, measured against what is summed."""
import argparse
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import mask_draw_ref as P
from helpers import TOKENS_EN, asr_conf, grad_ok, rel_err, relu_gated_tol
from test_gpu_attn import _ref

pytestmark = pytest.mark.gpu

NAMES = ("ctx", "dq", "dk", "dv", "dqv", "dpos")
FLOOR = {"ctx": 2e-5, "dq": 5e-5, "dk": 5e-5, "dv": 5e-5, "dqv": 5e-5, "dpos": 5e-5}


# ------------------------------------------------------------------------------------------------ inputs, reference, routes
def _inputs(B, T1, T2, H, rel, seed, dk=64, q_scale=1.0, k_blocks=None, device="cuda"):
    """q [B*T1, H*dk], k / v [B*T2, H*dk], pos [2*T1-1, H*dk], the two biases [H*dk] and the context gradient, drawn on the host
    (the same numbers wherever the file runs).  ``k_blocks`` [B][..]: utterance b's keys j are scaled by k_blocks[b][j // 128]."""
    g = torch.Generator().manual_seed(seed)
    D = H * dk
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v, dctx = r(B * T1, D) * q_scale, r(B * T2, D), r(B * T2, D), r(B * T1, D)
    pos = r(2 * T1 - 1, D) if rel else None
    u, vb = (r(D) * 0.5, r(D) * 0.5) if rel else (None, None)
    if k_blocks is not None:
        w = torch.tensor(k_blocks)[:, torch.arange(T2) // 128]                       # [B, T2]
        k = (k.view(B, T2, D) * w[:, :, None]).reshape(B * T2, D)
    cu = lambda t: None if t is None else t.to(device).contiguous()
    return dict(q=cu(q), k=cu(k), v=cu(v), pos=cu(pos), u=cu(u), vb=cu(vb), dctx=cu(dctx))


def _uncancelled(attn, dctx4, qu, qv, k, v, pos, scale):
    """largest |value| of the score-side gradients with dS+ = attn * dPd * scale in place of dS = attn * (dPd - D) * scale"""
    B, T1, T2 = qu.shape[0], qu.shape[1], k.shape[1]
    g = attn * torch.einsum("bihd,bjhd->bhij", dctx4, v) * scale
    out = {"dq": torch.einsum("bhij,bjhd->bihd", g, k), "dk": torch.einsum("bhij,bihd->bjhd", g, qu)}
    if pos is not None:
        idx = (T1 - 1 - torch.arange(T1, device=g.device))[:, None] + torch.arange(T2, device=g.device)[None, :]
        gs = torch.zeros(B, g.shape[1], T1, 2 * T1 - 1, dtype=g.dtype, device=g.device).scatter_(3, idx.expand_as(g), g)
        out["dqv"] = torch.einsum("bhic,chd->bihd", gs, pos)
        out["dpos"] = torch.einsum("bhic,bihd->chd", gs, qv)
    return {n: float(t.abs().max()) for n, t in out.items()}


def _ref_heads(qu, qv, k, v, pos, lens, causal, mask, keep):
    """``_ref`` is written for four heads; heads are independent, so another head count goes through it four heads at a time, the
    last group filled up with all-zero heads whose results are cut off again"""
    H = qu.shape[2]
    pad = (-H) % 4

    def fill(t, d):
        if t is None or pad == 0:
            return t
        return torch.cat([t, t.new_zeros(*t.shape[:d], pad, *t.shape[d + 1:])], d)
    qu, qv, k, v, pos, mask = fill(qu, 2), fill(qv, 2), fill(k, 2), fill(v, 2), fill(pos, 1), fill(mask, 1)
    outs = [_ref(qu[:, :, g:g + 4], qv[:, :, g:g + 4], k[:, :, g:g + 4], v[:, :, g:g + 4], None if pos is None else pos[:, g:g + 4],
                 lens, causal, drop_mask=None if mask is None else mask[:, g:g + 4], keep=keep) for g in range(0, H + pad, 4)]
    return torch.cat([o[0] for o in outs], 2)[:, :, :H], torch.cat([o[1] for o in outs], 1)[:, :H]


def _reference(x, B, T1, T2, H, klens, causal, dk=64, dtype=torch.float64, mask=None, keep=1.0):
    """``_ref`` of test_gpu_attn.py with (q + u) and (q + v) as separate leaves -> dict of ctx, every gradient (flat, as the kernels
    lay them out), the probabilities and, for gradients that are identically zero, the ``_uncancelled`` scale.  ``_ref`` divides by
    sqrt(64): another head size goes in with its queries scaled by sqrt(64 / dk), inside the graph."""
    D = H * dk
    dev = x["q"].device
    lens = torch.full((B,), T2, device=dev) if klens is None else torch.tensor(klens, device=dev).clamp(max=T2)
    q4 = x["q"].to(dtype).view(B, T1, H, dk)
    rel = x["pos"] is not None
    qu = (q4 + (x["u"].to(dtype).view(H, dk) if rel else 0)).detach().requires_grad_(True)
    qv = (q4 + (x["vb"].to(dtype).view(H, dk) if rel else 0)).detach().requires_grad_(True)
    k4 = x["k"].to(dtype).view(B, T2, H, dk).detach().requires_grad_(True)
    v4 = x["v"].to(dtype).view(B, T2, H, dk).detach().requires_grad_(True)
    p4 = x["pos"].to(dtype).view(-1, H, dk).detach().requires_grad_(True) if rel else None
    f = math.sqrt(64.0 / dk)
    ctx, attn = _ref_heads(qu * f, qv * f, k4, v4, p4, lens, causal, None if mask is None else mask.to(dtype), keep)
    dctx4 = x["dctx"].to(dtype).view(B, T1, H, dk)
    ctx.backward(dctx4)
    out = dict(ctx=ctx.detach().reshape(B * T1, D), dq=qu.grad.reshape(B * T1, D), dk=k4.grad.reshape(B * T2, D),
               dv=v4.grad.reshape(B * T2, D), attn=attn.detach(), lens=lens)
    if rel:
        out.update(dqv=qv.grad.reshape(B * T1, D), dpos=p4.grad.reshape(-1, D))
    if dtype == torch.float64 and any(float(out[n].abs().max()) == 0.0 for n in NAMES if n in out):
        pd = attn.detach() if mask is None else attn.detach() * mask.to(dtype) / keep
        out["uncancelled"] = _uncancelled(pd, dctx4, qu.detach(), qv.detach(), k4.detach(), v4.detach(),
                                          None if p4 is None else p4.detach(), 1.0 / math.sqrt(dk))
    return out


@functools.lru_cache(maxsize=None)
def _case(B, T1, T2, H, rel, causal, klens, seed, dk=64):
    """inputs and float64 reference of one case, computed once and shared by the routes (nobody writes to either)"""
    x = _inputs(B, T1, T2, H, rel, seed, dk=dk)
    return x, _reference(x, B, T1, T2, H, klens, causal, dk=dk)


def _nan(rows, D):
    return torch.full((rows, D), float("nan"), device="cuda")


def _run_fused(x, B, T1, T2, H, klens, causal, p_att=0.0, saved=None):
    """one forward (unless ``saved`` = (ctx, saved state) of an earlier one is given) and one backward on the fused kernels"""
    from tavsr import functional as F_
    D = H * 64
    kl = None if klens is None else torch.tensor(klens, device="cuda")
    kw = dict(pos=x["pos"], bias_u=x["u"], bias_v=x["vb"])
    if saved is None:
        ctx, sv = F_._AttnFused.fwd(x["q"], 0, x["k"], 0, x["v"], 0, B, T1, T2, H, 64, kl, causal, p_att=p_att, **kw)
    else:
        ctx, sv = saved
    dq, dk_, dv_ = _nan(B * T1, D), _nan(B * T2, D), _nan(B * T2, D)
    dqv, dp = F_._AttnFused.bwd(x["dctx"], ctx, sv, x["q"], 0, x["k"], 0, x["v"], 0, dq, 0, dk_, 0, dv_, 0, B, T1, T2, H, 64, kl,
                                causal, **kw)
    out = dict(ctx=ctx, dq=dq, dk=dk_, dv=dv_, lse=sv[0], tok=sv[1], saved=(ctx, sv))
    if x["pos"] is not None:
        out.update(dqv=dqv, dpos=dp)
    return out


def _run_core(x, B, T1, T2, H, klens, causal, dk=64):
    """the same on the GEMM + softmax chain (``_SelfAttnCore``, csrc/attn.hip)"""
    from tavsr import functional as F_
    from tavsr import ops
    D = H * dk
    kl = None if klens is None else torch.tensor(klens, device="cuda")
    qu, qv = (x["q"], None) if x["pos"] is None else ops.add_head_bias(x["q"], x["u"], x["vb"])
    ctx, attn, tok = F_._SelfAttnCore.fwd(qu, D, 0, x["k"], D, 0, x["v"], D, 0, B, T1, T2, H, dk, kl, causal, qv=qv, p=x["pos"])
    dq, dk_, dv_ = _nan(B * T1, D), _nan(B * T2, D), _nan(B * T2, D)
    dqv, dp = F_._SelfAttnCore.bwd(x["dctx"], attn, qu, D, 0, x["k"], D, 0, x["v"], D, 0, dq, D, 0, dk_, D, 0, dv_, D, 0, B, T1, T2,
                                   H, dk, qv=qv, p=x["pos"], tok=tok)
    out = dict(ctx=ctx, dq=dq, dk=dk_, dv=dv_)
    if x["pos"] is not None:
        out.update(dqv=dqv, dpos=dp)
    return out


def _err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _close(got, ref, tag, tol=FLOOR):
    """finite, and within ``tol`` of the reference per output (a gradient whose reference is identically zero: see the header)"""
    for n in NAMES:
        if n not in ref:
            assert got.get(n) is None, (tag, n)
            continue
        a, b = got[n], ref[n]
        assert a.shape == b.shape, (tag, n, a.shape, b.shape)
        assert bool(torch.isfinite(a).all()), (tag, n)
        if float(b.abs().max()) == 0.0:
            scale = ref["uncancelled"][n]
            assert scale > 0.0, (tag, n)
            e = float(a.double().abs().max()) / scale
        else:
            e = _err(a, b)
        assert e < tol[n], (tag, n, e)


def _same_bits(a, b, tag):
    for n in NAMES:
        if a.get(n) is not None:
            assert torch.equal(a[n], b[n]), (tag, n)


def _check(route, B, T1, T2, H, rel, causal, klens, seed, dk=64):
    x, ref = _case(B, T1, T2, H, rel, causal, None if klens is None else tuple(klens), seed, dk)
    tag = (route, B, T1, T2, H, rel, causal, klens)
    run = (lambda: _run_fused(x, B, T1, T2, H, klens, causal)) if route == "fused" else \
          (lambda: _run_core(x, B, T1, T2, H, klens, causal, dk=dk))
    got = run()
    _close(got, ref, tag)
    _same_bits(got, run(), tag)
    return x, ref, got


ROUTES = pytest.mark.parametrize("route", ["fused", "core"])


# ------------------------------------------------------------------------------------------------ 1. boundary sweep, rel-pos
@ROUTES
@pytest.mark.parametrize("T,klens", [
    (1, [1, 1]),               # W = 2T - 1 = 1: every positional row is the clamped one
    (31, [31, 1]), (32, [32, 31]), (33, [33, 32]),                    # the key / query tile of 32
    (64, [64, 33]),
    (127, [127, 96]), (128, [128, 127]), (129, [129, 128]),           # the key block and the workgroup of 128
    (160, [160, 129]),
    (256, [256, 255]), (257, [257, 256]),                             # two blocks, two workgroups
    (129, None),               # klens == NULL
    (129, [136, 129]),         # klens > T2 is clamped to T2
])
def test_rel_pos_self_attention_at_tile_and_block_boundaries(route, T, klens):
    _check(route, 2, T, T, 4, True, False, klens, seed=1000 + T)


# ------------------------------------------------------------------------------------------------ 2. causal
@ROUTES
@pytest.mark.parametrize("T", [1, 32, 33, 128, 129, 257])
def test_causal_self_attention_across_the_tile_cut_off(route, T):
    """decoder / LM self-attention: the causal cut-off of the key-tile loops on and beside a tile and a block boundary; rows
    i >= klens keep exactly klens keys"""
    klens = [T, max(1, T - 32), 1]
    _, ref, _ = _check(route, 3, T, T, 4, False, True, klens, seed=2000 + T)
    live = (ref["attn"] > 0).sum(-1)                                                            # [B, H, T]
    want = torch.minimum(torch.arange(1, T + 1, device="cuda")[None, :], ref["lens"][:, None])  # min(i + 1, klens)
    assert torch.equal(live, want[:, None, :].expand_as(live))


# ------------------------------------------------------------------------------------------------ 3. cross attention
@ROUTES
@pytest.mark.parametrize("T1,T2,klens", [
    (1, 129, [129, 128]),
    (5, 499, [499, 257]),          # the decoder over a 20 s memory: four key blocks for one query tile
    (33, 128, [128, 1]),
    (200, 7, [7, 3]),              # pass 1 of the backward: two workgroups launched, one key tile
    (129, 1, [1, 1]),
    (40, 257, [256, 33]),
])
def test_cross_attention_with_very_different_lengths(route, T1, T2, klens):
    _check(route, 2, T1, T2, 4, False, False, klens, seed=3000 + T1 + T2)


# ------------------------------------------------------------------------------------------------ 4. no keys beside live ones
@pytest.mark.parametrize("T1,T2,rel,causal", [(129, 129, True, False), (129, 129, False, True), (33, 129, False, False)])
def test_an_utterance_without_keys_among_live_ones(T1, T2, rel, causal):
    """klens = [T2, 0, 1]: utterance 1 gets exact zeros (ctx, dq, dk, dv, dqv, its ds_skew slab) and lse = +inf, takes no part in
    dpos, and its neighbours meet the float64 tolerances"""
    from tavsr import ops
    B, H, D = 3, 4, 256
    klens = [T2, 0, 1]
    x, ref, got = _check("fused", B, T1, T2, H, rel, causal, klens, seed=4000 + T1 + T2 + int(causal))
    for n, T in (("ctx", T1), ("dq", T1), ("dk", T2), ("dv", T2), ("dqv", T1)):
        if n in ref:
            assert float(ref[n].reshape(B, T, D)[1].abs().max()) == 0.0
            assert int((got[n].view(B, T, D)[1] != 0).sum()) == 0, n
    lse = got["lse"].view(B, H, T1)
    assert bool((lse[1] == float("inf")).all()) and bool(torch.isfinite(lse[[0, 2]]).all())
    if rel:
        kl = torch.tensor(klens, device="cuda")
        dq, dk_, dv_ = _nan(B * T1, D), _nan(B * T2, D), _nan(B * T2, D)
        ctx, (lse_, tok) = got["saved"]
        _, sk = ops.attn_bwd(x["dctx"], ctx, lse_, tok, x["q"], 0, x["k"], 0, x["v"], 0, B, T1, T2, H, 64, dq, 0, dk_, 0, dv_, 0,
                             klens=kl, pos=x["pos"], bias_u=x["u"], bias_v=x["vb"])
        assert sk.shape[:3] == (H, B, T1) and int((sk[:, 1] != 0).sum()) == 0 and float(sk[:, 0].abs().max()) > 0.0
        # the positional gradient without utterance 1 altogether (its rows are zero in the reference too)
        keep = [0, 2]
        sel = lambda t, T: t.view(B, T, D)[keep].reshape(-1, D).contiguous()
        x2 = dict(q=sel(x["q"], T1), k=sel(x["k"], T2), v=sel(x["v"], T2), dctx=sel(x["dctx"], T1), pos=x["pos"], u=x["u"], vb=x["vb"])
        ref2 = _reference(x2, 2, T1, T2, H, [klens[b] for b in keep], causal)
        assert _err(ref2["dpos"], ref["dpos"]) < 1e-12 and _err(got["dpos"], ref2["dpos"]) < FLOOR["dpos"]


# ------------------------------------------------------------------------------------------------ 5. head counts, refusals
@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("rel,causal", [(True, False), (False, True)])
def test_other_head_counts(H, rel, causal):
    """b = bh / H, h = bh % H with H = 1 (D = 64) and H = 8 (D = 512): one partial second tile, ragged keys"""
    _check("fused", 2, 33, 33, H, rel, causal, [33, 20], seed=5000 + H + int(rel))


def _refused(code, B, T1, T2, H, dk, q_off=0, with_pos=False):
    """``tavsr_attn_fwd`` and ``tavsr_attn_bwd`` at the C entry points must return ``code`` from the shared argument check, which
    runs before any launch: every output keeps what it held"""
    from tavsr import _lib, ops
    D = H * dk
    x = torch.zeros(B * max(T1, T2) + 1, D, device="cuda")            # q, k and v: never read
    pos = torch.zeros(2 * T1 - 1, D, device="cuda") if with_pos else None
    d = ops._attn_desc(x, q_off, x, 0, x, 0, B, T1, T2, H, dk, None, False, pos, None, None, None)
    outs = [torch.full((B * T, D), 7.0, device="cuda") for T in (T1, T1, T1, T2, T2)]
    ctx, dq, dqv, dk_, dv_ = outs
    lse = torch.full((B * H, T1), 7.0, device="cuda")
    sk = torch.full((H, B, T1, ops.pad4(2 * T1 - 1)), 7.0, device="cuda") if with_pos else None
    L, p = _lib.lib(), _lib.ptr
    rc = L.tavsr_attn_fwd(C.byref(d), p(ctx), D, p(lse), _lib.stream())
    assert rc == _lib.ENUMS[code], ("fwd", rc, L.tavsr_last_error_string().decode())
    rc = L.tavsr_attn_bwd(C.byref(d), p(x), p(x), D, p(lse), p(dq), p(dqv), D, p(dk_), D, p(dv_), D, p(sk),
                          0 if sk is None else sk.shape[-1], _lib.stream())
    assert rc == _lib.ENUMS[code], ("bwd", rc, L.tavsr_last_error_string().decode())
    torch.cuda.synchronize()
    for t in outs + [lse] + ([sk] if with_pos else []):
        assert bool((t == 7.0).all())


def test_refusals_of_the_fused_entry_points():
    _refused("TAVSR_EUNSUPPORTED", 2, 8, 8, 8, 32)                        # head size 32
    _refused("TAVSR_EINVAL", 2, 5, 7, 4, 64, with_pos=True)               # positions with T1 != T2
    _refused("TAVSR_EALIGN", 2, 8, 8, 4, 64, q_off=1)                     # a q window that starts 4 bytes into a row
    _refused("TAVSR_EUNSUPPORTED", 16384, 1, 1, 4, 64)                    # B * H = 65536: past the grid's y dimension


# ------------------------------------------------------------------------------------------------ 6. a moving running maximum
@pytest.mark.parametrize("T1,rel,causal,seed", [(300, True, False, 0), (300, False, True, 924), (40, False, False, 0)])
def test_running_maximum_that_moves_between_key_blocks(T1, rel, causal, seed):
    """q = 2 randn, keys scaled per block of 128: utterance 0 by [0.5, 1.5, 3.0] - its maximum rises at every block, so the online
    softmax rescales by a tiny alpha -, utterance 1 by [3.0, 1.5, 0.5] - set in block 0, later blocks barely count.  |scaled score|
    reaches ~30, most rows are peaked: the fast exp / log see large arguments.  Bound: max(project floor, 4 * e32), e32 the error
    of the same reference evaluated in float32 (the convention of test_gpu_vocab.py).

    The causal case counts utterance 0's rows i >= 256 only, and row i has just i - 255 keys of the last block against 256 earlier
    ones: about 78 % of those rows peak there with most seeds (72 - 83 % over seeds 0 - 23), so the seed is one of the few (5 of the
    first 1432) whose draw reaches the 85 % asked of the inputs."""
    B, T2, H, klens = 2, 300, 4, [300, 257]
    x = _inputs(B, T1, T2, H, rel, seed=seed, q_scale=2.0, k_blocks=[[0.5, 1.5, 3.0], [3.0, 1.5, 0.5]])
    ref = _reference(x, B, T1, T2, H, klens, causal)
    # the inputs do what they are meant to do (on the reference, never on the kernel's output)
    top, arg = ref["attn"].max(-1)                                                  # [B, H, T1]
    rows0 = slice(256, None) if causal else slice(None)
    last, first = float((arg[0, :, rows0] >= 256).double().mean()), float((arg[1] < 128).double().mean())
    peaked = float((top > 0.5).double().mean())
    print(f"moving max T1={T1} rel={rel} causal={causal}: utt 0 peaks in the last block {last:.3f}, utt 1 in the first {first:.3f}, "
          f"rows with p_max > 0.5 {peaked:.3f}")
    assert last >= 0.85 and first >= 0.85 and peaked >= 0.40
    r32 = _reference(x, B, T1, T2, H, klens, causal, dtype=torch.float32)
    got = _run_fused(x, B, T1, T2, H, klens, causal)
    tol = {}
    for n in NAMES:
        if n in ref:
            e32, ek = _err(r32[n], ref[n]), _err(got[n], ref[n])
            tol[n] = max(FLOOR[n], 4 * e32)
            print(f"  {n}: kernel err {ek:.2e} (e32 {e32:.2e}, ratio {ek / max(e32, 1e-30):.2f})")
    _close(got, ref, ("moving max", T1, rel, causal), tol=tol)
    _same_bits(got, _run_fused(x, B, T1, T2, H, klens, causal), "moving max")


# ------------------------------------------------------------------------------------------------ 7. dropout, mask predicted
def _philox_words(ctr, seed):
    """Philox4x32-10 of mask_draw_ref.py over an array of 64-bit counters -> [n, 4] words (uint64 holding 32-bit values)"""
    M, sh = np.uint64(P.M32), np.uint64(32)
    c0, c1, c2, c3 = ctr & M, ctr >> sh, np.zeros_like(ctr), np.zeros_like(ctr)
    k0, k1 = seed & P.M32, (seed >> 32) & P.M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> sh) ^ c1 ^ np.uint64(k0), (p0 >> sh) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & M, p0 & M, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & P.M32, (k1 + 0xBB67AE85) & P.M32
    return np.stack([c0, c1, c2, c3], axis=1)


def _predicted_mask(tok, B, H, T1, T2):
    """element (b, h, i, j) is kept iff word(offset + ((b*H + h)*T1 + i) * pad4(T2) + j, seed) >= thr"""
    p, offset, seed_t = tok
    seed = int(seed_t.item()) & 0xFFFFFFFFFFFFFFFF
    thr = int(float(np.float32(p)) * 2 ** 32)
    T2p = (T2 + 3) // 4 * 4
    assert offset % 4 == 0
    n4 = B * H * T1 * T2p // 4
    words = _philox_words(np.uint64(offset // 4) + np.arange(n4, dtype=np.uint64), seed)     # word e of counter c: element 4c + e
    for c in (0, 1, n4 // 2, n4 - 1):                                                        # the array form against the scalar one
        for e in range(4):
            assert int(words[c, e]) == P.word(offset + 4 * c + e, seed)
    keep = (words >= np.uint64(thr)).reshape(B, H, T1, T2p)[..., :T2]
    return torch.from_numpy(np.ascontiguousarray(keep)).cuda()


@pytest.mark.parametrize("B,H,T1,T2,rel,causal,klens,p", [
    (2, 4, 150, 150, True, False, [150, 131], 0.1),         # two key blocks
    (2, 4, 130, 130, False, True, [130, 64], 0.25),         # what LM / decoder self-attention runs
    (2, 4, 20, 131, False, False, [131, 67], 0.1),          # pad4(T2) = 132 != T2: the row stride of the counters
    (1, 2, 33, 33, True, False, None, 0.25),
])
def test_dropout_against_the_mask_predicted_from_the_counters(B, H, T1, T2, rel, causal, klens, p):
    """the forward and both backward passes restate the counter arithmetic separately: each is held to the float64 reference under
    the mask computed here from the token (one wrong bit on a live probability moves a ctx row by ~1/T: 100 times the bound)"""
    from tavsr import ops
    x = _inputs(B, T1, T2, H, rel, seed=7000 + T1 + T2)
    ops.manual_seed(4321 + T1)
    got = _run_fused(x, B, T1, T2, H, klens, causal, p_att=p)
    tok = got["tok"]
    assert tok[0] == p and tok[1] == 0
    mask = _predicted_mask(tok, B, H, T1, T2)
    frac = float(mask.double().mean())
    assert abs(frac - (1 - p)) < 4 * math.sqrt(p * (1 - p) / mask.numel()), frac          # four sigma of a fair draw
    ref = _reference(x, B, T1, T2, H, klens, causal, mask=mask, keep=1 - p)
    tag = ("dropout", B, H, T1, T2, rel, causal)
    _close(got, ref, tag)
    # the next site of the same pass: the counter range right behind this one, another mask
    got2 = _run_fused(x, B, T1, T2, H, klens, causal, p_att=p)
    assert got2["tok"][1] - tok[1] == B * H * T1 * ops.pad4(T2)
    mask2 = _predicted_mask(got2["tok"], B, H, T1, T2)
    assert not torch.equal(mask, mask2)
    _close(got2, _reference(x, B, T1, T2, H, klens, causal, mask=mask2, keep=1 - p), tag + ("second",))
    # the first token still regenerates the first mask
    _same_bits(got, _run_fused(x, B, T1, T2, H, klens, causal, saved=got["saved"]), tag)


# ------------------------------------------------------------------------------------------------ 8. head sizes other than 64
@pytest.mark.parametrize("H", [8, 2])
@pytest.mark.parametrize("T", [33, 129])
@pytest.mark.parametrize("rel,causal", [(True, False), (False, True)])
def test_core_route_at_other_head_sizes(H, T, rel, causal):
    """D = 256 as 8 heads of 32 or 2 heads of 128: the GEMM + softmax chain is the only route (the fused entry refuses dk != 64)"""
    _check("core", 2, T, T, H, rel, causal, [T, T - 13], seed=8000 + H + T, dk=256 // H)


def test_model_with_eight_heads_matches_oracle():
    """the audio-only recipe with ``attention_heads: 8`` in encoder and decoder (dk = 32: every attention of the model on the
    core route) against the oracle built from the same dict, at the measures of test_gpu_vsr.py"""
    from oracle.model import build_asr_oracle, fill_parameters_, synth
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=2, dec_blocks=1, attention_heads=8)
    conf["decoder_conf"]["attention_heads"] = 8
    conf["token_list"] = list(TOKENS_EN)
    assert conf["encoder_conf"]["output_size"] // conf["encoder_conf"]["attention_heads"] == 32
    oracle = build_asr_oracle(copy.deepcopy(conf), TOKENS_EN)
    fill_parameters_(oracle, seed=88)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    assert sorted(model.state_dict().keys()) == sorted(oracle.state_dict().keys())
    model.load_state_dict(oracle.state_dict())
    model = model.cuda().train()
    oracle.train()
    B, T = 3, 50
    speech, slens = synth((B, T, 80), seed=15), torch.tensor([50, 41, 30])
    text, tlens = synth((B, 6), seed=16, kind="int", lo=1, hi=40), torch.tensor([6, 4, 2])
    for i, l in enumerate(tlens):
        text[i, l:] = -1
    lo, so, _ = oracle(speech, slens, text, tlens)
    lo.backward()
    lg, sg, _ = model(speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda())
    lg.backward()
    assert rel_err(lg.detach().cpu(), lo.detach()) < 1e-4
    assert rel_err(sg["loss_ctc"].cpu(), so["loss_ctc"]) < 1e-4 and rel_err(sg["loss_att"].cpu(), so["loss_att"]) < 1e-4
    po = dict(oracle.named_parameters())
    for n, p in model.named_parameters():
        if po[n].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        assert grad_ok(p.grad.cpu(), po[n].grad, relu_gated_tol(n, 5e-3)), n
