"""Hand-written forward/backward of the hot-path blocks as ``torch.autograd.Function``s.

Each Function is one node of the autograd graph (a whole Branchformer layer, the whole
Conv2dSubsampling, a decoder layer, ...) whose forward and backward are sequences of C-ABI calls
(``tavsr.ops``).  Gradient accumulation at fan-out points, residual adds, activations and their
derivatives are all fused into those kernels (GEMM epilogues, ``dx_add`` of the LayerNorm
backward), so no torch arithmetic kernel runs on the hot path.  The Python here only orders calls
and owns buffers; it is written so that each Function body can move behind a single C entry point
(`tavsr_bf_layer_fwd/bwd`) without changing callers.

Reference semantics followed are cited per Function.
"""
from __future__ import annotations

import math
import os
from typing import Any, List, NamedTuple, Optional

import torch

from . import ops
from ._lib import guarded

# Does the node being run have a backward pass?  Set by every Function.forward from ctx.needs_input_grad: a forward under
# no_grad / in eval mode does not write the [M, 2048] pre-activations of its feed-forward and cgMLP blocks (26 MB each).
_NEED_BWD = [True]
_GRAD_MODE = [True]


def grad_apply(fn, *args):
    """``fn.apply(*args)`` that also tells the node whether autograd is recording: ``ctx.needs_input_grad`` only mirrors the
    inputs' ``requires_grad`` and ignores ``torch.no_grad()``, and inside ``Function.forward`` grad mode reads disabled."""
    _GRAD_MODE[0] = torch.is_grad_enabled()
    try:
        return fn.apply(*args)
    finally:
        _GRAD_MODE[0] = True


def _note_ctx(ctx):
    """does this node get a backward pass?  (returned, and passed on explicitly by the callers)"""
    nig = getattr(ctx, "needs_input_grad", None)
    need = (True if nig is None else any(nig)) and _GRAD_MODE[0]
    _NEED_BWD[0] = need
    return need


# ------------------------------------------------------------------------------------------------
# building blocks shared by the Functions: tavsr/layer_blocks.py (re-exported: tests and scripts reach them as F_._FFN, ...)
# ------------------------------------------------------------------------------------------------
from .layer_blocks import (EPS_ESPNET, FAST_ATTN_PARAMS, FF_PARAMS, FFM_PARAMS, AttnBranch, AttnSaved, CgmlpBranch,  # noqa: E402,F401
                           CgmlpSaved, FastAttnBranch, FastAttnSaved, FFNSaved, _AttnFused, _drop_, _drop_bwd, _drop_bwd_, _FFN,
                           _SelfAttnCore)

# the positional chain of the attention branch's backward with the layer's weight gradients, beside the chain (read here at call
# time and passed down as ``lazy``: tests flip it on this module)
_POS_DW_BESIDE = os.environ.get("TAVSR_POS_DW_BESIDE", "1") != "0"


# ------------------------------------------------------------------------------------------------
# Branchformer encoder layer
# ------------------------------------------------------------------------------------------------
# the eight parameters of the learned-average merge in the order ops.merge_fwd / merge_bwd take them and the C descriptors'
# ``merge_p`` / ``g_merge_p`` arrays hold them
MERGE_PARAMS = ("pooling_proj1.weight", "pooling_proj2.weight", "pooling_proj1.bias", "pooling_proj2.bias",
                "weight_proj1.weight", "weight_proj2.weight", "weight_proj1.bias", "weight_proj2.bias")

# Every parameter of the layer, once: (name, field of tavsr_bf_layer_desc, gradient field of tavsr_bf_layer_bwd_desc).  No forward
# field: the merge parameters (``merge_p``); no gradient field: those, and the five d_model LayerNorms, whose gradients come back
# in one buffer (``g_ln``, _BWD_NORMS).  The tailored stream's descriptor has the same fields except for its one branch norm
# (``br_ln_w`` / ``br_ln_b``: functional_av._ts_c_desc).
_BF_PARAMS = (
    ("norm_ff_macaron.weight", "ffm_ln_w", None), ("norm_ff_macaron.bias", "ffm_ln_b", None),
    ("feed_forward_macaron.w_1.weight", "ffm_w1", "g_ffm_w1"), ("feed_forward_macaron.w_1.bias", "ffm_b1", "g_ffm_b1"),
    ("feed_forward_macaron.w_2.weight", "ffm_w2", "g_ffm_w2"), ("feed_forward_macaron.w_2.bias", "ffm_b2", "g_ffm_b2"),
    ("norm_mha.weight", "mha_ln_w", None), ("norm_mha.bias", "mha_ln_b", None),
    ("attn.linear_q.weight", "wq", "g_wq"), ("attn.linear_q.bias", "bq", "g_bq"),
    ("attn.linear_k.weight", "wk", "g_wk"), ("attn.linear_k.bias", "bk", "g_bk"),
    ("attn.linear_v.weight", "wv", "g_wv"), ("attn.linear_v.bias", "bv", "g_bv"),
    ("attn.linear_out.weight", "wo", "g_wo"), ("attn.linear_out.bias", "bo", "g_bo"),
    ("attn.linear_pos.weight", "wpos", "g_wpos"), ("attn.pos_bias_u", "pos_u", "g_pos_u"), ("attn.pos_bias_v", "pos_v", "g_pos_v"),
    ("norm_mlp.weight", "mlp_ln_w", None), ("norm_mlp.bias", "mlp_ln_b", None),
    ("cgmlp.channel_proj1.0.weight", "cg_w1", "g_cg_w1"), ("cgmlp.channel_proj1.0.bias", "cg_b1", "g_cg_b1"),
    ("cgmlp.csgu.norm.weight", "csgu_ln_w", "g_csgu_ln_w"), ("cgmlp.csgu.norm.bias", "csgu_ln_b", "g_csgu_ln_b"),
    ("cgmlp.csgu.conv.weight", "csgu_cw", "g_csgu_cw"), ("cgmlp.csgu.conv.bias", "csgu_cb", "g_csgu_cb"),
    ("cgmlp.channel_proj2.weight", "cg_w2", "g_cg_w2"), ("cgmlp.channel_proj2.bias", "cg_b2", "g_cg_b2"),
    *((n, None, None) for n in MERGE_PARAMS),
    ("merge_proj.weight", "merge_w", "g_merge_w"), ("merge_proj.bias", "merge_b", "g_merge_b"),
    ("norm_ff.weight", "ff_ln_w", None), ("norm_ff.bias", "ff_ln_b", None),
    ("feed_forward.w_1.weight", "ff_w1", "g_ff_w1"), ("feed_forward.w_1.bias", "ff_b1", "g_ff_b1"),
    ("feed_forward.w_2.weight", "ff_w2", "g_ff_w2"), ("feed_forward.w_2.bias", "ff_b2", "g_ff_b2"),
    ("norm_final.weight", "final_ln_w", None), ("norm_final.bias", "final_ln_b", None),
)
# parameter order of BranchformerLayerFn (None entries allowed for absent branches): the calling convention of cached_params
BF_PARAM_NAMES = tuple(n for n, _, _ in _BF_PARAMS)
DESC_FIELD = {n: f for n, f, _ in _BF_PARAMS if f is not None}                 # parameter -> field of the forward descriptor
_DESC_PARAMS = tuple((f, n) for n, f, _ in _BF_PARAMS if f is not None)
_BWD_FIELDS = tuple((g, n) for n, _, g in _BF_PARAMS if g is not None)          # gradient slot -> parameter
_I = {n: i for i, n in enumerate(BF_PARAM_NAMES)}
# ... of an E-Branchformer layer (merge ``dwconv``): the same list with the merge convolution's two parameters behind it.  A list of
# its own: a Branchformer layer gathered by it would carry two ``None`` entries, and the C-side backward takes complete lists only.
EBF_PARAM_NAMES = BF_PARAM_NAMES + ("depthwise_conv_fusion.weight", "depthwise_conv_fusion.bias")


# ... of a Branchformer layer whose attention is FastSelfAttention (``fast_selfattn``): its ten parameters in place of the
# relative-position attention's eleven.  A list of its own for the same reason.
_QI = BF_PARAM_NAMES.index("attn.linear_q.weight")
FAST_PARAM_NAMES = BF_PARAM_NAMES[:_QI] + FAST_ATTN_PARAMS + tuple(n for n in BF_PARAM_NAMES[_QI:] if not n.startswith("attn."))


def _param_names(cfg):
    if cfg.get("attn_kind") == "fast_selfattn":
        return FAST_PARAM_NAMES
    return EBF_PARAM_NAMES if cfg["merge"] == "dwconv" else BF_PARAM_NAMES


def _layer_c_ok(x, cfg, P, pd, pos_emb=None) -> bool:
    """the recipe form csrc/layer.hip sequences (both branches, learned-average merge + merge_proj); the shapes are the
    library's to judge (tavsr_branchformer_layer_ok).  Un-captured loops only unless TAVSR_LAYER_C=capture: a captured step
    replays the same kernels either way, and the capture of the Python sequencing measured 1 % faster (allocation order)."""
    if not ops.LAYER_C or ops.PROFILE is not None or (ops.LAYER_C_EAGER_ONLY and torch.cuda.is_current_stream_capturing()):
        return False
    if cfg.get("attn_kind", "rel_selfattn") != "rel_selfattn" or pos_emb is None:      # the sequencer knows the rel_pos attention alone
        return False
    if not (cfg["has_attn"] and cfg["has_mlp"] and cfg["merge"] == "learned_ave" and not cfg["merge_identity"]):
        return False
    B, T, D = x.shape
    cw, w1, w1m = P[_I["cgmlp.csgu.conv.weight"]], P[_I["feed_forward.w_1.weight"]], P[_I["feed_forward_macaron.w_1.weight"]]
    return (x.is_contiguous() and (pos_emb is None or pos_emb.is_contiguous()) and w1.shape == w1m.shape
            and bool(ops.lib().tavsr_branchformer_layer_ok(B, T, D, cfg["heads"], w1.shape[0], 2 * cw.shape[0], cw.shape[-1])))


_DESC_TMPL = {}       # id(parameter list of a layer) -> (storage addresses, descriptor bytes with the parameter fields filled)
_LAYER_LAYOUT = {}    # shape key -> ({buffer: (offset, shape)}, floats): the kept state of one layer as ONE allocation


def _layer_layout(B, T, D, H, N1, C2, need):
    """Every buffer a C-side layer forward writes besides its output, as offsets (256-byte aligned) into one allocation:
    fifty allocator calls and tensor objects per layer were a third of an un-captured step's host time."""
    key = (B, T, D, H, N1, C2, need)
    lay = _LAYER_LAYOUT.get(key)
    if lay is None:
        M, W, Cn = B * T, 2 * T - 1, C2 // 2
        Mp = (M + 127) // 128 * 128
        items = [(k, (M, D)) for k in ("x1", "n_mha", "n_mlp", "cx", "xa", "xm", "m", "x2", "x3")]
        items += [("qkv", (M, 3 * D)), ("pp", (W, D)), ("lse", (B * H, T)), ("g", (M, C2)), ("u", (M, Cn)), ("g_mean", (M,)),
                  ("g_rstd", (M,)), ("score", (2, B, T)), ("pooled", (4, M))]
        rows = {}
        if need:
            items += [("ffm_n", (M, D)), ("ff_n", (M, D))]
            items += [(k, (Mp, N1)) for k in ("ffm_z", "ffm_h", "ff_z", "ff_h")]      # (the streaming kernel writes whole row blocks)
            rows = {k: M for k in ("ffm_z", "ffm_h", "ff_z", "ff_h")}
            items += [("g_z", (M, C2)), ("gn", (M, Cn)), ("conv", (M, Cn))]
            items += [(k, (M,)) for k in ("ffm_mean", "ffm_rstd", "br_mean", "br_rstd", "ff_mean", "ff_rstd", "fin_mean", "fin_rstd")]
        off, o = {}, 0
        for k, shp in items:
            n = 1
            for v in shp:
                n *= v
            off[k] = (o, (rows[k],) + tuple(shp[1:]) if k in rows else tuple(shp))
            o += (n + 63) // 64 * 64
        lay = _LAYER_LAYOUT[key] = (off, o)
    return lay


class _MergeSaved(NamedTuple):
    """kept by the layer's merge and tail: the learned average's scores, its pooled vectors / row dots and the two weights
    [B, 2] (all ``None`` for the other merge forms), the merged rows ``m`` (merge_proj's input; ``None`` from the one-launch tail
    without ``save``) and the tokens of the concat buffer's dropout and of the tail's."""
    score: Any
    pooled: Any
    wts: Any
    m: Any
    t_cat: Any
    t_m: Any


def _layer_sv(flat, off, x2d, toks, wts):
    """the kept state as the tensors the Python sequencing keeps (views of the one allocation)"""
    def g(k):
        e = off.get(k)
        if e is None:
            return None
        o, shp = e
        n = 1
        for v in shp:
            n *= v
        return flat[o: o + n].view(shp)
    return {"ffm": FFNSaved(x=x2d, mean=g("ffm_mean"), rstd=g("ffm_rstd"), n=g("ffm_n"), z=g("ffm_z"), h=g("ffm_h"), t_in=toks[0],
                            t_out=toks[1]),
            "attn": AttnSaved(mean=g("br_mean"), rstd=g("br_rstd"), n=g("n_mha"), qkv=g("qkv"), pp=g("pp"), qu=None, qv=None, cx=g("cx"),
                              attn=(g("lse"), toks[2]), t_att=None, t_br=toks[3]),
            "mlp": CgmlpSaved(mean=g("br_mean"), rstd=g("br_rstd"), n=g("n_mlp"), g=g("g"), z=g("g_z"), gn=g("gn"), gmean=g("g_mean"),
                              grstd=g("g_rstd"), u=g("u"), conv=g("conv"), t_u=toks[4], t_br=toks[5]),
            "merge": _MergeSaved(score=g("score"), pooled=g("pooled"), wts=wts, m=g("m"), t_cat=None, t_m=toks[6]),
            "ff": FFNSaved(x=g("x2"), mean=g("ff_mean"), rstd=g("ff_rstd"), n=g("ff_n"), z=g("ff_z"), h=g("ff_h"), t_in=toks[7],
                           t_out=toks[8]),
            "final": (g("x3"), g("fin_mean"), g("fin_rstd")),
            "x1": g("x1"), "xa": g("xa"), "xm": g("xm")}


class _LazySV:
    """``ctx.sv`` of a C-side forward: the tensors of the Python backward are only built if that path runs"""
    __slots__ = ("flat", "off", "x2d", "toks", "wts", "_sv")

    def __init__(self, flat, off, x2d, toks, wts):
        self.flat, self.off, self.x2d, self.toks, self.wts, self._sv = flat, off, x2d, toks, wts, None

    def __getitem__(self, k):
        if self._sv is None:
            self._sv = _layer_sv(self.flat, self.off, self.x2d, self.toks, self.wts)
        return self._sv[k]


# ---- plumbing of the C sequencers' descriptors (tavsr_bf_layer_desc, tavsr_tailored_stream_desc / _layer_desc)
def _draw_tokens(d, rates, sizes, device):
    """the dropout tokens of a C-side forward, drawn in the order the Python sequencing draws them (same masks either way) and
    written into the descriptor's ``drop_off`` / ``seed``; None where the rate is 0"""
    toks = [ops._new_token(r, n, device) if r and r > 0.0 else None for r, n in zip(rates, sizes)]
    for j, t in enumerate(toks):
        if t is not None:
            d.drop_off[j] = t[1]
            d.seed = ops._addr(t[2])
    return toks


def _side_queue(d):
    """``stream2`` / ``ev_fork`` / ``ev_join`` of a descriptor: the calling stream's side queue and fork / join events (one queue:
    the calling stream itself - the events then order nothing new) -> (calling stream, side queue)"""
    main = torch.cuda.current_stream()
    side = ops.branch_stream(main) if ops.forks_enabled() else main
    ev = ops.branch_events(main)
    d.stream2, d.ev_fork, d.ev_join = side.cuda_stream, ev[0].cuda_event, ev[1].cuda_event
    return main, side


_WS_FLOATS = {}       # (entry point, shape key) -> floats of workspace the library asks for


def _workspace(d, query, key, like):
    """``ws`` / ``ws_floats`` of a descriptor: the size is asked of the library (entry point ``query``) once per shape key, the
    block is allocated per call and returned (the caller keeps it until its launches are enqueued)"""
    import ctypes as C
    nws = _WS_FLOATS.get((query, key))
    if nws is None:
        nws = _WS_FLOATS[(query, key)] = getattr(ops.lib(), query)(C.byref(d))
    ws = ops.empty(max(nws, 4), like=like)
    d.ws, d.ws_floats = ops._addr(ws), nws
    return ws


def _layer_c_forward(ctx, x, pos_emb, lens, cfg, P, need):
    """BranchformerLayerFn.forward as one C call (tavsr_branchformer_layer_fwd).  Host side of an un-captured step: the
    parameter fields of the descriptor come from a per-layer template (rebuilt when a parameter's storage moves), everything the
    call writes besides its output is ONE allocation (``_layer_layout``), and the tensors the Python backward would read are
    views built only if that path runs (``_LazySV``)."""
    from ._lib import BfLayerDesc, check, lib, param_ptrs
    import ctypes as C
    B, T, D = x.shape
    M, H = B * T, cfg["heads"]
    N1 = P[_I["feed_forward.w_1.weight"]].shape[0]
    C2 = P[_I["cgmlp.channel_proj1.0.weight"]].shape[0]
    Cn = C2 // 2
    pd, pa = cfg.get("p", 0.0), cfg.get("p_att", 0.0)
    x2d = x.view(M, D)
    sig = param_ptrs(P)
    tm = _DESC_TMPL.get(id(P))
    if tm is None or tm[0] != sig:
        t = BfLayerDesc()
        for f, n in _DESC_PARAMS:
            setattr(t, f, sig[_I[n]])
        for j, n in enumerate(MERGE_PARAMS):
            t.merge_p[j] = sig[_I[n]]
        tm = _DESC_TMPL[id(P)] = (sig, bytes(t))
    d = BfLayerDesc.from_buffer_copy(tm[1])
    d.B, d.T, d.D, d.H, d.ffn_units, d.cg_units, d.cg_kernel = B, T, D, H, N1, C2, 31
    d.ffn_act, d.save = ops.ACT[cfg["ffn_act"]], int(need)
    d.p_drop, d.p_att, d.coeff = pd, pa, cfg.get("coeff", 1.0)
    d.x, d.pos_emb, d.lens = ops._addr(x2d), ops._addr(pos_emb), ops._addr(lens)
    toks = [None] * 9
    if pd > 0.0 or pa > 0.0:
        sizes = (M * N1, M * D, B * H * T * ops.pad4(T), M * D, M * Cn, M * D, M * D, M * N1, M * D)
        toks = _draw_tokens(d, (pd, pd, pa, pd, pd, pd, pd, pd, pd), sizes, x.device)
    off, nfl = _layer_layout(B, T, D, H, N1, C2, bool(need))
    flat = ops.empty(nfl, like=x)
    y = ops.empty(M, D, like=x)
    wts = ops.empty(B, 2, like=x)      # (its own block: the module keeps it as weight_global / weight_local beyond the step)
    base = ops._addr(flat)
    for k, (o, _) in off.items():
        setattr(d, k, base + 4 * o)
    d.y, d.wts = ops._addr(y), ops._addr(wts)
    main, _ = _side_queue(d)
    ws = _workspace(d, "tavsr_branchformer_layer_ws", (B, T, D, H, N1, C2, int(need), pd > 0.0, pa > 0.0), x)
    check(lib().tavsr_branchformer_layer_fwd(C.byref(d), main.cuda_stream), "tavsr_branchformer_layer_fwd")
    ctx.sv, ctx.cfg, ctx.P, ctx.lens, ctx.pos_emb = _LazySV(flat, off, x2d, toks, wts), cfg, P, lens, pos_emb
    ctx.shape = (B, T, D)
    if need:
        ctx.cdesc = d      # the descriptor (raw addresses of the parameters and of every kept buffer; ctx.sv / ctx.P hold the tensors)
    # (ws goes back to the allocator here: every launch that reads it is enqueued, the side queue has been joined into the calling
    # one inside the call, and the block can only be handed to later work of the calling queue)
    cfg["_last_w"] = wts
    return y.view(B, T, D)


# the five d_model LayerNorms, whose (dgamma, dbeta) pairs come back in one buffer, in its order
_BWD_NORMS = ("norm_final", "norm_ff", "norm_mlp", "norm_mha", "norm_ff_macaron")


_GRAD_LAYOUT = {}     # id(parameter list) -> (shapes, [(slot, field or merge index, offset, numel, shape)], floats)


def _grad_layout(P, D):
    """the layer's parameter gradients as views of ONE allocation (256-byte aligned offsets); the five d_model LayerNorms'
    (dgamma, dbeta) pairs are one contiguous run, as tavsr_branchformer_layer_bwd writes them"""
    shapes = tuple(None if p is None else tuple(p.shape) for p in P)
    lay = _GRAD_LAYOUT.get(id(P))
    if lay is None or lay[0] != shapes:
        ent, o = [], 0
        for f, n in _BWD_FIELDS:
            shp = shapes[_I[n]]
            k = 1
            for v in shp:
                k *= v
            ent.append((_I[n], f, o, k, shp))
            o += (k + 63) // 64 * 64
        for j, n in enumerate(MERGE_PARAMS):
            shp = shapes[_I[n]]
            k = 1
            for v in shp:
                k *= v
            ent.append((_I[n], j, o, k, shp))
            o += (k + 63) // 64 * 64
        ln0 = o
        for j, n in enumerate(_BWD_NORMS):
            ent.append((_I[n + ".weight"], None, o, D, (D,)))
            ent.append((_I[n + ".bias"], None, o + D, D, (D,)))
            o += 2 * D
        lay = _GRAD_LAYOUT[id(P)] = (shapes, ent, ln0, o)
    return lay


def _layer_c_backward(ctx, dy):
    """BranchformerLayerFn.backward as one C call (tavsr_branchformer_layer_bwd) on the state a C forward call left: allocates
    the gradients (one block, handed out as views), fills the descriptor; bit-identical to the Python sequencing below."""
    from ._lib import BfLayerBwdDesc, check, lib
    import ctypes as C
    d, P = ctx.cdesc, ctx.P
    B, T, D = ctx.shape
    M = B * T
    dy2 = dy.contiguous().view(M, D)
    main, side = _side_queue(d)
    b = BfLayerBwdDesc()
    b.fwd = C.pointer(d)
    _, ent, ln0, nfl = _grad_layout(P, D)
    gflat = ops.empty(nfl, like=dy2)
    base = ops._addr(gflat)
    G: List[Optional[torch.Tensor]] = [None] * len(BF_PARAM_NAMES)
    for slot, f, o, k, shp in ent:
        G[slot] = gflat[o: o + k].view(shp)
        if f is None:
            continue
        if isinstance(f, int):
            b.g_merge_p[f] = base + 4 * o
        else:
            setattr(b, f, base + 4 * o)
    dx = ops.empty(M, D, like=dy2)
    b.dy, b.dx, b.g_ln = ops._addr(dy2), ops._addr(dx), base + 4 * ln0
    ws = _workspace(b, "tavsr_branchformer_layer_bwd_ws", (B, T, D, d.H, d.ffn_units, d.cg_units, d.p_drop > 0.0), dy2)
    beside = side is not main and ops.WGRAD_SLOT == 0 and ops.wgrad_may_go_beside(P) and ops.wgrad_open(main, side)
    b.wgrad_beside = 1 if beside else 0
    check(lib().tavsr_branchformer_layer_bwd(C.byref(b), main.cuda_stream), "tavsr_branchformer_layer_bwd")
    if beside:      # what those launches read and write is freed on THIS stream (rule 1 of _lib.py, by hand: the addresses were taken here)
        sv = ctx.sv
        for t in (ws, gflat, dy2, sv.flat, sv.x2d, sv.wts, ctx.pos_emb):
            if torch.is_tensor(t) and not isinstance(t, torch.nn.Parameter):
                t.record_stream(side)
    ctx.sv = ctx.cdesc = None
    return (dx.view(B, T, D), None, None, None, *G)


def _bf_branch_out(h, w, b, cat, off, pd, rowdot):
    """a branch's output projection -> (branch output, its dropout token, the merge's row dots of it): into the branch's half of
    the concat buffer (masked later, both halves in one call), or with the dropout - x1 = dropout(x_att), x2 = dropout(x2):
    encoder_layer.py:212,224 - and, for the fused tail, the merge's row dots in the launch's epilogue"""
    if cat is not None:
        ops.linear(h, w, b, out=cat, out_off=off, ldc=cat.shape[1])
        return cat[:, off: off + w.shape[0]], None, None
    if rowdot is not None and ops.rowdot_ok(h, w):
        return ops.linear_drop(h, w, b, pd, rowdot=rowdot)
    return (*ops.linear_drop(h, w, b, pd), None)


def _bf_merge_fwd(p, cfg, xa, xm, cat, x1, mp, rowdots, lens, B, T, need):
    """the layer behind the branch join: the merge (learned average | fixed average | concat | the one branch there is) and the
    tail x1 + coeff * dropout(merge_proj(m)) - as one launch with the learned average where the kernel takes the shape, with an
    identity merge_proj for a single-branch layer (encoder_layer.py:232-309) -> (x2, _MergeSaved)"""
    merge, pd, coeff = cfg["merge"], cfg.get("p", 0.0), cfg.get("coeff", 1.0)
    D = x1.shape[1]
    t_cat = _drop_(cat, pd) if cat is not None else None      # both halves in one call (iid)
    score = pooled = wts = x2 = None
    if mp is not None:
        if not cfg["merge_identity"] and ops.merge_proj_ok(xa, xm, p["merge_proj.weight"], T, D, res=x1):
            # merge + merge_proj + dropout + residual: the whole tail behind the join as ONE launch
            score, pooled, wts, m, x2, t_m = ops.merge_proj_fwd(xa, xm, lens, mp, p["merge_proj.weight"], p["merge_proj.bias"], x1, coeff,
                                                                pd, B, T, save=need, rowdots=rowdots)
        else:
            score, pooled, wts, m = ops.merge_fwd(xa, xm, lens, mp, B, T)       # pooling + weighted sum: one launch for T <= 128
    elif xa is not None and xm is not None and merge == "fixed_ave":
        cw = cfg["cgmlp_weight"]
        m = ops.axpby(xa, xm, 1.0 - cw, cw)
    elif xa is not None and xm is not None and merge == "concat":
        m = cat
    elif xa is not None and xm is not None and merge == "dwconv":
        # E-Branchformer (espnet2 e_branchformer_encoder.py): merge_proj(cat + depthwise_conv_fusion(cat)); the sum is kept - it is
        # merge_proj's input, which its weight gradient reads - and so is cat, which the convolution's weight gradient reads
        cw = p["depthwise_conv_fusion.weight"]
        m = ops.dwconv_add_fwd(cat, cw.reshape(cw.shape[0], -1), p["depthwise_conv_fusion.bias"], B, T)
    else:
        m = xa if xa is not None else xm
    if x2 is not None:
        pass                                            # (the fused tail above)
    elif cfg["merge_identity"]:
        t_m, md = None, m
        if pd > 0.0:                                    # x + coeff * dropout(x1 | x2)  (encoder_layer.py:302-309)
            md, t_m = ops.dropout(m.contiguous(), pd)
        x2 = ops.axpby(x1, md, 1.0, coeff)
    else:                                               # x + coeff * dropout(merge_proj(.))  (:232-300)
        x2, t_m = ops.linear_drop(m, p["merge_proj.weight"], p["merge_proj.bias"], pd, alpha=coeff, res=x1)
    return x2, _MergeSaved(score=score, pooled=pooled, wts=wts, m=m, t_cat=t_cat, t_m=t_m)


def _bf_merge_bwd(p, cfg, sv, dx2, dxd, lens, B, T, grp, G):
    """backward of _bf_merge_fwd from dx2 (``dxd``: dx2 under the tail's mask, where the LayerNorm backward above wrote it) ->
    (dxa, dxm, masked): the gradients of the two branch outputs (None for an absent branch), and whether they already are under the
    branch outputs' dropout masks (the learned average's backward applies them itself: no mask launches at the head of the
    branches)"""
    ms, coeff, merge = sv["merge"], cfg.get("coeff", 1.0), cfg["merge"]
    has_attn, has_mlp = cfg["has_attn"], cfg["has_mlp"]
    two = has_attn and has_mlp
    if cfg["merge_identity"]:
        dm = ops.axpby(dx2, None, coeff, 0.0) if (coeff != 1.0 or ms.t_m is not None) else dx2
        _drop_bwd_(dm, ms.t_m)
    else:       # merge projection: x2 = x1 + coeff * (m Wm^T + bm)
        dxd = _drop_bwd(dx2, ms.t_m) if dxd is None else dxd
        G["merge_proj.weight"], G["merge_proj.bias"] = grp.add(dxd, ms.m, alpha=coeff, bias_grad=True)
        dm = ops.linear_dx(dxd, p["merge_proj.weight"], alpha=coeff)
    if two and merge == "learned_ave":
        dxa, dxm, mg = ops.merge_bwd(dm, sv["xa"], sv["xm"], lens, [p[k] for k in MERGE_PARAMS], ms.score, ms.pooled, ms.wts, B, T,
                                     drop1=sv["attn"].t_br, drop2=sv["mlp"].t_br)
        G.update((k, g.view_as(p[k])) for k, g in zip(MERGE_PARAMS, mg))
        return dxa, dxm, True
    if two and merge == "fixed_ave":
        cw = cfg["cgmlp_weight"]
        return ops.axpby(dm, None, 1.0 - cw, 0.0), ops.axpby(dm, None, cw, 0.0), False
    if two and merge == "concat":
        D = dx2.shape[1]
        _drop_bwd_(dm, ms.t_cat)
        return dm[:, :D], dm[:, D:], False
    if two and merge == "dwconv":      # dm is the gradient of cat + conv(cat): through the convolution, then as concat
        D = dx2.shape[1]
        cw = p["depthwise_conv_fusion.weight"]
        dm, gcw, G["depthwise_conv_fusion.bias"] = ops.dwconv_add_bwd(dm, sv["cat"], cw.reshape(cw.shape[0], -1), B, T)
        G["depthwise_conv_fusion.weight"] = gcw.view_as(cw)
        _drop_bwd_(dm, ms.t_cat)
        return dm[:, :D], dm[:, D:], False
    return (dm if has_attn else None), (dm if has_mlp else None), False


class BranchformerLayerFn(torch.autograd.Function):
    """``MyBranchformerEncoderLayer.forward`` (src/encoder/branchformer/encoder_layer.py:153-321) with
    dropout / stochastic depth disabled (rate 0 or eval); ``coeff`` is the stochastic-depth scale."""

    @staticmethod
    def forward(ctx, x, pos_emb, lens, cfg, *P):
        need = _note_ctx(ctx)
        pd = cfg.get("p", 0.0)                                # dropout rate (0 in eval)
        if _layer_c_ok(x, cfg, P, pd, pos_emb):
            return _layer_c_forward(ctx, x, pos_emb, lens, cfg, P, need)
        B, T, D = x.shape
        M = B * T
        p = dict(zip(_param_names(cfg), P))
        act, merge = cfg["ffn_act"], cfg["merge"]             # learned_ave | fixed_ave | concat (+ identity flag for one branch)
        has_attn, has_mlp = cfg["has_attn"], cfg["has_mlp"]
        two = has_attn and has_mlp
        sv = {}
        # the macaron block's finishing launch also normalises its output for the two branches (one statistics pass)
        br_norms = ([(p["norm_mha.weight"], p["norm_mha.bias"])] if has_attn else []) + \
                   ([(p["norm_mlp.weight"], p["norm_mlp.bias"])] if has_mlp else [])
        ffs = cfg.get("ff_scale", 0.5)                        # 1.0 for an E-Branchformer layer without the macaron block
        if p["feed_forward_macaron.w_1.weight"] is not None:
            x1, sv["ffm"], nbr, bmean, brstd = _FFN.fwd_ln(x.reshape(M, D), *[p[k] for k in FFM_PARAMS], act, ffs, br_norms, p=pd,
                                                           save=need)
        else:      # (E-Branchformer, macaron_ffn=False) the branch LayerNorms are launches of their own
            x1, sv["ffm"], nbr, bmean, brstd = x.reshape(M, D), None, [], None, None
            for gam, bet in br_norms:
                n_, bmean, brstd = ops.layernorm_fwd(x1, gam, bet, EPS_ESPNET)
                nbr.append(n_)
        cat = ops.empty(M, 2 * D, like=x) if merge in ("concat", "dwconv") else None
        mp = [p[k] for k in MERGE_PARAMS] if two and merge == "learned_ave" else None
        # the fused tail takes the merge's row dots from the epilogues of the launches that store the branch outputs
        use_rd = (mp is not None and ops.MERGE_ROWDOT and not cfg["merge_identity"] and ops.MERGE_PROJ and ops.MERGE_ROWS
                  and bool(ops.lib().tavsr_merge_proj_ok(T, D)))
        xa = xm = rd_a = rd_m = None
        br = ops.BranchScope(two)     # attention branch beside the cgMLP branch (joined before the merge)
        with br:
            if has_attn and cfg.get("attn_kind") == "fast_selfattn":
                # x1 = dropout(attn(x1, mask)): the module's output is the branch's (no linear_out); FastSelfAttention's three
                # dropouts run at attention_dropout_rate (encoder.py:250-257), the layer's own at dropout_rate
                xa, s = FastAttnBranch.fwd(nbr[0], p, lens, B, T, cfg["heads"], cfg.get("p_att", 0.0), out=cat)
                t_xa = None
                if cat is None and pd > 0.0:
                    xa, t_xa = ops.dropout(xa, pd)
                sv["attn"] = s._replace(mean=bmean, rstd=brstd, t_br=t_xa)
            elif has_attn:
                cx, s = AttnBranch.fwd(nbr[0], p, pos_emb, lens, B, T, cfg["heads"], cfg.get("p_att", 0.0))
                xa, t_xa, rd_a = _bf_branch_out(cx, p["attn.linear_out.weight"], p["attn.linear_out.bias"], cat, 0, pd,
                                                (mp[0], mp[4]) if use_rd else None)
                sv["attn"] = s._replace(mean=bmean, rstd=brstd, t_br=t_xa)
        if has_mlp:
            u, s = CgmlpBranch.fwd(nbr[-1], p, B, T, pd, need)
            xm, t_xm, rd_m = _bf_branch_out(u, p["cgmlp.channel_proj2.weight"], p["cgmlp.channel_proj2.bias"], cat, D, pd,
                                            (mp[1], mp[5]) if use_rd else None)
            sv["mlp"] = s._replace(mean=bmean, rstd=brstd, t_br=t_xm)
        br.join()
        x2, sv["merge"] = _bf_merge_fwd(p, cfg, xa, xm, cat, x1, mp, (rd_a, rd_m) if rd_a is not None and rd_m is not None else None,
                                        lens, B, T, need)
        if p["feed_forward.w_1.weight"] is not None:
            x3, sv["ff"], (y,), fmean, frstd = _FFN.fwd_ln(x2, *[p[k] for k in FF_PARAMS], act, ffs,
                                                           [(p["norm_final.weight"], p["norm_final.bias"])], p=pd, save=need)
        else:      # (E-Branchformer, use_ffn=False) norm_final is a LayerNorm of its own
            x3, sv["ff"] = x2, None
            y, fmean, frstd = ops.layernorm_fwd(x2, p["norm_final.weight"], p["norm_final.bias"], EPS_ESPNET)
        sv["final"] = (x3, fmean, frstd)
        sv["x1"], sv["xa"], sv["xm"], sv["cat"] = x1, xa, xm, (cat if merge == "dwconv" else None)
        ctx.sv, ctx.cfg, ctx.P, ctx.lens, ctx.pos_emb = sv, cfg, P, lens, pos_emb
        ctx.shape = (B, T, D)
        cfg["_last_w"] = sv["merge"].wts   # (weight_global, weight_local) for the introspection attributes
        return y.view(B, T, D)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        if (getattr(ctx, "cdesc", None) is not None and ops.LAYER_C and ops.PROFILE is None and all(p is not None for p in ctx.P)
                and not (ops.LAYER_C_EAGER_ONLY and torch.cuda.is_current_stream_capturing())):
            return _layer_c_backward(ctx, dy)
        sv, cfg, P = ctx.sv, ctx.cfg, ctx.P
        B, T, D = ctx.shape
        act = cfg["ffn_act"]
        has_attn, has_mlp = cfg["has_attn"], cfg["has_mlp"]
        p = dict(zip(_param_names(cfg), P))
        G = {}
        beside = ops.wgrad_may_go_beside(P)
        grp = ops.WgradGroup()     # every weight gradient of the layer in one grouped launch (flushed at the end)
        lng = ops.LNGroup()        # ... and the five d=256 LayerNorms' (dgamma, dbeta) partials in one reduction
        x3, fmean, frstd = sv["final"]
        # each LayerNorm backward whose dx the next block's dropout mask is applied to also writes the masked copy
        ffs = cfg.get("ff_scale", 0.5)
        t_ffm = sv["ffm"].t_out if sv["ffm"] is not None else None
        t_m = None if cfg["merge_identity"] else sv["merge"].t_m
        if sv["ff"] is not None:
            dx3, G["norm_final.weight"], G["norm_final.bias"], *dyd = lng.bwd(dy.contiguous().view(B * T, D), x3, fmean, frstd,
                                                                             p["norm_final.weight"], drop=sv["ff"].t_out)
            dx2, gs, *dxd = _FFN.bwd(dx3, sv["ff"], p["norm_ff.weight"], p["feed_forward.w_1.weight"], p["feed_forward.w_2.weight"], act,
                                     ffs, grp=grp, lng=lng, dyd=dyd[0] if dyd else None, out_drop=t_m)
            G.update(zip(FF_PARAMS, gs))
        else:      # no closing feed-forward block: norm_final's backward hands the merge its gradient (and the masked copy)
            dx2, G["norm_final.weight"], G["norm_final.bias"], *dxd = lng.bwd(dy.contiguous().view(B * T, D), x3, fmean, frstd,
                                                                             p["norm_final.weight"], drop=t_m)
        dxa, dxm, masked = _bf_merge_bwd(p, cfg, sv, dx2, dxd[0] if dxd else None, ctx.lens, B, T, grp, G)
        x1 = sv["x1"]
        dx1 = dx2  # residual path; branch gradients are folded in through dx_add
        br = ops.BranchScope(has_attn and has_mlp)     # attention-branch backward beside the cgMLP-branch backward
        late = ()
        with br:
            if has_attn:
                sa = sv["attn"]
                if sa.t_br is not None and not masked:
                    dxa = _drop_bwd(dxa.contiguous(), sa.t_br)
                if cfg.get("attn_kind") == "fast_selfattn":
                    dn_a = FastAttnBranch.bwd(dxa, sa, p, ctx.lens, B, T, cfg["heads"], grp, G)
                else:
                    dn_a, late = AttnBranch.bwd(dxa, sa, p, ctx.pos_emb, ctx.lens, B, T, cfg["heads"], grp, G,
                                                lazy=beside and _POS_DW_BESIDE)
        if has_mlp:
            sm = sv["mlp"]
            if sm.t_br is not None and not masked:
                dxm = _drop_bwd(dxm.contiguous(), sm.t_br)
            dn = CgmlpBranch.bwd(dxm, sm, p, B, T, grp, G)
            dx1, G["norm_mlp.weight"], G["norm_mlp.bias"], *dyd = lng.bwd(dn, x1, sm.mean, sm.rstd, p["norm_mlp.weight"], dx_add=dx1,
                                                                          drop=None if has_attn else t_ffm)
        br.join()
        if has_attn:     # same accumulation order into dx1 as a single stream: cgMLP branch first, then attention
            dx1, G["norm_mha.weight"], G["norm_mha.bias"], *dyd = lng.bwd(dn_a, x1, sa.mean, sa.rstd, p["norm_mha.weight"], dx_add=dx1,
                                                                          drop=t_ffm)
        if sv["ffm"] is not None:
            dx, gs = _FFN.bwd(dx1, sv["ffm"], p["norm_ff_macaron.weight"], p["feed_forward_macaron.w_1.weight"],
                              p["feed_forward_macaron.w_2.weight"], act, ffs, grp=grp, lng=lng, dyd=dyd[0] if dyd else None)
            G.update(zip(FFM_PARAMS, gs))
        else:
            dx = dx1
        if beside:       # no reader before the end of the pass: beside the next layer's chain (the positional chain first)
            ops.wgrad_beside(lambda: ([f() for f in late], grp.flush(), lng.flush()))
        else:
            grp.flush()
            lng.flush()
        ctx.sv = None
        return (dx.view(B, T, D), None, None, None, *[None if prm is None else G.get(n) for n, prm in zip(_param_names(cfg), P)])


# ------------------------------------------------------------------------------------------------
# LayerNorm / Linear as stand-alone nodes (after_norm, ctc_lo, decoder output layer)
# ------------------------------------------------------------------------------------------------
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        y, mean, rstd = ops.layernorm_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, mean, rstd, w)
        return y.view(shp)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        x2, mean, rstd, w = ctx.saved_tensors
        dx, gw, gb = ops.layernorm_bwd(dy.contiguous().view(x2.shape), x2, mean, rstd, w)
        return dx.view(dy.shape), gw, gb, None


class InterCTCConditionFn(torch.autograd.Function):
    """x + conditioning_layer(softmax(ctc_lo(h)))  - self-conditioned intermediate CTC
    (src/encoder/branchformer/encoder.py:389-401, tailored/encoder.py:296-318; ``CTC.softmax`` src/ctc/ctc.py:160-168).
    ``h`` is the (normalised) intermediate output the posteriors are taken from, ``x`` the stream they are added to."""

    @staticmethod
    def forward(ctx, x, h, ctc_w, ctc_b, cond_w, cond_b):
        shp = x.shape
        D = shp[-1]
        x2, h2 = x.reshape(-1, D), h.reshape(-1, D)
        M, V = x2.shape[0], ctc_w.shape[0]
        S = ops.pad4(V)
        logits = ops.empty(1, 1, M, S, like=x)
        ops.linear(h2, ctc_w, ctc_b, out=logits, ldc=S)
        vlen = torch.full((1,), V, dtype=torch.int64, device=x.device)
        prob = ops.softmax_fwd(logits, None, vlen, 1.0, T2=V)
        y = ops.empty(M, D, like=x)
        ops.gemm(M, D, V, prob, S, cond_w, cond_w.stride(0), y, D, bias=cond_b, R=x2, ldr=x2.stride(0))
        ctx.save_for_backward(h2, prob, ctc_w, cond_w)
        ctx.dims = (shp, M, V, S, D)
        return y.view(shp)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        h2, prob, ctc_w, cond_w = ctx.saved_tensors
        shp, M, V, S, D = ctx.dims
        dy2 = dy.contiguous().view(M, D)
        p2 = prob.view(M, S)
        # conditioning layer: y = x + prob W_c^T + b_c
        gcw = ops.empty(D, V, like=dy2)
        ops.gemm(D, V, M, dy2, D, p2, S, gcw, V, a_kmajor=True, b_kmajor=True)
        gcb = ops.colsum(dy2)
        dprob = ops.empty(1, 1, M, S, like=dy2)
        ops.gemm(M, V, D, dy2, D, cond_w, cond_w.stride(0), dprob, S, b_kmajor=True)
        dlog, _ = ops.softmax_bwd(prob, dprob, 1.0, T2=V)
        dl2 = dlog.view(M, S)
        # ctc_lo: logits = h W^T + b
        gw = ops.empty(V, D, like=dy2)
        ops.gemm(V, D, M, dl2, S, h2, h2.stride(0), gw, D, a_kmajor=True, b_kmajor=True)
        gb = ops.empty(V, like=dy2)
        ops.colsum(dl2[:, :V], out=gb)
        dh = ops.empty(M, D, like=dy2)
        ops.gemm(M, D, V, dl2, S, ctc_w, ctc_w.stride(0), dh, D, b_kmajor=True)
        return dy, dh.view(shp), gw, gb, gcw, gcb


class AddPEFn(torch.autograd.Function):
    """xscale * x + alpha * pe[:T]: the absolute positional encodings as an encoder embed (espnet PositionalEncoding: xscale =
    sqrt(d), no alpha; ScaledPositionalEncoding: xscale = 1, ``alpha`` the learnable scalar, read on the device)."""

    @staticmethod
    def forward(ctx, x, alpha, pe, xscale):
        ctx.pe, ctx.xscale, ctx.has_alpha = pe, xscale, alpha is not None
        return ops.add_pe(x, pe, alpha, xscale)

    @staticmethod
    @guarded
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = dy if ctx.xscale == 1.0 else ops.axpby(dy, None, ctx.xscale, 0.0)
        da = ops.add_pe_dalpha(dy, ctx.pe).view(()) if ctx.has_alpha and ctx.needs_input_grad[1] else None
        return dx, da, None, None


class DropoutFn(torch.autograd.Function):
    """stand-alone dropout node (positional-encoding dropouts, src/ctc/ctc.py:143)."""

    @staticmethod
    def forward(ctx, x, p):
        y, ctx.tok = ops.dropout(x.contiguous(), p)
        return y

    @staticmethod
    @guarded
    def backward(ctx, dy):
        return ops.dropout(dy.contiguous(), ctx.tok[0], token=ctx.tok)[0], None


class LinearFn(torch.autograd.Function):
    """y = alpha * (x W^T + b)."""

    @staticmethod
    def forward(ctx, x, w, b, alpha):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        y = ops.linear(x2, w, b, alpha=alpha)
        ctx.save_for_backward(x2, w)
        ctx.alpha, ctx.has_b = alpha, b is not None
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    @guarded
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(x2.shape[0], w.shape[0])
        dx = ops.linear_dx(dy2, w, alpha=ctx.alpha) if ctx.needs_input_grad[0] else None
        if ctx.has_b:
            gw, gb = ops.linear_dw(dy2, x2, alpha=ctx.alpha, bias_grad=True)
        else:
            gw, gb = ops.linear_dw(dy2, x2, alpha=ctx.alpha), None
        return (None if dx is None else dx.view(*dy.shape[:-1], w.shape[1])), gw, gb, None


# ------------------------------------------------------------------------------------------------
# Conv2dSubsampling (espnet subsampling.py; encoder.py:149-155,364): conv-relu-conv-relu-linear, x sqrt(d)
# ------------------------------------------------------------------------------------------------
CONV2_IMPLICIT = True      # Conv2dSubsampling's second convolution without im2col (shapes it does not take: im2col + GEMM)


class Conv2dSubsamplingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wo, bo, xscale):
        B, T, F = x.shape
        Cn = w1.shape[0]
        if CONV2_IMPLICIT and ops.BLOCKS_C and ops.conv2d_subsample_ok(x, w1, wo):      # the whole module as one C call
            out, T2, F2, kept, desc = ops.conv2d_subsample_fwd(x, w1.contiguous(), b1, w2.contiguous(), b2, wo.contiguous(), bo, xscale)
            ctx.cdesc, ctx.ckept, ctx.cparams = desc, kept, (w1, b1, w2, b2, wo, bo)
            ctx.save_for_backward()
            ctx.dims = (B, T, F, Cn, T2, F2, xscale, w1.shape, w2.shape, wo.shape)
            return out.view(B, T2, -1)
        ctx.cdesc, ctx.cparams = None, (w1, b1, w2, b2, wo, bo)
        y1 = ops.conv1_fwd(x.contiguous(), w1.reshape(Cn, 9), b1)              # [B,T1,F1,C] NHWC, relu
        # torch (co, ci, kh, kw) -> (co, kh, kw, ci) to match the channels-last patch order
        w2r = ops.transpose_inner(w2, Cn, Cn, 9).view(Cn, 9 * Cn)
        T1, F1 = y1.shape[1], y1.shape[2]
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        if CONV2_IMPLICIT and Cn % 64 == 0 and (B * T2 * F2) % 32 == 0:        # image rows as the GEMM operand: no patch matrix
            col = None
            y2 = ops.conv3x3_fwd(y1.view(B * T1 * F1, Cn), w2r, T1, F1, stride=2, pad0=True, bias=b2, act="relu")
        else:
            col, T2, F2 = ops.im2col3x3s2(y1)                                  # [B*T2*F2, 9C]
            y2 = ops.linear(col, w2r, b2, act="relu")                          # [B*T2*F2, C] == (b,t,f,c)
        # out Linear consumes (c*F2 + f); re-index its weight to (f*C + c) instead of transposing activations
        wor = ops.transpose_inner(wo, wo.shape[0], Cn, F2).view(wo.shape[0], F2 * Cn)
        out = ops.linear(y2.view(B * T2, F2 * Cn), wor, bo, alpha=xscale)
        ctx.save_for_backward(x, y1, col, y2, w2r, wor)      # col is None on the implicit route
        ctx.dims = (B, T, F, Cn, T2, F2, xscale, w1.shape, w2.shape, wo.shape)
        return out.view(B, T2, -1)

    @staticmethod
    @guarded
    def backward(ctx, dout):
        B, T, F, Cn, T2, F2, xscale, w1s, w2s, wos = ctx.dims
        do = dout.contiguous().view(B * T2, -1)
        if ctx.cdesc is not None:
            gw1, gb1, gw2, gb2, gwo, gbo = ops.conv2d_subsample_bwd(ctx.cdesc, do, (w1s, w2s, wos), params=ctx.cparams, kept=ctx.ckept)
            ctx.cdesc = ctx.ckept = ctx.cparams = None
            return None, gw1, gb1, gw2, gb2, gwo, gbo, None
        x, y1, col, y2, w2r, wor = ctx.saved_tensors
        y2f = y2.view(B * T2, F2 * Cn)
        # dz2 = (do @ wor) * xscale * relu'(y2)
        dz2 = ops.linear_dx(do, wor, alpha=xscale, DZ=y2f, dact="relu").view(B * T2 * F2, Cn)
        res = {}

        def wgrads():
            gwor, res["gbo"] = ops.linear_dw(do, y2f, alpha=xscale, bias_grad=True)        # [odim, F2*C], [odim]
            if col is None:
                gw2r, res["gb2"] = ops.conv3x3_dw(dz2, y1.view(-1, Cn), y1.shape[1], y1.shape[2], stride=2, pad0=True, bias_grad=True)
            else:
                gw2r, res["gb2"] = ops.linear_dw(dz2, col, bias_grad=True)                 # [C, 9C], [C]
            res["gwo"] = ops.transpose_inner(gwor, wos[0], F2, Cn).view(wos)
            res["gw2"] = ops.transpose_inner(gw2r, Cn, 9, Cn).view(w2s)

        ops.wgrad_beside(wgrads) if ops.wgrad_may_go_beside(ctx.cparams) else wgrads()      # (as the C-side block: beside the dgrad chain)
        dcol = ops.linear_dx(dz2, w2r)                                          # [B*T2*F2, 9C]
        dz1 = ops.col2im3x3s2_relu(dcol, y1)
        gw1, gb1 = ops.conv1_bwd(dz1, x.contiguous(), Cn)
        return None, gw1.view(w1s), gb1, res["gw2"], res["gb2"], res["gwo"], res["gbo"], None


# ------------------------------------------------------------------------------------------------
# CTC loss (src/ctc/ctc.py:133-158): Linear -> log_softmax -> CTCLoss(none, zero_infinity) -> sum/B
# ------------------------------------------------------------------------------------------------
class CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hs, w, b, hlens, ys, ylens, reduce, zero_infinity):
        B, T, D = hs.shape
        x2 = hs.reshape(B * T, D)
        logits = ops.linear(x2, w, b).view(B, T, -1)
        nll, g = ops.ctc_loss(logits, hlens, ys, ylens, 0, zero_infinity)
        ctx.save_for_backward(x2, w, g)
        ctx.reduce, ctx.B = reduce, B
        if reduce:
            return ops.colsum(nll.view(B, 1), scale=1.0 / B).view(())   # loss.sum() / B  (ctc.py:64-66)
        return ops.axpby(nll, None, 1.0 / B, 0.0)

    @staticmethod
    @guarded
    def backward(ctx, dl):
        x2, w, g = ctx.saved_tensors
        B = ctx.B
        V = w.shape[0]
        g2 = g.view(-1, V)
        if not ctx.reduce:
            raise NotImplementedError("reduce=False backward is not on the shipped path")
        gs = ops.scale_dev(g2, dl.contiguous(), 1.0 / B)   # dlogits = g * dl / B, dl stays on the device
        dx = ops.linear_dx(gs, w)
        gw, gb = ops.linear_dw(gs, x2, bias_grad=True)
        return dx.view(B, -1, x2.shape[1]), gw, gb, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# Transformer decoder, teacher forced (espnet2 TransformerDecoder.forward + DecoderLayer.forward,
# called at src/models/espnet_model.py:557-560).  The whole stack is ONE autograd node so the six
# per-layer gradients w.r.t. the encoder memory are accumulated in GEMM epilogues.
# ------------------------------------------------------------------------------------------------
DEC_LAYER_PARAM_NAMES = (
    "norm1.weight", "norm1.bias",
    "self_attn.linear_q.weight", "self_attn.linear_q.bias", "self_attn.linear_k.weight", "self_attn.linear_k.bias",
    "self_attn.linear_v.weight", "self_attn.linear_v.bias", "self_attn.linear_out.weight", "self_attn.linear_out.bias",
    "norm2.weight", "norm2.bias",
    "src_attn.linear_q.weight", "src_attn.linear_q.bias", "src_attn.linear_k.weight", "src_attn.linear_k.bias",
    "src_attn.linear_v.weight", "src_attn.linear_v.bias", "src_attn.linear_out.weight", "src_attn.linear_out.bias",
    "norm3.weight", "norm3.bias",
    "feed_forward.w_1.weight", "feed_forward.w_1.bias", "feed_forward.w_2.weight", "feed_forward.w_2.bias",
)
_NL = len(DEC_LAYER_PARAM_NAMES)
_DI = {n: i for i, n in enumerate(DEC_LAYER_PARAM_NAMES)}


class TransformerDecoderFn(torch.autograd.Function):
    """P = [embed.0.weight, (26 per layer) x num_blocks, after_norm.weight, after_norm.bias,
    output_layer.weight, output_layer.bias];  returns logits [B, L, V]."""

    @staticmethod
    def project_memory(mem2, nb, D, P):
        """kv_all [B T, nb * 2 D]: layer li's source-attention keys at columns 2 li D, values at (2 li + 1) D"""
        kv_all = ops.empty(mem2.shape[0], nb * 2 * D, like=mem2)
        kvp = [(P[1 + li * _NL + _DI[f"src_attn.linear_{c}.weight"]], P[1 + li * _NL + _DI[f"src_attn.linear_{c}.bias"]], (2 * li + j) * D)
               for li in range(nb) for j, c in enumerate("kv")]
        for i in range(0, len(kvp), 12):
            ops.linear_group(mem2, kvp[i: i + 12], kv_all)
        return kv_all

    @staticmethod
    def forward(ctx, memory, hlens, ys_in, ys_lens, pe, cfg, *P):
        need = _note_ctx(ctx)
        B, T, D = memory.shape
        L = ys_in.shape[1]
        H = cfg["heads"]
        dk = D // H
        nb = cfg["num_blocks"]
        M = B * L
        mem2 = memory.reshape(B * T, D)
        emb_w = P[0]
        pd, ppos, pself, psrc = (cfg.get(k, 0.0) for k in ("p", "p_pos", "p_self", "p_src"))
        causal = bool(cfg.get("causal", True))      # False: the MLM decoder's self-attention (key padding only, espnet2 mlm_decoder.py)
        memory_kv = cfg.get("memory_kv")             # the layers' key / value projections of the memory, computed by an earlier call
        if memory_kv is not None and need:
            raise NotImplementedError("memory_kv is the decoding path: no backward pass through a hoisted projection")
        x = ops.embed_pe(ys_in.contiguous(), emb_w, pe, math.sqrt(D)).view(M, D)
        t_pos = _drop_(x, ppos)                              # PositionalEncoding dropout
        saved = []
        # the key / value projections of the encoder memory do not depend on the decoder's state: all layers' in grouped launches up front
        # (2400 tiles of M = B T rows) instead of one 200-tile launch inside every layer's chain; layer li reads its window of kv_all
        ldkv = nb * 2 * D
        if memory_kv is not None:
            assert memory_kv.shape == (B * T, ldkv) and memory_kv.is_contiguous(), (memory_kv.shape, (B * T, ldkv))
            kv_all = memory_kv
        else:
            kv_all = TransformerDecoderFn.project_memory(mem2, nb, D, P)
        for li in range(nb):
            p = lambda n, li=li: P[1 + li * _NL + _DI[n]]
            s = {}
            # --- masked self attention
            n1, m1, r1 = ops.layernorm_fwd(x, p("norm1.weight"), p("norm1.bias"), EPS_ESPNET)
            qkv = ops.empty(M, 3 * D, like=x)
            ops.linear_group(n1, [(p(f"self_attn.linear_{c}.weight"), p(f"self_attn.linear_{c}.bias"), j * D)
                                  for j, c in enumerate("qkv")], qkv)
            fused = ops.ATTN_FUSED and dk == 64
            if fused:
                tk_a = "fused"
                cx, attn = _AttnFused.fwd(qkv, 0, qkv, D, qkv, 2 * D, B, L, L, H, dk, ys_lens, causal, p_att=pself)
            else:
                cx, attn, tk_a = _SelfAttnCore.fwd(qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, B, L, L, H, dk, ys_lens, causal,
                                                   p_att=pself)
            x1, tk_r = ops.linear_drop(cx, p("self_attn.linear_out.weight"), p("self_attn.linear_out.bias"), pd, res=x)   # x + dropout(self_attn(...))
            s["self"] = (x, m1, r1, n1, qkv, cx, attn, tk_a, tk_r)
            # --- source attention over the encoder memory
            n2, m2, r2 = ops.layernorm_fwd(x1, p("norm2.weight"), p("norm2.bias"), EPS_ESPNET)
            q2 = ops.linear(n2, p("src_attn.linear_q.weight"), p("src_attn.linear_q.bias"))
            ko = 2 * li * D
            if fused:
                tk_a2 = "fused"
                cx2, attn2 = _AttnFused.fwd(q2, 0, kv_all, ko, kv_all, ko + D, B, L, T, H, dk, hlens, False, p_att=psrc)
            else:
                cx2, attn2, tk_a2 = _SelfAttnCore.fwd(q2, D, 0, kv_all, ldkv, ko, kv_all, ldkv, ko + D, B, L, T, H, dk, hlens, False,
                                                      p_att=psrc)
            x2, tk_r2 = ops.linear_drop(cx2, p("src_attn.linear_out.weight"), p("src_attn.linear_out.bias"), pd, res=x1)   # x + dropout(src_attn(...))
            s["src"] = (x1, m2, r2, n2, q2, ko, cx2, attn2, tk_a2, tk_r2)
            # --- position-wise FFN (ReLU, scale 1)
            x, s["ff"] = _FFN.fwd(x2, p("norm3.weight"), p("norm3.bias"), p("feed_forward.w_1.weight"),
                                  p("feed_forward.w_1.bias"), p("feed_forward.w_2.weight"), p("feed_forward.w_2.bias"),
                                  "relu", 1.0, p=pd, save=need)
            saved.append(s)
        an_w, an_b, out_w, out_b = P[1 + nb * _NL: 1 + nb * _NL + 4]
        xn, mf, rf = ops.layernorm_fwd(x, an_w, an_b, EPS_ESPNET)
        logits = ops.linear(xn, out_w, out_b)
        ctx.saved, ctx.final, ctx.t_pos = saved, (x, mf, rf, xn), t_pos
        ctx.P, ctx.cfg, ctx.dims = P, cfg, (B, T, L, D, H, dk, nb)
        ctx.mem2, ctx.ys_in, ctx.hlens, ctx.ys_lens, ctx.kv_all = mem2, ys_in, hlens, ys_lens, kv_all
        return logits.view(B, L, -1)

    @staticmethod
    @guarded
    def backward(ctx, dlogits):
        P = ctx.P
        B, T, L, D, H, dk, nb = ctx.dims
        M = B * L
        G: List[Optional[torch.Tensor]] = [None] * len(P)
        an_i = 1 + nb * _NL
        an_w, an_b, out_w, out_b = P[an_i: an_i + 4]
        x, mf, rf, xn = ctx.final
        dl = dlogits.contiguous().view(M, -1)
        G[an_i + 2], G[an_i + 3] = ops.linear_dw(dl, xn, bias_grad=True)
        dxn = ops.linear_dx(dl, out_w)
        lng = ops.LNGroup(cap=3 * nb + 1)     # all LayerNorms of the decoder: one (dgamma, dbeta) reduction at the end
        # (every LayerNorm backward also writes its dx under the mask of the residual block below it: no dropout launches)
        dx, G[an_i], G[an_i + 1], *dyd = lng.bwd(dxn, x, mf, rf, an_w, drop=ctx.saved[nb - 1]["ff"][-1])
        mem2, kv_all = ctx.mem2, ctx.kv_all
        ldkv = nb * 2 * D
        dkv_all = torch.empty_like(kv_all)      # every layer's (dK | dV) side by side: the memory's gradient is ONE K = 2 D nb GEMM at the end
        # the weight gradients of ALL layers in a few grouped launches at the end: a layer's own group is 384 tiles of K = 1312 (1.5 per compute
        # unit, 42 TFLOP/s, 95 us of the 280 a layer's backward takes); 2304 tiles together run at the rate of the encoder's groups
        grp = ops.WgradGroup()
        beside = ops.wgrad_may_go_beside(P)
        for li in reversed(range(nb)):
            base = 1 + li * _NL
            p = lambda n, base=base: P[base + _DI[n]]

            def put(n, g, base=base):
                G[base + _DI[n]] = g

            s = ctx.saved[li]
            dx2, gs, *dt2 = _FFN.bwd(dx, s["ff"], p("norm3.weight"), p("feed_forward.w_1.weight"), p("feed_forward.w_2.weight"),
                                     "relu", 1.0, grp=grp, lng=lng, dyd=dyd[0] if dyd else None, out_drop=s["src"][-1])
            for n_, g in zip(("norm3.weight", "norm3.bias", "feed_forward.w_1.weight", "feed_forward.w_1.bias",
                              "feed_forward.w_2.weight", "feed_forward.w_2.bias"), gs):
                put(n_, g)
            # --- source attention
            x1, m2, r2, n2, q2, ko, cx2, attn2, tk_a2, tk_r2 = s["src"]
            dt2 = dt2[0] if dt2 else _drop_bwd(dx2, tk_r2)
            gw_, gb_ = grp.add(dt2, cx2, bias_grad=True)
            put("src_attn.linear_out.weight", gw_); put("src_attn.linear_out.bias", gb_)
            dcx2 = ops.linear_dx(dt2, p("src_attn.linear_out.weight"))
            dq2 = ops.empty(M, D, like=dl)
            if tk_a2 == "fused":
                _AttnFused.bwd(dcx2, cx2, attn2, q2, 0, kv_all, ko, kv_all, ko + D, dq2, 0, dkv_all, ko, dkv_all, ko + D, B, L, T, H, dk,
                               ctx.hlens, False)
            else:
                _SelfAttnCore.bwd(dcx2, attn2, q2, D, 0, kv_all, ldkv, ko, kv_all, ldkv, ko + D, dq2, D, 0, dkv_all, ldkv, ko,
                                  dkv_all, ldkv, ko + D, B, L, T, H, dk, tok=tk_a2)
            gw_, gb_ = grp.add(dq2, n2, bias_grad=True)
            put("src_attn.linear_q.weight", gw_); put("src_attn.linear_q.bias", gb_)
            for j, nm in enumerate(("k", "v")):
                gw_, gb_ = grp.add(dkv_all[:, ko + j * D: ko + (j + 1) * D], mem2, bias_grad=True)
                put(f"src_attn.linear_{nm}.weight", gw_); put(f"src_attn.linear_{nm}.bias", gb_)
            dn2 = ops.linear_dx(dq2, p("src_attn.linear_q.weight"))
            dx1, g1, g2, *dt1 = lng.bwd(dn2, x1, m2, r2, p("norm2.weight"), dx_add=dx2, drop=s["self"][-1])
            put("norm2.weight", g1); put("norm2.bias", g2)
            # --- self attention
            x0, m1, r1, n1, qkv, cx, attn, tk_a, tk_r = s["self"]
            dt1 = dt1[0] if dt1 else _drop_bwd(dx1, tk_r)
            gw_, gb_ = grp.add(dt1, cx, bias_grad=True)
            put("self_attn.linear_out.weight", gw_); put("self_attn.linear_out.bias", gb_)
            dcx = ops.linear_dx(dt1, p("self_attn.linear_out.weight"))
            dqkv = torch.empty_like(qkv)
            if tk_a == "fused":
                _AttnFused.bwd(dcx, cx, attn, qkv, 0, qkv, D, qkv, 2 * D, dqkv, 0, dqkv, D, dqkv, 2 * D, B, L, L, H, dk,
                               ctx.ys_lens, bool(ctx.cfg.get("causal", True)))
            else:
                _SelfAttnCore.bwd(dcx, attn, qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, dqkv, 3 * D, 0, dqkv, 3 * D, D,
                                  dqkv, 3 * D, 2 * D, B, L, L, H, dk, tok=tk_a)
            for j, nm in enumerate(("q", "k", "v")):
                gw_, gb_ = grp.add(dqkv[:, j * D:(j + 1) * D], n1, bias_grad=True)
                put(f"self_attn.linear_{nm}.weight", gw_); put(f"self_attn.linear_{nm}.bias", gb_)
            dn1 = ops.linear_dx_cat(dqkv, [p(f"self_attn.linear_{c}.weight") for c in "qkv"])
            dx, g1, g2, *dyd = lng.bwd(dn1, x0, m1, r1, p("norm1.weight"), dx_add=dx1,
                                       drop=ctx.saved[li - 1]["ff"][-1] if li else None)
            put("norm1.weight", g1); put("norm1.bias", g2)
            if beside and li and (nb - li) % _DEC_WGRAD == 0:
                ops.wgrad_beside(grp.flush)
        # (in the layers' chain it was an accumulating K = 2 D launch over B T rows per layer - the only launches of the chain over the memory's
        # rows rather than the 1312 token rows)
        dmem = ops.linear_dx_cat(dkv_all, [P[1 + li * _NL + _DI[f"src_attn.linear_{c}.weight"]] for li in range(nb) for c in "kv"])
        grp.flush()
        lng.flush()
        _drop_bwd_(dx, ctx.t_pos)
        G[0] = ops.embed_bwd(ctx.ys_in.contiguous(), dx, math.sqrt(D), P[0].shape[0])
        ctx.saved = ctx.kv_all = None
        return (dmem.view(B, T, D), None, None, None, None, None, *G)


_DEC_WGRAD = int(os.environ.get("TAVSR_DEC_WGRAD", "5"))     # layers between two flushes of the decoder's weight gradients (6: one flush at the end)


class LabelSmoothingLossFn(torch.autograd.Function):
    """espnet LabelSmoothingLoss (KL, sum / batch) on decoder logits; also yields the th_accuracy counters.
    ``count`` (optional, [n] int32 on the device; used with ``normalize_length``): the number of real target tokens as per-row
    counts that only the device knows (ops.mask_uniform's ``n_target``) - the loss is sum / max(1, sum(count)) with the
    reciprocal formed on the device in fp32, so nothing is read on the host and the step stays capturable."""

    @staticmethod
    def forward(ctx, logits, target, ignore, smoothing, normalize_length, count=None):
        B, L, V = logits.shape
        row, g, correct = ops.lsm_loss(logits.reshape(B * L, V), target.reshape(-1).contiguous(), ignore, smoothing)
        ctx.mark_non_differentiable(correct)
        if normalize_length and count is not None:
            inv = ops.count_recip(count)
            ctx.save_for_backward(g, inv)
            ctx.B, ctx.denom = B, None
            return ops.scale_dev(ops.colsum(row.view(-1, 1)), inv).view(()), correct
        denom = B
        if normalize_length:      # espnet LabelSmoothingLoss: sum / number of real target tokens (a host count, as espnet's .item())
            if logits.is_cuda and torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("length_normalized_loss=true reads the token count on the host: not capturable")
            denom = max(1, int((target != ignore).sum()))
        ctx.save_for_backward(g)
        ctx.B, ctx.denom = B, denom
        return ops.colsum(row.view(-1, 1), scale=1.0 / denom).view(()), correct

    @staticmethod
    @guarded
    def backward(ctx, dl, _dc):
        if ctx.denom is None:
            g, inv = ctx.saved_tensors
            s = ops.scale_dev(dl.reshape(1).contiguous(), inv)
            return ops.scale_dev(g, s).view(ctx.B, -1, g.shape[-1]), None, None, None, None, None
        (g,) = ctx.saved_tensors
        return ops.scale_dev(g, dl.contiguous(), 1.0 / ctx.denom).view(ctx.B, -1, g.shape[-1]), None, None, None, None, None


class WeightedSumFn(torch.autograd.Function):
    """loss = a*l1 + b*l2 on 0-dim device tensors (espnet_model.py:330)."""

    @staticmethod
    def forward(ctx, l1, l2, a, b):
        ctx.ab = (a, b)
        return ops.axpby(l1.reshape(1).contiguous(), l2.reshape(1).contiguous(), a, b).view(())

    @staticmethod
    @guarded
    def backward(ctx, dl):
        a, b = ctx.ab
        d = dl.reshape(1).contiguous()
        return ops.axpby(d, None, a, 0.0).view(()), ops.axpby(d, None, b, 0.0).view(()), None, None
