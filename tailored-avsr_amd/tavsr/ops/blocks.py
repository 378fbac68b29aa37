"""Encoder blocks: the streaming feed-forward block, cgMLP / CSGU, Conv2dSubsampling as C calls, depthwise convolutions,
the branch merge, and the element-wise helpers they share.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from .. import ops
from .._lib import ACT, check, lib, ptr, require_cuda, stream
from .base import _addr, _ptr_array, _zero_page, empty
from .rng import _new_token, dropout
from .streams import branch_events, branch_stream, forks_enabled, wgrad_may_go_beside, wgrad_open

__all__ = ["ffn2_usable", "ffn2_shape_ok", "ffn2_fwd", "DnSlabs", "ffn2_bwd_dx", "axpby", "scale_dev", "axpby2d", "act_bwd_",
           "dwconv_gate_fwd", "csgu_usable", "csgu_rowstat_ok", "csgu_fwd", "cgmlp_block_ok", "cgmlp_fwd", "cgmlp_bwd",
           "conv2d_subsample_ok", "conv2d_subsample_fwd", "conv2d_subsample_bwd", "dwconv_gate_bwd", "dwconv_add_ok", "dwconv_add_fwd",
           "dwconv_add_bwd", "glu_dwconv_ok", "glu_dwconv_fwd", "glu_dwconv_bwd", "merge_pool_fwd", "merge_rows_ok", "merge_fwd",
           "merge_proj_ok", "merge_proj_fwd", "merge_combine", "merge_bwd", "act_"]


def ffn2_usable(x, w1, act) -> bool:
    return ops.FFN2 and ffn2_shape_ok(x, w1, act)


def ffn2_shape_ok(x, w1, act) -> bool:
    return (x.dim() == 2 and x.shape[1] == 256 and w1.shape[0] >= 1024 and w1.shape[0] % 32 == 0
            and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and w1.is_contiguous()
            and act in ("relu", "swish", "tanh", "hardtanh", "selu"))


def ffn2_fwd(x, ln_w, ln_b, eps, w1, b1, w2, b2, act, scale, p=0.0, save=True, ln2=(), ln2_eps=1e-12, ln2_stats=False):
    """y = x + scale * dropout(w2 dropout(act(w1 LN(x) + b1)) + b2) and, for every (gamma, beta) in ``ln2`` (at most two),
    LayerNorm(y) * gamma + beta.  Returns (y, saved, ln2_outs, (ln2_mean, ln2_rstd)) with saved = (n, mean, rstd, z, h,
    tok_in, tok_out) as the GEMM path keeps it (None entries when ``save`` is false): the dropout masks are the ones the GEMM
    epilogues would draw, so the GEMM-based backward pairs with this forward."""
    from .._lib import FfnDesc
    M, D = x.shape
    N1 = w1.shape[0]
    require_cuda(x, ln_w, ln_b, w1, b1, w2, b2)
    assert w1.is_contiguous() and w2.is_contiguous() and w1.shape == (N1, D) and w2.shape == (D, N1) and len(ln2) <= 2
    d = FfnDesc()
    d.M, d.D, d.N1, d.act, d.scale, d.eps = M, D, N1, ACT[act], scale, eps
    d.x, d.ldx = _addr(x), x.stride(0)
    d.ln_w, d.ln_b, d.w1, d.b1, d.w2, d.b2 = (_addr(t) for t in (ln_w, ln_b, w1, b1, w2, b2))
    y = empty(M, D, like=x)
    d.y = _addr(y)
    n = mean = rstd = z = h = None
    if save:
        n, mean, rstd = empty(M, D, like=x), empty(M, like=x), empty(M, like=x)
        Mp = (M + 127) // 128 * 128       # whole 128-row blocks are stored
        z, h = empty(Mp, N1, like=x)[:M], empty(Mp, N1, like=x)[:M]
        d.n_out, d.mean, d.rstd, d.z, d.h = (_addr(t) for t in (n, mean, rstd, z, h))
    tok_in = tok_out = None
    if p and p > 0.0:
        tok_in = _new_token(p, M * N1, x.device)
        tok_out = _new_token(p, M * D, x.device)
        d.p_drop, d.seed, d.offset_in, d.offset_out = p, _addr(tok_in[2]), tok_in[1], tok_out[1]
    outs = []
    for k, (g, b) in enumerate(ln2):
        o = empty(M, D, like=x)
        outs.append(o)
        d.ln2_w[k], d.ln2_b[k], d.ln2_out[k] = _addr(g), _addr(b), _addr(o)
    m2 = r2 = None
    if ln2 and ln2_stats:
        m2, r2 = empty(M, like=x), empty(M, like=x)
        d.ln2_mean, d.ln2_rstd = _addr(m2), _addr(r2)
    d.ln2_eps = ln2_eps
    nws = lib().tavsr_ffn2_ws(M, D, N1)
    ws = empty(nws, like=x)
    d.ws, d.ws_floats = _addr(ws), nws
    check(lib().tavsr_ffn2_fwd(C.byref(d), stream()), "tavsr_ffn2_fwd")
    return y, (n, mean, rstd, z, h, tok_in, tok_out), outs, (m2, r2)


class DnSlabs:
    """dn of ``ffn2_bwd_dx(..., sum_dn=False)``: the unsummed partials in the launch's workspace (tavsr_ffn2_slab_layout)"""
    __slots__ = ("ws", "wpb", "rb", "shape")

    def __init__(self, ws, wpb, rb, shape):
        self.ws, self.wpb, self.rb, self.shape = ws, wpb, rb, shape


def ffn2_bwd_dx(dyd, alpha, w1, w2, z, act, tok_in, sum_dn=True):
    """(dz [M, N1], dn [M, 256]) of the block: dz = ((alpha * dyd) w2) * mask / keep * act'(z), dn = dz w1 - the streaming
    counterpart of linear_dx_drop + linear_dx (weights untransposed).  ``sum_dn`` False: dn comes back as ``DnSlabs`` for
    ``LNGroup.bwd``, which sums the partials where it reads the rows."""
    M, D = dyd.shape
    N1 = w1.shape[0]
    require_cuda(dyd, w1, w2, z)
    assert w1.is_contiguous() and w2.is_contiguous() and z.is_contiguous() and z.shape == (M, N1)
    dz = empty((M + 127) // 128 * 128, N1, like=dyd)[:M]
    dn = empty(M, D, like=dyd) if sum_dn else None
    nws = lib().tavsr_ffn2_ws(M, D, N1)
    ws = empty(nws, like=dyd)
    check(lib().tavsr_ffn2_bwd_dx(ptr(dyd), dyd.stride(0), alpha, ptr(w1), ptr(w2), ptr(z), ACT[act], M, D, N1,
                                  tok_in[0] if tok_in else 0.0, ptr(tok_in[2] if tok_in else None), tok_in[1] if tok_in else 0, ptr(dz),
                                  ptr(dn), ptr(ws), nws, stream()), "tavsr_ffn2_bwd_dx")
    if sum_dn:
        return dz, dn
    lay = _SLAB_LAYOUT.get((M, N1))
    if lay is None:
        wpb, rb = C.c_int32(0), C.c_int32(0)
        check(lib().tavsr_ffn2_slab_layout(M, N1, C.byref(wpb), C.byref(rb)), "tavsr_ffn2_slab_layout")
        lay = _SLAB_LAYOUT[(M, N1)] = (wpb.value, rb.value)
    return dz, DnSlabs(ws, lay[0], lay[1], (M, D))


_SLAB_LAYOUT = {}


def axpby(x, y=None, a=1.0, b=1.0, out=None):
    if out is None:
        out = torch.empty_like(x)
    assert x.is_contiguous() and (y is None or y.is_contiguous()) and out.is_contiguous()
    require_cuda(x, y, out)
    check(lib().tavsr_axpby(ptr(x), ptr(y), a, b, ptr(out), x.numel(), stream()), "tavsr_axpby")
    return out


def scale_dev(x, s, c=1.0):
    """x * (c * s) with ``s`` a 0-dim / 1-element device tensor."""
    require_cuda(x, s)
    assert x.is_contiguous()
    out = torch.empty_like(x)
    check(lib().tavsr_scale_dev(ptr(x), ptr(s), c, ptr(out), x.numel(), stream()), "tavsr_scale_dev")
    return out


def axpby2d(x, y, a, b, out):
    M, N = x.shape
    require_cuda(x, y, out)
    check(lib().tavsr_axpby2d(ptr(x), x.stride(0), ptr(y), 0 if y is None else y.stride(0), a, b, ptr(out), out.stride(0), M, N, stream()),
          "tavsr_axpby2d")
    return out


def act_bwd_(dh, z, act):
    """in place: dh *= act'(z)."""
    assert dh.is_contiguous() and z.is_contiguous()
    check(lib().tavsr_act_bwd(ptr(dh), ptr(z), ptr(dh), dh.numel(), ACT[act], stream()), "tavsr_act_bwd")
    return dh


# ---------------------------------------------------------------------------------------------- cgMLP / merge
def dwconv_gate_fwd(gn, r, w, bias, B, T):
    M, Cn = gn.shape
    K = w.shape[-1]
    out, conv = empty(M, Cn, like=gn), empty(M, Cn, like=gn)
    require_cuda(gn, r, w, bias)
    check(lib().tavsr_dwconv_gate_fwd(ptr(gn), ptr(r), r.stride(0), ptr(w), ptr(bias), ptr(out), ptr(conv), B, T, Cn, K, stream()),
          "tavsr_dwconv_gate_fwd")
    return out, conv


def csgu_usable(g, w) -> bool:
    return (ops.CSGU_FUSED and w.shape[-1] == 31 and g.shape[1] % 128 == 0 and g.is_contiguous() and g.data_ptr() % 16 == 0)


def csgu_rowstat_ok(x, w1) -> bool:
    """can channel_proj1's GEMM leave the CSGU's LayerNorm statistics (tavsr_gemm_desc.rowstat)?  (16-byte path, gate half of
    at most 1024 channels in whole 64-column tiles)"""
    return (ops.CSGU_STATS_IN_GEMM and ops.PROFILE is None 
            and w1.is_contiguous() and w1.shape[0] % 128 == 0 and w1.shape[0] <= 2048
            and x.shape[1] % 32 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def csgu_fwd(g, ln_w, ln_b, eps, w, bias, B, T, p=0.0, save=True, rowstat=None):
    """dropout(g[:, :C] * dwconv(LayerNorm(g[:, C:]))) in one pass over g (+ the statistics launch, unless ``rowstat`` - the
    row statistics the GEMM that produced g left, ops.linear(..., rowstat=) - is given).  Returns
    (u, conv, gn, mean, rstd, token); conv / gn only when ``save``."""
    M, C2 = g.shape
    Cn = C2 // 2
    require_cuda(g, ln_w, ln_b, w, bias)
    out = empty(M, Cn, like=g)
    conv, gn = (empty(M, Cn, like=g), empty(M, Cn, like=g)) if save else (None, None)
    mean, rstd = empty(M, like=g), empty(M, like=g)
    tok = _new_token(p, M * Cn, g.device) if p and p > 0.0 else None
    check(lib().tavsr_csgu_fwd(ptr(g), g.stride(0), ptr(ln_w), ptr(ln_b), eps, ptr(w), ptr(bias), ptr(out), ptr(gn), ptr(conv), ptr(mean),
                               ptr(rstd), tok[0] if tok else 0.0, ptr(tok[2] if tok else None), tok[1] if tok else 0, B, T, Cn, w.shape[-1],
                               ptr(rowstat), stream()), "tavsr_csgu_fwd")
    return out, conv, gn, mean, rstd, tok


def cgmlp_block_ok(x, w1, cw) -> bool:
    """the shapes tavsr_cgmlp_fwd sequences (kernel 31, C <= 1024, one-pass CSGU with the statistics from channel_proj1's epilogue)"""
    C2 = w1.shape[0]
    return (ops.PROFILE is None and ops.CSGU_FUSED and ops.CSGU_STATS_IN_GEMM and cw.shape[-1] == 31 and C2 % 128 == 0 and C2 // 2 <= 1024
            and x.is_contiguous() and x.shape[1] % 32 == 0 and w1.is_contiguous() and cw.is_contiguous())


def cgmlp_fwd(x, w1, b1, ln_w, ln_b, cw, cb, w2, b2, B, T, *, p=0.0, p_out=0.0, alpha=1.0, res=None, save=True):
    """espnet ConvolutionalGatingMLP with the branch's dropout / residual around it as ONE C call (tavsr_cgmlp_fwd, csrc/blocks.hip):
    -> (out, (g, z, gn, gmean, grstd, u, conv, t_u, t_out), desc); ``desc`` is what ``cgmlp_bwd`` wants back."""
    M, D = x.shape
    C2 = w1.shape[0]
    Cn = C2 // 2
    require_cuda(x, res, w1, b1, ln_w, ln_b, cw, cb, w2, b2)
    d = L.CgmlpDesc()
    d.B, d.T, d.D, d.units, d.kernel, d.save = B, T, D, C2, cw.shape[-1], int(save)
    t_u = _new_token(p, M * Cn, x.device) if p and p > 0.0 else None
    t_out = _new_token(p_out, M * D, x.device) if p_out and p_out > 0.0 else None
    d.p_drop, d.p_out, d.alpha = (p if t_u else 0.0), (p_out if t_out else 0.0), alpha
    seed = (t_u or t_out or (0.0, 0, None))[2]
    d.seed, d.off_u, d.off_out = _addr(seed), (t_u[1] if t_u else 0), (t_out[1] if t_out else 0)
    g, u, out = empty(M, C2, like=x), empty(M, Cn, like=x), empty(M, D, like=x)
    gmean, grstd = empty(M, like=x), empty(M, like=x)
    z = gn = conv = None
    if save:
        z, gn, conv = empty(M, C2, like=x), empty(M, Cn, like=x), empty(M, Cn, like=x)
    for f, t in (("x", x), ("res", res), ("w1", w1), ("b1", b1), ("ln_w", ln_w), ("ln_b", ln_b), ("cw", cw), ("cb", cb), ("w2", w2),
                 ("b2", b2), ("g", g), ("g_z", z), ("gn", gn), ("g_mean", gmean), ("g_rstd", grstd), ("u", u), ("conv", conv), ("out", out)):
        setattr(d, f, _addr(t))
    nws = lib().tavsr_cgmlp_ws(C.byref(d))
    ws = empty(max(nws, 4), like=x)
    d.ws, d.ws_floats = _addr(ws), nws
    check(lib().tavsr_cgmlp_fwd(C.byref(d), stream()), "tavsr_cgmlp_fwd")
    return out, (g, z, gn, gmean, grstd, u, conv, t_u, t_out), d


def cgmlp_bwd(desc, dy, params):
    """backward of ``cgmlp_fwd`` (its descriptor; the caller keeps the forward's tensors alive): -> (dx, (g_w1, g_b1, g_ln_w, g_ln_b,
    g_cw, g_cb, g_w2, g_b2)); ``params`` = the eight parameters in that order (shapes of the gradients)."""
    M, D = dy.shape
    require_cuda(dy)
    b = L.CgmlpBwdDesc()
    b.fwd = C.pointer(desc)
    dx = empty(M, D, like=dy)
    grads = [torch.empty_like(q, memory_format=torch.contiguous_format) for q in params]
    b.dy, b.dx = _addr(dy), _addr(dx)
    for f, t in zip(("g_w1", "g_b1", "g_ln_w", "g_ln_b", "g_cw", "g_cb", "g_w2", "g_b2"), grads):
        setattr(b, f, _addr(t))
    nws = lib().tavsr_cgmlp_bwd_ws(C.byref(b))
    ws = empty(max(nws, 4), like=dy)
    b.ws, b.ws_floats = _addr(ws), nws
    check(lib().tavsr_cgmlp_bwd(C.byref(b), stream()), "tavsr_cgmlp_bwd")
    return dx, grads


def conv2d_subsample_ok(x, w1, wo) -> bool:
    B, T, F = x.shape
    Cn = w1.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    return ops.PROFILE is None and T >= 7 and F >= 7 and Cn % 64 == 0 and (B * T2 * F2) % 32 == 0 and wo.shape[0] % 4 == 0


def conv2d_subsample_fwd(x, w1, b1, w2, b2, wo, bo, xscale):
    """espnet Conv2dSubsampling as ONE C call (tavsr_conv2d_subsample_fwd): -> (out [B*T2, odim], T2, F2, kept tensors, desc)"""
    B, T, F = x.shape
    Cn, odim = w1.shape[0], wo.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    x = x.contiguous()
    require_cuda(x, w1, b1, w2, b2, wo, bo)
    assert all(t.is_contiguous() for t in (w1, w2, wo))
    d = L.SubsampleDesc()
    d.B, d.T, d.F, d.C, d.odim, d.xscale = B, T, F, Cn, odim, xscale
    y1, y2 = empty(B, T1, F1, Cn, like=x), empty(B * T2 * F2, Cn, like=x)
    w2r, wor, out = empty(Cn, 9 * Cn, like=x), empty(odim, F2 * Cn, like=x), empty(B * T2, odim, like=x)
    for f, t in (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("wo", wo), ("bo", bo), ("zero_page", _zero_page(x.device)),
                 ("y1", y1), ("y2", y2), ("w2r", w2r), ("wor", wor), ("out", out)):
        setattr(d, f, _addr(t))
    nws = lib().tavsr_conv2d_subsample_ws(C.byref(d))
    ws = empty(max(nws, 4), like=x)
    d.ws, d.ws_floats = _addr(ws), nws
    check(lib().tavsr_conv2d_subsample_fwd(C.byref(d), stream()), "tavsr_conv2d_subsample_fwd")
    return out, T2, F2, (x, y1, y2, w2r, wor), d


def conv2d_subsample_bwd(desc, dout, shapes, params=None, kept=()):
    """-> (g_w1, g_b1, g_w2, g_b2, g_wo, g_bo) in the torch layouts ``shapes`` = (w1, w2, wo shapes).  ``params`` (the module's six
    parameters) + ``kept`` (the forward's buffers): the weight gradients may run on the side queue, un-joined (``wgrad_may_go_beside``)."""
    require_cuda(dout)
    w1s, w2s, wos = shapes
    b = L.SubsampleBwdDesc()
    b.fwd = C.pointer(desc)
    grads = [empty(*w1s, like=dout), empty(w1s[0], like=dout), empty(*w2s, like=dout), empty(w2s[0], like=dout),
             empty(*wos, like=dout), empty(wos[0], like=dout)]
    b.dout = _addr(dout)
    for f, t in zip(("g_w1", "g_b1", "g_w2", "g_b2", "g_wo", "g_bo"), grads):
        setattr(b, f, _addr(t))
    nws = lib().tavsr_conv2d_subsample_bwd_ws(C.byref(b))
    ws = empty(max(nws, 4), like=dout)
    b.ws, b.ws_floats = _addr(ws), nws
    main = torch.cuda.current_stream()
    side = branch_stream(main) if (params is not None and forks_enabled() and ops.WGRAD_SLOT == 0) else None
    beside = side is not None and wgrad_may_go_beside(params) and wgrad_open(main, side)
    if beside:
        b.wgrad_beside, b.stream2, b.ev_fork = 1, side.cuda_stream, branch_events(main)[0].cuda_event
    check(lib().tavsr_conv2d_subsample_bwd(C.byref(b), stream()), "tavsr_conv2d_subsample_bwd")
    if beside:      # what the side queue's launches read and write is freed on THIS stream (rule 1 of _lib.py, by hand)
        for t in (ws, dout, *grads, *kept):
            if torch.is_tensor(t) and not isinstance(t, torch.nn.Parameter):
                t.record_stream(side)
    return grads


def dwconv_gate_bwd(du, gn, r, conv, w, dr, B, T, zr=None, act="gelu"):
    """``zr`` (kernel size 31): r = act(zr); dr comes back as the gradient w.r.t. zr."""
    M, Cn = gn.shape
    K = w.shape[-1]
    dgn = empty(M, Cn, like=gn)
    dw, db = torch.empty_like(w), empty(Cn, like=gn)
    ws = empty(lib().tavsr_dwconv_gate_bwd_ws(B, T, Cn, K), like=gn)
    if zr is not None:
        require_cuda(du, gn, r, conv, w, dr, zr)
        check(lib().tavsr_dwconv_gate_bwd_act(ptr(du), ptr(gn), ptr(r), r.stride(0), ptr(conv), ptr(w), ptr(dr), dr.stride(0), ptr(dgn),
                                              ptr(dw), ptr(db), 0, ptr(ws), B, T, Cn, K, ptr(zr), zr.stride(0), ACT[act], stream()),
              "tavsr_dwconv_gate_bwd_act")
        return dgn, dw, db
    check(lib().tavsr_dwconv_gate_bwd(ptr(du), ptr(gn), ptr(r), r.stride(0), ptr(conv), ptr(w), ptr(dr), dr.stride(0), ptr(dgn), ptr(dw),
                                      ptr(db), 0, ptr(ws), B, T, Cn, K, stream()), "tavsr_dwconv_gate_bwd")
    return dgn, dw, db


def dwconv_add_ok(B, T, Cn, K) -> bool:
    return bool(lib().tavsr_dwconv_add_ok(B, T, Cn, K))


def dwconv_add_fwd(x, w, bias, B, T, out=None):
    """u = x + depthwise_conv1d_K(x) over time (E-Branchformer's merge convolution): x [B*T, C] rows (any row stride),
    w [C, K], bias [C].  T is dense: no lengths.  Shapes the kernel does not take are an error (there is no other route)."""
    M, Cn = x.shape
    require_cuda(x, w, bias)
    assert M == B * T and x.stride(1) == 1 and w.is_contiguous()
    if out is None:
        out = empty(M, Cn, like=x)
    check(lib().tavsr_dwconv_add_fwd(ptr(x), x.stride(0), ptr(w), ptr(bias), ptr(out), out.stride(0), B, T, Cn, w.shape[-1], stream()),
          "tavsr_dwconv_add_fwd")
    return out


def dwconv_add_bwd(du, x, w, B, T, dx=None):
    """backward of dwconv_add_fwd -> (dx, dw [C, K], dbias [C]); dw / dbias are reduced in a fixed order (no atomics)."""
    M, Cn = x.shape
    K = w.shape[-1]
    require_cuda(du, x, w)
    assert M == B * T and du.shape == x.shape and du.stride(1) == 1 and x.stride(1) == 1 and w.is_contiguous()
    if dx is None:
        dx = empty(M, Cn, like=x)
    dw, db = empty(Cn, K, like=x), empty(Cn, like=x)
    ws = empty(max(1, lib().tavsr_dwconv_add_bwd_ws(B, T, Cn, K)), like=x)
    check(lib().tavsr_dwconv_add_bwd(ptr(du), du.stride(0), ptr(x), x.stride(0), ptr(w), ptr(dx), dx.stride(0), ptr(dw), ptr(db), 0,
                                     ptr(ws), B, T, Cn, K, stream()), "tavsr_dwconv_add_bwd")
    return dx, dw, db


def glu_dwconv_ok(B, T, Cn, K) -> bool:
    return bool(lib().tavsr_glu_dwconv_ok(B, T, Cn, K))


def glu_dwconv_fwd(h, w, bias, B, T, out=None):
    """z = depthwise_conv1d_K(glu(h)) over time (the Conformer convolution module between its pointwise convolutions):
    h [B*T, 2C] rows (any row stride), w [C, K], bias [C] -> z [B*T, C].  The gated rows are never stored.  T is dense: no
    lengths.  Shapes the kernel does not take are an error (there is no other route)."""
    M, C2 = h.shape
    Cn = w.shape[0]
    require_cuda(h, w, bias)
    assert M == B * T and C2 == 2 * Cn and h.stride(1) == 1 and w.is_contiguous()
    if out is None:
        out = empty(M, Cn, like=h)
    assert out.shape == (M, Cn) and out.stride(1) == 1
    check(lib().tavsr_glu_dwconv_fwd(ptr(h), h.stride(0), ptr(w), ptr(bias), ptr(out), out.stride(0), B, T, Cn, w.shape[-1], stream()),
          "tavsr_glu_dwconv_fwd")
    return out


def glu_dwconv_bwd(dz, h, w, B, T, dh=None):
    """backward of glu_dwconv_fwd -> (dh [B*T, 2C], dw [C, K], dbias [C]); the gated rows are recomputed from h, dw / dbias are
    reduced in a fixed order (no atomics)."""
    M, C2 = h.shape
    Cn, K = w.shape
    require_cuda(dz, h, w)
    assert M == B * T and C2 == 2 * Cn and dz.shape == (M, Cn) and dz.stride(1) == 1 and h.stride(1) == 1 and w.is_contiguous()
    if dh is None:
        dh = empty(M, C2, like=h)
    assert dh.shape == (M, C2) and dh.stride(1) == 1
    dw, db = empty(Cn, K, like=h), empty(Cn, like=h)
    ws = empty(max(1, lib().tavsr_glu_dwconv_bwd_ws(B, T, Cn, K)), like=h)
    check(lib().tavsr_glu_dwconv_bwd(ptr(dz), dz.stride(0), ptr(h), h.stride(0), ptr(w), ptr(dh), dh.stride(0), ptr(dw), ptr(db), ptr(ws),
                                     B, T, Cn, K, stream()), "tavsr_glu_dwconv_bwd")
    return dh, dw, db


def merge_pool_fwd(x1, x2, lens, params, B, T, lens2=None):
    D = x1.shape[-1]
    score, pooled, w = empty(2, B, T, like=x1), empty(2, B, D, like=x1), empty(B, 2, like=x1)
    require_cuda(x1, x2, lens, lens2)
    check(lib().tavsr_merge_pool_fwd(ptr(x1), ptr(x2), ptr(lens), ptr(lens2), _ptr_array(params), ptr(score), ptr(pooled), ptr(w),
                                     B, T, D, stream()), "tavsr_merge_pool_fwd")
    return score, pooled, w


def merge_rows_ok(T, D) -> bool:
    return ops.MERGE_ROWS and bool(lib().tavsr_merge_rows_ok(T, D))


def merge_fwd(x1, x2, lens, params, B, T, lens2=None):
    """merge_pool_fwd + merge_combine: (score, aux, w, w[:, 0] * x1 + w[:, 1] * x2); ``aux`` is what ``merge_bwd`` wants back
    with the other two: the pooled vectors [2, B, D] of the one-workgroup-per-utterance launches, or the row dot products
    [4, B*T] of the row-parallel ones (D = 256)."""
    D = x1.shape[-1]
    score, w = empty(2, B, T, like=x1), empty(B, 2, like=x1)
    out = torch.empty_like(x1)
    require_cuda(x1, x2, lens, lens2)
    assert x1.is_contiguous() and x2.is_contiguous()
    if merge_rows_ok(T, D):
        dots = empty(4, B * T, like=x1)
        check(lib().tavsr_merge_rows_fwd(ptr(x1), ptr(x2), ptr(lens), ptr(lens2), _ptr_array(params), ptr(dots), ptr(score), ptr(w),
                                         ptr(out), B, T, D, stream()), "tavsr_merge_rows_fwd")
        return score, dots, w, out
    score, pooled, w = merge_pool_fwd(x1, x2, lens, params, B, T, lens2=lens2)     # other widths: one workgroup per utterance
    return score, pooled, w, merge_combine(x1, x2, w, B, T)


def merge_proj_ok(x1, x2, w, T, D, res=None) -> bool:
    return (ops.MERGE_PROJ and ops.MERGE_ROWS and w.shape == (D, D) and w.is_contiguous() and x1.is_contiguous() and x2.is_contiguous()
            and (res is None or res.is_contiguous()) and bool(lib().tavsr_merge_proj_ok(T, D)))


def merge_proj_fwd(x1, x2, lens, params, w, b, res, alpha, p, B, T, lens2=None, save=True, rowdots=None):
    """the layer's tail behind the branch join in one launch (csrc/mergeproj.hip): learned_ave merge of x1 / x2 and
    ``res + alpha * dropout(merge_proj(mix), p)`` -> (score, dots, wts, mix | None, out, token).  ``dots`` / ``score`` / ``wts`` are
    what ``merge_bwd`` wants back (the row-parallel route's saved tensors), ``mix`` merge_proj's saved input (``save``)."""
    D = x1.shape[-1]
    M = B * T
    require_cuda(x1, x2, lens, lens2, w, b, res)
    score, wts, dots = empty(2, B, T, like=x1), empty(B, 2, like=x1), empty(4, M, like=x1)
    mix = torch.empty_like(x1) if save else None
    out = torch.empty_like(x1)
    tok = _new_token(p, M * D, x1.device) if p and p > 0.0 else None
    rd1, rd2 = rowdots if rowdots is not None else (None, None)      # the producers' GEMM epilogues left the row dots (linear_drop(rowdot=))
    assert rd1 is None or (rd1.shape == (M, 4, 2) and rd2.shape == (M, 4, 2) and rd1.is_contiguous() and rd2.is_contiguous())
    check(lib().tavsr_merge_proj_fwd_dots(ptr(x1), ptr(x2), ptr(lens), ptr(lens2), _ptr_array(params), ptr(w), ptr(b), ptr(res), alpha,
                                          p if tok is not None else 0.0, ptr(None if tok is None else tok[2]), 0 if tok is None else tok[1],
                                          ptr(rd1), ptr(rd2), ptr(dots), ptr(score), ptr(wts), ptr(mix), ptr(out), B, T, D, stream()),
          "tavsr_merge_proj_fwd_dots")
    return score, dots, wts, mix, out, tok


def merge_combine(x1, x2, w, B, T):
    D = x1.shape[-1]
    out = torch.empty_like(x1)
    check(lib().tavsr_merge_combine(ptr(x1), ptr(x2), ptr(w), ptr(out), B, T, D, stream()), "tavsr_merge_combine")
    return out


def merge_bwd(dm, x1, x2, lens, params, score, pooled, w, B, T, lens2=None, drop1=None, drop2=None):
    """``pooled``: the ``aux`` of merge_fwd.  ``drop1`` / ``drop2`` (dropout tokens of the two branch outputs): dx1 / dx2 come
    back under those masks - from the same launch on the row-parallel route, by a dropout launch each otherwise."""
    D = x1.shape[-1]
    dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
    # gradient order: weight{pool1,pool2,w1,w2} then bias{pool1,pool2,w1,w2}
    order = [0, 1, 4, 5, 2, 3, 6, 7]
    dparams = [torch.empty_like(params[i]) for i in order]
    if pooled.dim() == 2:          # row dots: the row-parallel launches
        require_cuda(dm, x1, x2, lens, lens2, score, pooled, w)
        assert dm.is_contiguous() and x1.is_contiguous() and x2.is_contiguous()
        ws = empty(lib().tavsr_merge_rows_bwd_ws(B, T, D), like=x1)
        seed = (drop1 or drop2 or (0.0, 0, None))[2]
        assert drop1 is None or drop2 is None or drop1[2] is drop2[2] or drop1[2].data_ptr() == drop2[2].data_ptr()
        p1, o1 = (drop1[0], drop1[1]) if drop1 is not None else (0.0, 0)
        p2, o2 = (drop2[0], drop2[1]) if drop2 is not None else (0.0, 0)
        check(lib().tavsr_merge_rows_bwd(ptr(dm), ptr(x1), ptr(x2), ptr(lens), ptr(lens2), _ptr_array(params), ptr(score), ptr(w),
                                         ptr(pooled), ptr(dx1), ptr(dx2), _ptr_array(dparams), 0, ptr(ws), p1, o1, p2, o2, ptr(seed), B, T,
                                         D, stream()), "tavsr_merge_rows_bwd")
        grads = [None] * 8
        for g, i in zip(dparams, order):
            grads[i] = g
        return dx1, dx2, grads
    ws = empty(lib().tavsr_merge_bwd_ws(B, D), like=x1)
    check(lib().tavsr_merge_bwd(ptr(dm), ptr(x1), ptr(x2), ptr(lens), ptr(lens2), _ptr_array(params), ptr(score), ptr(pooled),
                                ptr(w), ptr(dx1), ptr(dx2), _ptr_array(dparams), 0, ptr(ws), B, T, D, stream()),
          "tavsr_merge_bwd")
    grads = [None] * 8
    for g, i in zip(dparams, order):
        grads[i] = g
    if drop1 is not None:
        dropout(dx1, drop1[0], out=dx1, token=drop1)
    if drop2 is not None:
        dropout(dx2, drop2[0], out=dx2, token=drop2)
    return dx1, dx2, grads


def act_(x, act):
    """x = act(x) in place."""
    require_cuda(x)
    assert x.is_contiguous()
    check(lib().tavsr_act_fwd(ptr(x), ptr(x), x.numel(), ACT[act], stream()), "tavsr_act_fwd")
    return x
