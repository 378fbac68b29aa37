"""The blocks an encoder layer is sequenced from, each written once: the feed-forward block, the attention cores, the
relative-position attention branch, the cgMLP branch and the Conformer convolution module, with the state each keeps for its
backward as a named tuple.

``tavsr.functional`` (Branchformer layer, decoder) and ``tavsr.functional_av`` (tailored audio-visual stream) order these
blocks; the C sequencers of csrc/layer.hip leave the same state behind (``functional._layer_sv``, ``functional_av._ts_c_desc``)
so that the Python backward runs on either.  The named tuples are that contract: a field a C forward leaves ``None`` is named
in the type's docstring.  Parameters come as a mapping by name (``p``), gradients go into a dict by name (``G``).
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch

from . import ops

EPS_ESPNET = 1e-12  # espnet LayerNorm eps

# the six parameters of a feed-forward block in the order _FFN.fwd takes them and _FFN.bwd returns their gradients
FFM_PARAMS = ("norm_ff_macaron.weight", "norm_ff_macaron.bias", "feed_forward_macaron.w_1.weight", "feed_forward_macaron.w_1.bias",
              "feed_forward_macaron.w_2.weight", "feed_forward_macaron.w_2.bias")
FF_PARAMS = ("norm_ff.weight", "norm_ff.bias", "feed_forward.w_1.weight", "feed_forward.w_1.bias", "feed_forward.w_2.weight",
             "feed_forward.w_2.bias")


class FFNSaved(NamedTuple):
    """kept by a feed-forward block: its input rows, the LayerNorm's statistics and output, the pre-activations and hidden rows
    [M, hidden] and the tokens of the inner / outer dropout.  Without ``save`` (a forward no backward follows) ``z`` is ``None``
    on the Python route, and a C forward leaves ``mean``, ``rstd``, ``n``, ``z`` and ``h`` all ``None``."""
    x: Any
    mean: Any
    rstd: Any
    n: Any
    z: Any
    h: Any
    t_in: Any
    t_out: Any


class AttnSaved(NamedTuple):
    """kept by the attention branch: statistics of the branch's LayerNorm and its output ``n``, the q | k | v rows, the projected
    positional rows, q + pos_bias_u / q + pos_bias_v, the context rows, the core's own state and the tokens of the
    probabilities' dropout and of the branch output's.  On the fused core (every C forward) ``qu``, ``qv`` and ``t_att`` are
    ``None`` and ``attn`` is (log-sum-exp rows, token); on the unfused one ``attn`` holds the probabilities.  ``mean`` / ``rstd``
    are ``None`` from a C forward without ``save``.  ``mean``, ``rstd`` and ``t_br`` are filled in by the caller of
    ``AttnBranch.fwd`` (the LayerNorm in front and the output projection behind are the caller's)."""
    mean: Any
    rstd: Any
    n: Any
    qkv: Any
    pp: Any
    qu: Any
    qv: Any
    cx: Any
    attn: Any
    t_att: Any
    t_br: Any


class FastAttnSaved(NamedTuple):
    """kept by the additive-attention branch: statistics of the branch's LayerNorm and its output ``n``, the q | k rows, the core's
    state (ops.fastattn_fwd: the two pooling weights [B, H, T], the pooled vectors before and after their dropout, their tokens),
    the rows ``wv`` = pk * q that ``transform`` reads, and the tokens of the module's output dropout and of the layer's.  ``mean``,
    ``rstd`` and ``t_br`` are filled in by the caller of ``FastAttnBranch.fwd``."""
    mean: Any
    rstd: Any
    n: Any
    qk: Any
    core: Any
    wv: Any
    t_tr: Any
    t_br: Any


class CgmlpSaved(NamedTuple):
    """kept by the cgMLP branch: statistics of the branch's LayerNorm and its output ``n``, channel_proj1's output ``g`` = gelu(z),
    the CSGU's normalised gate half with its statistics, the gated rows ``u``, the depthwise convolution's output and the tokens
    of the CSGU's dropout and of the branch output's.  Without ``save`` ``z``, ``gn`` and ``conv`` are ``None`` (``gn`` / ``conv``
    on the fused CSGU and from a C forward; ``z`` always), and so are ``mean`` / ``rstd`` from a C forward.  ``mean``, ``rstd`` and
    ``t_br`` are filled in by the caller of ``CgmlpBranch.fwd``."""
    mean: Any
    rstd: Any
    n: Any
    g: Any
    z: Any
    gn: Any
    gmean: Any
    grstd: Any
    u: Any
    conv: Any
    t_u: Any
    t_br: Any


def _drop_(x, p):
    """in-place train-mode dropout; returns the token that regenerates the mask (None when p == 0)."""
    if not p or p <= 0.0:
        return None
    return ops.dropout(x, p, out=x)[1]


def _drop_bwd_(dy, tok):
    """in-place backward of _drop_ (same mask, same scale); no-op without a token."""
    if tok is not None:
        ops.dropout(dy, tok[0], out=dy, token=tok)
    return dy


def _drop_bwd(dy, tok):
    """out-of-place variant for gradients that are still needed unmasked (residual paths)."""
    return dy if tok is None else ops.dropout(dy, tok[0], token=tok)[0]


class _FFN:
    """y = x + scale * drop(W2 drop(act(W1 LN(x) + b1)) + b2)   (encoder_layer.py:192-194,312-314; decoder FFN;
    the inner dropout is PositionwiseFeedForward's, the outer one the layer's: both rate ``p`` in the reference)."""

    @staticmethod
    def fwd(x, ln_w, ln_b, w1, b1, w2, b2, act, scale, eps=EPS_ESPNET, p=0.0, save=True):
        """``save``: keep what the backward needs (the [M, hidden] pre-activations); False for passes without one."""
        if ops.ffn2_usable(x, w1, act):      # streaming chain kernel (csrc/ffn2.hip) + finishing launch; GEMM-path masks
            y, (n, mean, rstd, z, h, t_in, t_out), _, _ = ops.ffn2_fwd(x, ln_w, ln_b, eps, w1, b1, w2, b2, act, scale, p=p,
                                                                       save=save)
            return y, FFNSaved(x=x, mean=mean, rstd=rstd, n=n, z=z, h=h, t_in=t_in, t_out=t_out)
        n, mean, rstd = ops.layernorm_fwd(x, ln_w, ln_b, eps)
        if save:
            h, z, t_in = ops.linear_drop(n, w1, b1, p, act=act, save_z=True)     # both dropouts ride in the GEMM epilogues
        else:
            (h, t_in), z = ops.linear_drop(n, w1, b1, p, act=act), None
        y, t_out = ops.linear_drop(h, w2, b2, p, alpha=scale, res=x)             # x + scale * dropout(.)
        return y, FFNSaved(x=x, mean=mean, rstd=rstd, n=n, z=z, h=h, t_in=t_in, t_out=t_out)

    @staticmethod
    def fwd_ln(x, ln_w, ln_b, w1, b1, w2, b2, act, scale, norms, eps=EPS_ESPNET, p=0.0, save=True):
        """``fwd`` plus the LayerNorms (espnet eps) the consumers of y start with: ``norms`` = [(gamma, beta), ...] (at most
        two) -> (y, saved, [n_k], mean, rstd).  On the streaming path they ride in the finishing launch (one statistics
        pass for all of them); otherwise they are the usual LayerNorm launches."""
        if ops.ffn2_usable(x, w1, act):
            y, (n, mean, rstd, z, h, t_in, t_out), outs, (m2, r2) = ops.ffn2_fwd(
                x, ln_w, ln_b, eps, w1, b1, w2, b2, act, scale, p=p, save=save, ln2=norms, ln2_eps=EPS_ESPNET, ln2_stats=save)
            return y, FFNSaved(x=x, mean=mean, rstd=rstd, n=n, z=z, h=h, t_in=t_in, t_out=t_out), outs, m2, r2
        y, saved = _FFN.fwd(x, ln_w, ln_b, w1, b1, w2, b2, act, scale, eps=eps, p=p, save=save)
        outs, m2, r2 = [], None, None
        for g, b in norms:
            o, m2, r2 = ops.layernorm_fwd(y, g, b, EPS_ESPNET)
            outs.append(o)
        return y, saved, outs, m2, r2

    @staticmethod
    def bwd(dy, saved, ln_w, w1, w2, act, scale, grp=None, lng=None, chain=True, dyd=None, out_drop=None):
        """returns dx (includes the residual path) and grads (ln_w, ln_b, w1, b1, w2, b2).  ``grp`` (ops.WgradGroup)
        defers the two weight gradients to the caller's grouped launch.  ``chain``: the two activation gradients as one
        streaming launch (ops.ffn2_bwd_dx) instead of two dgrad GEMMs - callers that run two of these blocks side by side
        on two launch queues pass False (a chain kernel owns every CU; two of them serialise, two GEMM sequences overlap)."""
        x, mean, rstd, n, z, h, t_in, t_out = saved
        wgrad = ops.linear_dw if grp is None else grp.add
        if dyd is None:              # (callers whose producer of dy is a LayerNorm backward get the masked copy from that launch)
            dyd = _drop_bwd(dy, t_out)
        gw2, gb2 = wgrad(dyd, h, alpha=scale, bias_grad=True)
        stream2 = chain and ops.FFN2_BWD and ops.ffn2_shape_ok(dyd, w1, act) and z.is_contiguous()
        if stream2:
            # the block's own LayerNorm backward is dn's only reader: it sums the launch's partials itself (no finishing launch)
            slab_ok = (ops.FFN2_BWD_LN and lng is not None and lng.takes(*x.shape) and (out_drop is None or ops.LN_BWD_DROP)
                       and x.is_contiguous())
            dz, dn = ops.ffn2_bwd_dx(dyd, scale, w1, w2, z, act, t_in, sum_dn=not slab_ok)
        else:
            dz = ops.linear_dx_drop(dyd, w2, t_in, alpha=scale, DZ=z, dact=act)    # inner mask and act'(z) in the epilogue
        gw1, gb1 = wgrad(dz, n, bias_grad=True)
        if not stream2:
            dn = ops.linear_dx(dz, w1)
        if out_drop is not None and lng is not None:       # + dx under the NEXT block's outer mask, from the same launch
            dx, gln_w, gln_b, dxd = lng.bwd(dn, x, mean, rstd, ln_w, dx_add=dy, drop=out_drop)
            return dx, (gln_w, gln_b, gw1, gb1, gw2, gb2), dxd
        ln_bwd = ops.layernorm_bwd if lng is None else lng.bwd      # lng: the node's shared (dgamma, dbeta) reduction
        dx, gln_w, gln_b = ln_bwd(dn, x, mean, rstd, ln_w, dx_add=dy)
        return dx, (gln_w, gln_b, gw1, gb1, gw2, gb2)


class _AttnFused:
    """Attention core on the fused kernels (ops.attn_fwd / attn_bwd): scores, rel_shift, mask, softmax, dropout and the
    context product in one launch; only the per-row log-sum-exp is kept for the backward, which recomputes the
    probabilities.  q / k / v are 2-D row buffers with element offsets of their column windows (as _SelfAttnCore)."""

    @staticmethod
    def fwd(q, q_off, kbuf, k_off, vbuf, v_off, B, T1, T2, H, dk, klens, causal, pos=None, bias_u=None, bias_v=None,
            p_att=0.0):
        ctx, lse, tok = ops.attn_fwd(q, q_off, kbuf, k_off, vbuf, v_off, B, T1, T2, H, dk, klens=klens, causal=causal,
                                     pos=pos, bias_u=bias_u, bias_v=bias_v, p_drop=p_att)
        return ctx, (lse, tok)

    @staticmethod
    def bwd(dctx, ctx, saved, q, q_off, kbuf, k_off, vbuf, v_off, dq, dq_off, dk_buf, dk_off, dv_buf, dv_off, B, T1, T2, H,
            dk, klens, causal, pos=None, bias_u=None, bias_v=None, lazy_dp=False):
        """writes d/d(q+u) into dq, dK, dV into their windows; rel-pos: returns (dqv, dp) with dp the gradient of the
        projected positional rows [2*T1-1, H*dk].  ``lazy_dp``: dp comes back as a function that computes it (two launches whose only
        reader is linear_pos's weight gradient: the caller may run them with its other weight gradients, off the backward chain)."""
        lse, tok = saved
        dqv, sk = ops.attn_bwd(dctx, ctx, lse, tok, q, q_off, kbuf, k_off, vbuf, v_off, B, T1, T2, H, dk, dq, dq_off,
                               dk_buf, dk_off, dv_buf, dv_off, klens=klens, causal=causal, pos=pos, bias_u=bias_u,
                               bias_v=bias_v)
        if pos is None:
            return None, None
        D = H * dk
        W, Wp = 2 * T1 - 1, sk.shape[-1]

        def make_dp():
            # dP[:,h] = sum_b ds_skew[h,b]^T (q + v)[b,:,h]  == one K = B*T1 GEMM per head
            _, qv = ops.add_head_bias(q[:, q_off: q_off + D], bias_u, bias_v)
            dp = ops.empty(W, D, like=dctx)
            ops.gemm(W, dk, B * T1, sk, Wp, qv, D, dp, D, a_kmajor=True, b_kmajor=True, nb1=H, sA=(B * T1 * Wp, 0),
                     sB=(dk, 0), sC=(dk, 0))
            return dp
        return dqv, (make_dp if lazy_dp else make_dp())


class _SelfAttnCore:
    """Scores/softmax/context of one attention call on head-strided buffers.

    q rows live in ``qbuf`` (row stride ldq, element offset q_off), k/v likewise; outputs go to
    ``ctx`` [B*T1, D].  rel-pos (espnet RelPositionMultiHeadedAttention) when ``p`` is given."""

    @staticmethod
    def fwd(qu, ldq, q_off, kbuf, ldk, k_off, vbuf, ldv, v_off, B, T1, T2, H, dk, klens, causal, qv=None, p=None,
            p_att=0.0):
        D = H * dk
        dev = qu
        S = ops.pad4(T2)   # padded score-row stride: 16-byte loads in the GEMMs that read the scores
        ac = ops.empty(H, B, T1, S, like=dev)
        # ac[h,b] = Qu[b,:,h] K[b,:,h]^T
        ops.gemm(T1, T2, dk, qu, ldq, kbuf, ldk, ac, S, a_off=q_off, b_off=k_off, nb1=B, nb2=H,
                 sA=(T1 * ldq, dk), sB=(T2 * ldk, dk), sC=(T1 * S, B * T1 * S))
        bd = None
        W = 0
        if p is not None:
            W = 2 * T1 - 1
            Wp = ops.pad4(W)
            bd = ops.empty(H, B, T1, Wp, like=dev)
            ops.gemm(T1, W, dk, qv, D, p, D, bd, Wp, nb1=B, nb2=H, sA=(T1 * D, dk), sB=(0, dk),
                     sC=(T1 * Wp, B * T1 * Wp))
        if p_att and p_att > 0.0:      # dropout on the probabilities (espnet forward_attention) by the softmax launch itself;
            attn, pv, tok = ops.softmax_fwd(ac, bd, klens, 1.0 / math.sqrt(dk), causal, T2=T2, W=W, p_drop=p_att)
            tok = (tok, pv)            # attn is kept; the dropped probabilities stay resident for dV (5 MB per layer)
        else:
            attn = ops.softmax_fwd(ac, bd, klens, 1.0 / math.sqrt(dk), causal, T2=T2, W=W)
            pv, tok = attn, None
        ctx = ops.empty(B * T1, D, like=dev)
        # ctx[b,:,h] = drop(attn)[h,b] V[b,:,h]
        ops.gemm(T1, dk, T2, pv, S, vbuf, ldv, ctx, D, b_off=v_off, b_kmajor=True, nb1=B, nb2=H,
                 sA=(T1 * S, B * T1 * S), sB=(T2 * ldv, dk), sC=(T1 * D, dk))
        return ctx, attn, tok

    @staticmethod
    def bwd(dctx, attn, qu, ldq, q_off, kbuf, ldk, k_off, vbuf, ldv, v_off, dq, lddq, dq_off, dk_buf, lddk, dk_off,
            dv_buf, lddv, dv_off, B, T1, T2, H, dk, qv=None, p=None, tok=None):
        """Writes dQ(u) into dq, dK into dk_buf, dV into dv_buf (head-strided); returns (dqv, dp) for rel-pos."""
        D = H * dk
        S = attn.shape[-1]
        sS = (T1 * S, B * T1 * S)
        dattn = torch.empty_like(attn)
        # dattn[h,b] = dctx[b,:,h] V[b,:,h]^T
        ops.gemm(T1, T2, dk, dctx, D, vbuf, ldv, dattn, S, b_off=v_off, nb1=B, nb2=H, sA=(T1 * D, dk),
                 sB=(T2 * ldv, dk), sC=sS)
        # dV[b,:,h] = drop(attn)[h,b]^T dctx[b,:,h]
        pv = attn if tok is None else tok[1]
        ops.gemm(T2, dk, T1, pv, S, dctx, D, dv_buf, lddv, c_off=dv_off, a_kmajor=True, b_kmajor=True, nb1=B, nb2=H,
                 sA=sS, sB=(T1 * D, dk), sC=(T2 * lddv, dk))
        del pv
        # dattn is the gradient of the dropped probabilities: the softmax backward regenerates the mask itself
        ds, sk = ops.softmax_bwd(attn, dattn, 1.0 / math.sqrt(dk), skew=p is not None, T2=T2,
                                 token=None if tok is None else tok[0])
        # dQu[b,:,h] = ds[h,b] K[b,:,h]
        ops.gemm(T1, dk, T2, ds, S, kbuf, ldk, dq, lddq, b_off=k_off, c_off=dq_off, b_kmajor=True, nb1=B, nb2=H,
                 sA=sS, sB=(T2 * ldk, dk), sC=(T1 * lddq, dk))
        # dK[b,:,h] = ds[h,b]^T Qu[b,:,h]
        ops.gemm(T2, dk, T1, ds, S, qu, ldq, dk_buf, lddk, b_off=q_off, c_off=dk_off, a_kmajor=True, b_kmajor=True,
                 nb1=B, nb2=H, sA=sS, sB=(T1 * ldq, dk), sC=(T2 * lddk, dk))
        if p is None:
            return None, None
        W = 2 * T1 - 1
        Wp = sk.shape[-1]
        dqv = ops.empty(B * T1, D, like=dctx)
        # dQv[b,:,h] = ds_skew[h,b] P[:,h]
        ops.gemm(T1, dk, W, sk, Wp, p, D, dqv, D, b_kmajor=True, nb1=B, nb2=H, sA=(T1 * Wp, B * T1 * Wp), sB=(0, dk),
                 sC=(T1 * D, dk))
        # dP[:,h] = sum_b ds_skew[h,b]^T Qv[b,:,h]  == one K = B*T1 GEMM per head
        dp = ops.empty(W, D, like=dctx)
        ops.gemm(W, dk, B * T1, sk, Wp, qv, D, dp, D, a_kmajor=True, b_kmajor=True, nb1=H, sA=(B * T1 * Wp, 0),
                 sB=(dk, 0), sC=(dk, 0))
        return dqv, dp


class AttnBranch:
    """The relative-position self-attention branch of an encoder layer between its LayerNorm and its output projection
    (espnet RelPositionMultiHeadedAttention; src/encoder/branchformer/encoder_layer.py:205-212, tailored/encoder_layer.py:185-196).
    The LayerNorm in front and the forward output projection are the caller's: they are what differs between the layers."""

    @staticmethod
    def fwd(n, p, pos_emb, lens, B, T, H, p_att):
        """normalised rows ``n`` [B*T, D] -> (context rows cx, AttnSaved without mean / rstd / t_br).  ``pos_emb`` None: plain
        multi-head attention over absolute positions (espnet MultiHeadedAttention, ``selfattn``): no positional rows, no head
        biases; ``pp``, ``qu`` and ``qv`` stay ``None`` and ``attn`` tells the core (a tuple: the fused one)."""
        M, D = n.shape
        dk = D // H
        qkv = ops.empty(M, 3 * D, like=n)
        ops.linear_group(n, [(p[f"attn.linear_{c}.weight"], p[f"attn.linear_{c}.bias"], j * D) for j, c in enumerate("qkv")], qkv)
        if pos_emb is None:
            if ops.ATTN_FUSED and dk == 64:
                t_att = None
                cx, attn = _AttnFused.fwd(qkv, 0, qkv, D, qkv, 2 * D, B, T, T, H, dk, lens, False, p_att=p_att)
            else:
                cx, attn, t_att = _SelfAttnCore.fwd(qkv, 3 * D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, B, T, T, H, dk, lens, False, p_att=p_att)
            return cx, AttnSaved(mean=None, rstd=None, n=n, qkv=qkv, pp=None, qu=None, qv=None, cx=cx, attn=attn, t_att=t_att, t_br=None)
        pp = ops.linear(pos_emb.reshape(-1, D), p["attn.linear_pos.weight"])
        bias_u, bias_v = p["attn.pos_bias_u"].reshape(-1), p["attn.pos_bias_v"].reshape(-1)
        if ops.ATTN_FUSED and dk == 64:
            qu = qv = t_att = None
            cx, attn = _AttnFused.fwd(qkv, 0, qkv, D, qkv, 2 * D, B, T, T, H, dk, lens, False, pos=pp, bias_u=bias_u, bias_v=bias_v,
                                      p_att=p_att)
        else:
            qu, qv = ops.add_head_bias(qkv[:, :D], bias_u, bias_v)
            cx, attn, t_att = _SelfAttnCore.fwd(qu, D, 0, qkv, 3 * D, D, qkv, 3 * D, 2 * D, B, T, T, H, dk, lens, False, qv=qv, p=pp,
                                                p_att=p_att)
        return cx, AttnSaved(mean=None, rstd=None, n=n, qkv=qkv, pp=pp, qu=qu, qv=qv, cx=cx, attn=attn, t_att=t_att, t_br=None)

    @staticmethod
    def bwd(d_out, saved, p, pos_emb, lens, B, T, H, grp, G, alpha=1.0, lazy=False):
        """``d_out``: gradient of the branch output under its dropout mask; the output was ``alpha`` times the projection.
        Returns (dn, late): the gradient of the normalised rows, and - ``lazy`` - the positional chain (the two positional bias
        sums, then the positional rows' gradient with linear_pos's weight gradient) as functions nobody on the backward chain
        waits for: the caller runs them, in this order, with its other weight gradients.  Fills ``G``; the weight gradients of
        the four projections go through ``grp``."""
        s = saved
        M, D = s.cx.shape
        dk = D // H
        G["attn.linear_out.weight"], G["attn.linear_out.bias"] = grp.add(d_out, s.cx, alpha=alpha, bias_grad=True)
        dcx = ops.linear_dx(d_out, p["attn.linear_out.weight"], alpha=alpha)
        dqkv = torch.empty_like(s.qkv)
        if pos_emb is None:      # plain multi-head attention: dQ goes straight into its window
            if isinstance(s.attn, tuple):
                _AttnFused.bwd(dcx, s.cx, s.attn, s.qkv, 0, s.qkv, D, s.qkv, 2 * D, dqkv, 0, dqkv, D, dqkv, 2 * D, B, T, T, H, dk, lens, False)
            else:
                _SelfAttnCore.bwd(dcx, s.attn, s.qkv, 3 * D, 0, s.qkv, 3 * D, D, s.qkv, 3 * D, 2 * D, dqkv, 3 * D, 0, dqkv, 3 * D, D,
                                  dqkv, 3 * D, 2 * D, B, T, T, H, dk, tok=s.t_att)
            for j, c in enumerate("qkv"):
                G[f"attn.linear_{c}.weight"], G[f"attn.linear_{c}.bias"] = grp.add(dqkv[:, j * D:(j + 1) * D], s.n, bias_grad=True)
            return ops.linear_dx_cat(dqkv, [p[f"attn.linear_{c}.weight"] for c in "qkv"]), []
        dqu = ops.empty(M, D, like=d_out)
        if s.qu is None:         # fused attention core
            dqv, dp = _AttnFused.bwd(dcx, s.cx, s.attn, s.qkv, 0, s.qkv, D, s.qkv, 2 * D, dqu, 0, dqkv, D, dqkv, 2 * D, B, T, T, H, dk,
                                     lens, False, pos=s.pp, bias_u=p["attn.pos_bias_u"].reshape(-1),
                                     bias_v=p["attn.pos_bias_v"].reshape(-1), lazy_dp=lazy)
        else:
            dqv, dp = _SelfAttnCore.bwd(dcx, s.attn, s.qu, D, 0, s.qkv, 3 * D, D, s.qkv, 3 * D, 2 * D, dqu, D, 0, dqkv, 3 * D, D,
                                        dqkv, 3 * D, 2 * D, B, T, T, H, dk, qv=s.qv, p=s.pp, tok=s.t_att)
        gu, gv, *late = ops.add2_colsum(dqu, dqv, dqkv[:, :D], lazy_sums=lazy)      # dQ = dQu + dQv and both bias gradients, one pass
        G["attn.pos_bias_u"], G["attn.pos_bias_v"] = gu.view_as(p["attn.pos_bias_u"]), gv.view_as(p["attn.pos_bias_v"])
        pe2d = pos_emb.reshape(-1, D)
        if callable(dp):         # the positional rows' gradient and linear_pos's weight gradient: 4 launches, ~55 us of the branch
            late.append(lambda: G.__setitem__("attn.linear_pos.weight", ops.linear_dw(dp(), pe2d)))
        else:
            G["attn.linear_pos.weight"] = ops.linear_dw(dp, pe2d)      # K = 2T-1: not a multiple of 32, stays alone
        for j, c in enumerate("qkv"):      # three problems with their own outputs (no sliced gradients)
            G[f"attn.linear_{c}.weight"], G[f"attn.linear_{c}.bias"] = grp.add(dqkv[:, j * D:(j + 1) * D], s.n, bias_grad=True)
        dn = ops.linear_dx_cat(dqkv, [p[f"attn.linear_{c}.weight"] for c in "qkv"])      # one K = 3D GEMM
        return dn, late


# the ten parameters of FastSelfAttention
FAST_ATTN_PARAMS = tuple(f"attn.{m}.{w}" for m in ("query", "query_att", "key", "key_att", "transform") for w in ("weight", "bias"))


class FastAttnBranch:
    """The additive-attention branch of an encoder layer behind its LayerNorm (espnet2 FastSelfAttention, ``fast_selfattn``;
    src/encoder/branchformer/encoder_layer.py:204-210: ``self.attn(x1, mask)``, no output projection of the layer's):
    q | k = query(n) | key(n), the pooling core on csrc/fastattn.hip, out = dropout(transform(pk * q)) + q.  The LayerNorm in front
    and the layer's dropout on ``out`` are the caller's."""

    @staticmethod
    def fwd(n, p, lens, B, T, H, p_drop, out=None):
        """normalised rows ``n`` [B*T, D] -> (the module's output rows, FastAttnSaved without mean / rstd / t_br).  ``out``: a
        [M, >= D] buffer whose first D columns receive the output (the concat merge's window); without dropout the transform GEMM
        writes there itself, with it the masked result is copied in (one more pass over [M, D])."""
        M, D = n.shape
        qk = ops.empty(M, 2 * D, like=n)
        ops.linear_group(n, [(p["attn.query.weight"], p["attn.query.bias"], 0), (p["attn.key.weight"], p["attn.key.bias"], D)], qk)
        wv, core = ops.fastattn_fwd(qk, p["attn.query_att.weight"], p["attn.query_att.bias"], p["attn.key_att.weight"],
                                    p["attn.key_att.bias"], lens, B, T, D, H, p=p_drop)
        if out is not None and not (p_drop and p_drop > 0.0):
            ops.linear(wv, p["attn.transform.weight"], p["attn.transform.bias"], res=qk[:, :D], out=out, out_off=0, ldc=out.shape[1])
            out, t_tr = out[:, :D], None
        else:
            y, t_tr = ops.linear_drop(wv, p["attn.transform.weight"], p["attn.transform.bias"], p_drop, res=qk[:, :D])
            if out is not None:
                ops.axpby2d(y, None, 1.0, 0.0, out[:, :D])
                y = out[:, :D]
            out = y
        return out, FastAttnSaved(mean=None, rstd=None, n=n, qk=qk, core=core, wv=wv, t_tr=t_tr, t_br=None)

    @staticmethod
    def bwd(d_out, saved, p, lens, B, T, H, grp, G):
        """``d_out``: gradient of the module's output (under the layer's dropout mask).  Returns the gradient of the normalised
        rows; fills ``G`` (the three projections' weight gradients through ``grp``; the four score gradients come from the
        core's fixed-order partial sums)."""
        s = saved
        M, D = s.wv.shape
        if s.t_tr is not None and not d_out.is_contiguous():      # (the concat merge hands over a column window)
            d_out = d_out.contiguous()
        dyt = _drop_bwd(d_out, s.t_tr)
        G["attn.transform.weight"], G["attn.transform.bias"] = grp.add(dyt, s.wv, bias_grad=True)
        dwv = ops.linear_dx(dyt, p["attn.transform.weight"])
        dqk, gwq, gbq, gwk, gbk = ops.fastattn_bwd(dwv, d_out, s.qk, s.core, p["attn.query_att.weight"], p["attn.key_att.weight"],
                                                   lens, B, T, D, H)
        G["attn.query_att.weight"], G["attn.query_att.bias"], G["attn.key_att.weight"], G["attn.key_att.bias"] = gwq, gbq, gwk, gbk
        G["attn.query.weight"], G["attn.query.bias"] = grp.add(dqk[:, :D], s.n, bias_grad=True)
        G["attn.key.weight"], G["attn.key.bias"] = grp.add(dqk[:, D:], s.n, bias_grad=True)
        return ops.linear_dx_cat(dqk, [p["attn.query.weight"], p["attn.key.weight"]])


class CgmlpBranch:
    """The cgMLP branch of an encoder layer (espnet ConvolutionalGatingMLP: channel_proj1 + gelu, CSGU) between its LayerNorm
    and channel_proj2 (src/encoder/branchformer/encoder_layer.py:214-224, tailored/encoder_layer.py:198-208).  The LayerNorm in
    front and the forward of channel_proj2 are the caller's."""

    @staticmethod
    def fwd(n, p, B, T, p_drop, need):
        """normalised rows ``n`` [B*T, D] -> (gated rows u, CgmlpSaved without mean / rstd / t_br)"""
        w1c, cw = p["cgmlp.channel_proj1.0.weight"], p["cgmlp.csgu.conv.weight"]
        # channel_proj1's epilogue leaves the CSGU's LayerNorm statistics as per-tile row sums (no statistics launch)
        rst = (ops.empty(n.shape[0], w1c.shape[0] // 64, 2, like=n)
               if (ops.CSGU_FUSED and cw.shape[-1] == 31 and ops.csgu_rowstat_ok(n, w1c)) else None)
        if need:
            g, z = ops.linear(n, w1c, p["cgmlp.channel_proj1.0.bias"], act="gelu", save_z=True, rowstat=rst)
        else:
            g, z = ops.linear(n, w1c, p["cgmlp.channel_proj1.0.bias"], act="gelu", rowstat=rst), None
        Cn = g.shape[1] // 2
        if ops.csgu_usable(g, cw):       # LayerNorm + depthwise convolution + gate + dropout: one pass over g
            u, conv, gn, gmean, grstd, t_u = ops.csgu_fwd(g, p["cgmlp.csgu.norm.weight"], p["cgmlp.csgu.norm.bias"], EPS_ESPNET,
                                                          cw.reshape(Cn, -1), p["cgmlp.csgu.conv.bias"], B, T, p=p_drop, save=need,
                                                          rowstat=rst)
        else:
            gn, gmean, grstd = ops.layernorm_fwd(g[:, Cn:], p["cgmlp.csgu.norm.weight"], p["cgmlp.csgu.norm.bias"], EPS_ESPNET)
            u, conv = ops.dwconv_gate_fwd(gn, g[:, :Cn], cw.reshape(Cn, -1), p["cgmlp.csgu.conv.bias"], B, T)
            t_u = _drop_(u, p_drop)      # csgu: dropout(x_r * x_g)
        return u, CgmlpSaved(mean=None, rstd=None, n=n, g=g, z=z, gn=gn, gmean=gmean, grstd=grstd, u=u, conv=conv, t_u=t_u, t_br=None)

    @staticmethod
    def bwd(d_out, saved, p, B, T, grp, G, alpha=1.0):
        """``d_out``: gradient of the branch output under its dropout mask; the output was ``alpha`` times channel_proj2's.
        Returns the gradient of the normalised rows; fills ``G`` (the two projections' weight gradients through ``grp``)."""
        s = saved
        Cn = s.g.shape[1] // 2
        G["cgmlp.channel_proj2.weight"], G["cgmlp.channel_proj2.bias"] = grp.add(d_out, s.u, alpha=alpha, bias_grad=True)
        du = ops.linear_dx_drop(d_out, p["cgmlp.channel_proj2.weight"], s.t_u, alpha=alpha)
        dg = torch.empty_like(s.g)
        cw = p["cgmlp.csgu.conv.weight"]
        fused = ops.CGMLP_ACT_BWD_FUSED and cw.shape[-1] == 31      # gelu'(z) applied by the two kernels that write dg's halves
        dgn, gcw, gcb = ops.dwconv_gate_bwd(du, s.gn, s.g[:, :Cn], s.conv, cw.reshape(Cn, -1), dg[:, :Cn], B, T,
                                            zr=s.z[:, :Cn] if fused else None)
        G["cgmlp.csgu.conv.weight"], G["cgmlp.csgu.conv.bias"] = gcw.view_as(cw), gcb
        if fused:
            _, G["cgmlp.csgu.norm.weight"], G["cgmlp.csgu.norm.bias"] = ops.layernorm_bwd_act(
                dgn, s.g[:, Cn:], s.gmean, s.grstd, p["cgmlp.csgu.norm.weight"], s.z[:, Cn:], "gelu", dx=dg[:, Cn:])
        else:
            _, G["cgmlp.csgu.norm.weight"], G["cgmlp.csgu.norm.bias"] = ops.layernorm_bwd(
                dgn, s.g[:, Cn:], s.gmean, s.grstd, p["cgmlp.csgu.norm.weight"], dx=dg[:, Cn:])
            ops.act_bwd_(dg, s.z, "gelu")
        G["cgmlp.channel_proj1.0.weight"], G["cgmlp.channel_proj1.0.bias"] = grp.add(dg, s.n, bias_grad=True)
        return ops.linear_dx(dg, p["cgmlp.channel_proj1.0.weight"])


# the eight parameters of the Conformer convolution module behind its LayerNorm, in the order ConvModuleBlock reads them
CONV_PARAMS = ("conv_module.pointwise_conv1.weight", "conv_module.pointwise_conv1.bias", "conv_module.depthwise_conv.weight",
               "conv_module.depthwise_conv.bias", "conv_module.norm.weight", "conv_module.norm.bias",
               "conv_module.pointwise_conv2.weight", "conv_module.pointwise_conv2.bias")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1      # torch.nn.BatchNorm1d defaults (espnet's ConvolutionModule sets neither)


class ConvSaved(NamedTuple):
    """kept by the convolution module: its input rows, the statistics of ``norm_conv`` and its output ``n``, pointwise_conv1's
    output ``h`` [M, 2C] (the GLU's input: the gated rows are never stored), the depthwise convolution's output ``z``, the
    BatchNorm statistics used (batch statistics in training), the activated rows ``y`` that pointwise_conv2 reads and the token
    of the layer's dropout on the module's output."""
    x: Any
    mean: Any
    rstd: Any
    n: Any
    h: Any
    z: Any
    bmean: Any
    brstd: Any
    y: Any
    t_out: Any


class ConvModuleBlock:
    """y = x + drop(pointwise_conv2(act(BatchNorm(depthwise_conv(glu(pointwise_conv1(LN(x))))))))   (espnet conformer/
    encoder_layer.py: x = residual + dropout(conv_module(norm_conv(x))); conformer/convolution.py).  The 1x1 convolutions are
    GEMMs on [M, .] rows, GLU + depthwise convolution one kernel (ops.glu_dwconv_fwd), BatchNorm the channels-last kernels of the
    lip front-end over all M = B*T rows, padded ones included - espnet masks nothing here.  ``bn`` = (running_mean, running_var,
    num_batches_tracked); a training forward updates them on the device, also without a backward to follow.
    ``ln_w is None``: the module alone (espnet ConvolutionModule.forward) - no LayerNorm in front, no residual, no dropout."""

    @staticmethod
    def fwd(x, ln_w, ln_b, p, bn, B, T, act, training, pd=0.0):
        w1, wd, w2 = (p[CONV_PARAMS[0]], p[CONV_PARAMS[2]], p[CONV_PARAMS[6]])
        Cn = wd.shape[0]
        if ln_w is None:
            n, mean, rstd = x, None, None
        else:
            n, mean, rstd = ops.layernorm_fwd(x, ln_w, ln_b, EPS_ESPNET)
        h = ops.linear(n, w1.reshape(2 * Cn, Cn), p[CONV_PARAMS[1]])
        z = ops.glu_dwconv_fwd(h, wd.reshape(Cn, -1), p[CONV_PARAMS[3]], B, T)
        if training:
            bmean, brstd = ops.bn_stats(z, BN_EPS, BN_MOMENTUM, *bn)
        else:
            bmean, brstd = bn[0], ops.rsqrt_eps(bn[1], BN_EPS)
        y = ops.bn_apply_fwd(z, bmean, brstd, p[CONV_PARAMS[4]], p[CONV_PARAMS[5]], None, act)
        if ln_w is None:
            out, t_out = ops.linear(y, w2.reshape(Cn, Cn), p[CONV_PARAMS[7]]), None
        else:
            out, t_out = ops.linear_drop(y, w2.reshape(Cn, Cn), p[CONV_PARAMS[7]], pd, res=x)
        return out, ConvSaved(x=x, mean=mean, rstd=rstd, n=n, h=h, z=z, bmean=bmean, brstd=brstd, y=y, t_out=t_out)

    @staticmethod
    def bwd(dy, saved, ln_w, p, B, T, act, grp, lng, G, dyd=None, out_drop=None):
        """``dy``: gradient of the block's output; ``dyd``: the same under the block's dropout mask where the caller has it.
        Returns (dx, gln_w, gln_b[, dx under ``out_drop``]) - dx includes the residual path; fills ``G`` with the module's
        eight gradients (the two 1x1 convolutions' weight gradients through ``grp``)."""
        s = saved
        w1, wd, w2 = (p[CONV_PARAMS[0]], p[CONV_PARAMS[2]], p[CONV_PARAMS[6]])
        Cn = wd.shape[0]
        if dyd is None:
            dyd = _drop_bwd(dy, s.t_out)
        gw2, G[CONV_PARAMS[7]] = grp.add(dyd, s.y, bias_grad=True)
        G[CONV_PARAMS[6]] = gw2.view_as(w2)
        da = ops.linear_dx(dyd, w2.reshape(Cn, Cn))
        _, dz, G[CONV_PARAMS[4]], G[CONV_PARAMS[5]] = ops.bn_bwd(da, s.z, s.bmean, s.brstd, p[CONV_PARAMS[4]], p[CONV_PARAMS[5]], None,
                                                                 act, need_dz=False)
        dh, gwd, G[CONV_PARAMS[3]] = ops.glu_dwconv_bwd(dz, s.h, wd.reshape(Cn, -1), B, T)
        G[CONV_PARAMS[2]] = gwd.view_as(wd)
        gw1, G[CONV_PARAMS[1]] = grp.add(dh, s.n, bias_grad=True)
        G[CONV_PARAMS[0]] = gw1.view_as(w1)
        dn = ops.linear_dx(dh, w1.reshape(2 * Cn, Cn))
        if ln_w is None:
            return dn, None, None
        return lng.bwd(dn, s.x, s.mean, s.rstd, ln_w, dx_add=dy, drop=out_drop)
