"""GPU: the oldest kernels of the library at the edges their first tests went around - csrc/norm.hip (LayerNorm forward / backward
at every NV, part-filled and idle chunks, a second trip of the backward's grid-stride loop, the statistics-only, accumulate, masked
copy and shared-slab calls; the column sums around the 64-chunk cap; the partial-slab sums around the 16-wave deal and the 4x
unroll; empty inputs) and the glue of csrc/attn.hip (softmax forward / backward at klens = 0 and > T2, part-filled last blocks,
padded rows with poison in the padding, the fused dropout forms; axpby, axpby2d, add_head_bias, act_bwd, scale_dev; refusals).

Restatements, case tables and inputs: tests/rowred_ref.py (tests/test_rowred_host.py checks them on the host).  Every comparison
against float64 is held to max(floor, 4 * e32) and printed (profiles/rowred_edges.txt keeps a run).  Every output and workspace is
pre-filled with NaN; outputs are windows of larger NaN buffers wherever the entry takes a leading dimension: the live part must come
back finite, everything around it as the same NaN bit for bit.  A second identical call is bit-equal."""
import importlib

import pytest
import torch

import ln_stats_ref as R
import rowred_ref as RR

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN_BITS = 0x7FC00000
F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _nan_filled_allocations(monkeypatch):
    """every tensor the ops wrappers allocate through ``empty`` (outputs, workspaces) starts as NaN"""
    def nan_empty(*shape, like=None, dtype=torch.float32, device=None):
        dev = like.device if like is not None else (device if device is not None else "cuda")
        t = torch.empty(shape, dtype=dtype, device=dev)
        return t.fill_(NAN) if t.is_floating_point() else t
    for name in ("tavsr.ops", "tavsr.ops.base", "tavsr.ops.norm", "tavsr.ops.attention", "tavsr.ops.blocks"):
        mod = importlib.import_module(name)
        if hasattr(mod, "empty"):
            monkeypatch.setattr(mod, "empty", nan_empty)


def _api():
    from tavsr import _lib
    return _lib.lib(), _lib.ptr, _lib.stream, _lib.check


class G:
    """an output: the live window [M, N] of a NaN-filled [M + 2, ld] buffer, ``off`` columns in (``flat``: a vector of N)"""

    def __init__(self, M, N, ld=None, off=4, flat=False, init=None):
        ld = N + 2 * off if ld is None else ld
        assert off + N <= ld
        self.buf = torch.full((M + 2, ld), NAN, device="cuda")
        self.v = self.buf[1:M + 1, off:off + N]
        self.live = torch.zeros(M + 2, ld, dtype=torch.bool, device="cuda")
        self.live[1:M + 1, off:off + N] = True
        if init is not None:
            self.v.copy_(init.reshape(M, N))
        if flat:
            assert M == 1
            self.v = self.v[0]

    def ok(self, what=""):
        bits = self.buf.view(torch.int32)
        assert bool((bits[~self.live] == NAN_BITS).all()), f"{what}: written outside the live window"
        assert bool(torch.isfinite(self.buf[self.live]).all()), f"{what}: live output not finite"
        return self

    def untouched(self, what=""):
        assert bool((self.buf.view(torch.int32) == NAN_BITS).all()), f"{what}: written"


def vec(n, init=None):
    """a vector of n live floats, 16-byte aligned"""
    return G(1, n, ld=RR.pad4(n) + 8, flat=True, init=init)


def part_vec(n, init=None):
    """``vec(n)`` that also stands for n = 0: a real address of which no float is live"""
    g = vec(max(n, 1))
    g.live[1, 4 + n:] = False
    if init is not None and n:
        g.v[:n] = init.cuda()
    return g


def dev_window(t, pad=4):
    """host [M, N] -> the same numbers on the device as a column window of a NaN-filled [M, N + 2 pad] buffer"""
    M, N = t.shape
    b = torch.full((M, N + 2 * pad), NAN)
    b[:, pad:pad + N] = t
    return b.cuda()[:, pad:pad + N]


def dev_vec(t, off=4):
    b = torch.full((t.numel() + 8,), NAN)
    b[off:off + t.numel()] = t
    return b.cuda()[off:off + t.numel()]


def _finish(bad):
    assert not bad, "\n" + "\n".join(line for _, line in bad)


def _same(a, b):
    """two runs' outputs: dicts of G (or tensors)"""
    assert a.keys() == b.keys()
    for k in a:
        p, q = (t.ok(k).buf if isinstance(t, G) else t for t in (a[k], b[k]))
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), f"{k}: the second call differs"


# ================================================================================================ LayerNorm
def _ln_fwd(x, w, b, M, D, stats_only=False):
    lib, ptr, stream, check = _api()
    y, mean, rstd = (None if stats_only else G(M, D)), vec(M), vec(M)
    check(lib.tavsr_layernorm_fwd(ptr(x), x.stride(0), ptr(w), ptr(b), R.EPS, None if stats_only else ptr(y.v), D + 8, ptr(mean.v),
                                  ptr(rstd.v), M, D, stream()), "tavsr_layernorm_fwd")
    return y, mean, rstd


def _ln_ws(M, D):
    return torch.full((max(1, _api()[0].tavsr_layernorm_bwd_ws(M, D)),), NAN, device="cuda")


def _ln_bwd(dy, x, mean, rstd, w, M, D, add=None, z=None, accumulate=0, init=(None, None)):
    lib, ptr, stream, check = _api()
    dx, dg, db, ws = G(M, D), vec(D, init[0]), vec(D, init[1]), _ln_ws(M, D)
    if z is None:
        check(lib.tavsr_layernorm_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(w), ptr(add),
                                      0 if add is None else add.stride(0), ptr(dx.v), D + 8, ptr(dg.v), ptr(db.v), accumulate, ptr(ws),
                                      M, D, stream()), "tavsr_layernorm_bwd")
    else:
        from tavsr._lib import ACT
        check(lib.tavsr_layernorm_bwd_act(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(w), ptr(dx.v), D + 8,
                                          ptr(dg.v), ptr(db.v), accumulate, ptr(ws), M, D, ptr(z), z.stride(0), ACT["gelu"], stream()),
              "tavsr_layernorm_bwd_act")
    return dx, dg, db


@torch.no_grad()
def _ln_device_inputs(M, D, family):
    x, gamma, beta, dy, add, z = RR.ln_inputs(M, D, family)
    return dev_window(x), dev_vec(gamma), dev_vec(beta), dev_window(dy), dev_window(add), dev_window(z)


def _ln_case(M, D, family=False):
    xc, w, b, dyc, addc, zc = _ln_device_inputs(M, D, family)

    def run():
        y, mean, rstd = _ln_fwd(xc, w, b, M, D)
        _, mean_s, rstd_s = _ln_fwd(xc, w, b, M, D, stats_only=True)
        dx, dg, db = _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D)
        dxa, dga, dba = _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D, add=addc)
        dz, dg2, db2 = _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D, z=zc)
        return dict(y=y, mean=mean, rstd=rstd, mean_s=mean_s, rstd_s=rstd_s, dx=dx, dgamma=dg, dbeta=db, dx_add=dxa, dgamma_a=dga,
                    dbeta_a=dba, dz=dz, dgamma2=dg2, dbeta2=db2)
    got = run()
    _same(got, run())
    # the statistics-only forward; the parameter gradients do not depend on dx_add or on the activation
    assert torch.equal(got["mean_s"].v, got["mean"].v) and torch.equal(got["rstd_s"].v, got["rstd"].v)
    for k in ("dgamma", "dbeta"):
        assert torch.equal(got[k + "_a"].v, got[k].v) and torch.equal(got[k + "2"].v, got[k].v)
    ref = RR.ln_refs(M, D, family)
    op, shape, bad = "layernorm" + (" family" if family else ""), f"M={M} D={D}", []
    for name, key, floor, rows in (("y", "y", "ln_fwd", True), ("mean", "mean", "ln_fwd", True), ("rstd", "rstd", "ln_fwd", True),
                                   ("dx", "dx", "ln_bwd", True), ("dgamma", "dgamma", "ln_bwd", False), ("dbeta", "dbeta", "ln_bwd", False),
                                   ("dx_add", "dx_add", "ln_bwd", True), ("dz", "dz", "ln_bwd", True)):
        a, r64, r32 = got[name].v, ref[F64][key], ref[F32][key]
        if family:
            bad += R.check(f"{op} {shape}", name, a, r64, r32, RR.FLOOR[floor], rows=rows)
        else:
            bad += RR.check(op, shape, name, a, r64, r32, RR.FLOOR[floor])
    _finish(bad)
    return got


@pytest.mark.parametrize("D,family", [(D, False) for D in RR.LN_WIDTHS] + [(D, True) for D in RR.LN_FAMILY_WIDTHS])
def test_layernorm_widths(D, family):
    """M = 19: every NV, full / part-filled / idle chunks, one lane (tests/test_rowred_host.py says which width is which)"""
    _ln_case(R.M_ROWS, D, family)


@pytest.mark.parametrize("M,D", RR.LN_SHORT + RR.LN_TALL)
def test_layernorm_heights(M, D):
    """one block with idle waves up to two blocks; 8203 rows: 1024 blocks, a second trip of 11 rows (a partial pair in a partial
    block), 1024 partial rows into the reduction.  Rows carry their own offset and scale (rowred_ref.row_tags)."""
    _ln_case(M, D)


@pytest.mark.parametrize("M,D", [(R.M_ROWS, 320), (9, 512), (RR.LN_TALL_M, 64)])
def test_layernorm_backward_accumulates_into_its_parameter_gradients(M, D):
    xc, w, b, dyc, addc, zc = _ln_device_inputs(M, D, False)
    _, mean, rstd = _ln_fwd(xc, w, b, M, D)
    g0, b0 = RR.host_randn(M + D, D) * 3, RR.host_randn(M + D + 1, D) * 3
    ref, bad = RR.ln_refs(M, D), []
    for z in (None, zc):
        plain = _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D, z=z)
        run = lambda: dict(zip(("dx", "dgamma", "dbeta"), _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D, z=z, accumulate=1, init=(g0, b0))))
        got = run()
        _same(got, run())
        assert torch.equal(got["dx"].v, plain[0].v)
        for k, init, p in (("dgamma", g0, plain[1]), ("dbeta", b0, plain[2])):
            assert torch.equal(got[k].v, init.cuda() + p.v)                        # one float32 addition on top of the plain result
            bad += RR.check("layernorm accumulate" + (" act" if z is not None else ""), f"M={M} D={D}", k, got[k].v,
                            init.double() + ref[F64][k], init + ref[F32][k], RR.FLOOR["ln_bwd"])
    _finish(bad)


@pytest.mark.parametrize("M,D", RR.LN_DROP)
def test_layernorm_backward_masked_copy_beyond_the_encoder_shapes(M, D):
    """tavsr_layernorm_bwd_partial_drop at NV = 2 and on a second trip: dx as the plain call's, dx_drop = ops.dropout(dx, p, token),
    bit for bit (as test_layernorm_backward_masked_copy_is_the_dropout_kernels at D = 256 / 1024, M <= 3168)"""
    from tavsr import ops
    x, gamma, beta, dy, add, _ = RR.ln_inputs(M, D)
    xc, w, b, dyc, addc = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), add.cuda()
    mean, rstd = ops.layernorm_fwd(xc, w, b, R.EPS)[1:]
    ops.manual_seed(11)
    tok = ops._new_token(0.1, M * D, xc.device)
    ref = ops.layernorm_bwd(dyc, xc, mean, rstd, w, dx_add=addc)
    want = ops.dropout(ref[0], 0.1, token=tok)[0]
    assert 0.05 < float((want == 0).float().mean()) < 0.15
    keep = ops.LN_BWD_DROP
    try:
        ops.LN_BWD_DROP = True

        def run():
            lng = ops.LNGroup(cap=2)
            dx, g1, g2, dxd = lng.bwd(dyc, xc, mean, rstd, w, dx_add=addc, drop=tok)
            lng.flush()
            return dict(dx=dx, dgamma=g1.clone(), dbeta=g2.clone(), dx_drop=dxd)
        got = run()
        _same(got, run())
    finally:
        ops.LN_BWD_DROP = keep
    for k, r in zip(("dx", "dgamma", "dbeta"), ref):
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], r), k
    assert bool(torch.isfinite(got["dx_drop"]).all()) and torch.equal(got["dx_drop"], want)
    r64 = RR.ln_refs(M, D)
    _finish(RR.check("layernorm partial_drop", f"M={M} D={D}", "dx_add", got["dx"], r64[F64]["dx_add"], r64[F32]["dx_add"], RR.FLOOR["ln_bwd"]))


@pytest.mark.parametrize("M,D", [(R.M_ROWS, 320), (RR.LN_TALL_M, 512)])
def test_layernorm_partials_in_a_shared_slab_and_their_strided_reduction(M, D):
    """tavsr_layernorm_bwd_partial into columns [2D, 4D) of a slab whose rows hold 3 x 2D (+ 4) floats, as LNGroup lays several
    LayerNorms side by side; tavsr_sum_partials with stride > n over that window.  The slab's other columns stay NaN."""
    lib, ptr, stream, check = _api()
    xc, w, b, dyc, addc, zc = _ln_device_inputs(M, D, False)
    _, mean, rstd = _ln_fwd(xc, w, b, M, D)
    nb = lib.tavsr_layernorm_bwd_ws(M, D) // (2 * D)
    assert nb == RR.ln_blocks(M)
    ld = 6 * D + 4

    def run():
        slab, dx, out = G(nb, 2 * D, ld=ld, off=2 * D), G(M, D), vec(2 * D)
        check(lib.tavsr_layernorm_bwd_partial(ptr(dyc), dyc.stride(0), ptr(xc), xc.stride(0), ptr(mean.v), ptr(rstd.v), ptr(w), None, 0,
                                              ptr(dx.v), D + 8, ptr(slab.v), ld, M, D, stream()), "tavsr_layernorm_bwd_partial")
        check(lib.tavsr_sum_partials(ptr(slab.v), nb, ld, ptr(out.v), 2 * D, 0, stream()), "tavsr_sum_partials")
        return dict(slab=slab, dx=dx, out=out)
    got = run()
    _same(got, run())
    plain = _ln_bwd(dyc, xc, mean.v, rstd.v, w, M, D)
    assert torch.equal(got["dx"].v, plain[0].v)
    assert torch.equal(got["out"].v[:D], plain[1].v) and torch.equal(got["out"].v[D:], plain[2].v)
    ref, bad = RR.ln_refs(M, D), []
    for k, a in (("dgamma", got["out"].v[:D]), ("dbeta", got["out"].v[D:])):
        bad += RR.check("layernorm shared slab", f"M={M} D={D}", k, a, ref[F64][k], ref[F32][k], RR.FLOOR["ln_bwd"])
    _finish(bad)


# ================================================================================================ column sums
@pytest.mark.parametrize("M,N", RR.COLSUM_CASES)
def test_colsum_and_add2_colsum(M, N):
    from tavsr import ops
    x, y = RR.colsum_inputs(M, N)
    xc, yc = dev_window(x, pad=3), dev_window(y, pad=5)              # row strides N + 6 and N + 10
    out0 = RR.host_randn(M + N, N) * 2

    def run():
        s1 = vec(N)
        ops.colsum(xc, out=s1.v)
        s2 = vec(N, init=out0)
        ops.colsum(xc, scale=0.5, out=s2.v, accumulate=True)
        o = G(M, N, off=2)                                            # row stride N + 4
        sx, sy = ops.add2_colsum(xc, yc, o.v)
        o2 = G(M, N, off=2)
        lx, ly, reduce = ops.add2_colsum(xc, yc, o2.v, lazy_sums=True)
        reduce()
        return dict(colsum=s1, scaled=s2, out=o, sum_x=sx, sum_y=sy, out_lazy=o2, lazy_x=lx, lazy_y=ly)
    got = run()
    _same(got, run())
    assert torch.equal(got["out"].v, xc + yc) and torch.equal(got["out_lazy"].v, xc + yc)
    assert torch.equal(got["lazy_x"], got["sum_x"]) and torch.equal(got["lazy_y"], got["sum_y"])
    (_, sx64, sy64), (_, sx32, sy32) = RR.add2_colsum(x, y, F64), RR.add2_colsum(x, y, F32)
    shape, f, bad = f"M={M} N={N}", RR.FLOOR["colsum"], []
    bad += RR.check("colsum", shape, "sum", got["colsum"].v, RR.colsum(x, F64), RR.colsum(x, F32), f)
    bad += RR.check("colsum scale,accum", shape, "sum", got["scaled"].v, RR.colsum(x, F64, 0.5, out0), RR.colsum(x, F32, 0.5, out0), f)
    bad += RR.check("add2_colsum", shape, "sum_x", got["sum_x"], sx64, sx32, f)
    bad += RR.check("add2_colsum", shape, "sum_y", got["sum_y"], sy64, sy32, f)
    _finish(bad)


@pytest.mark.parametrize("nparts", RR.SUM_NPARTS)
def test_sum_partials_around_the_wave_deal_and_the_unroll(nparts):
    lib, ptr, stream, check = _api()
    bad = []
    for n in RR.SUM_N:
        for stride in (n, n + RR.SUM_PAD):
            part = torch.full((nparts, stride), NAN)
            part[:, :n] = RR.host_randn(nparts + n, nparts, n) + 0.5
            pc, o0 = part.cuda(), RR.host_randn(n, n)
            for acc in (0, 1):
                def run():
                    out = vec(n, init=o0 if acc else None)
                    check(lib.tavsr_sum_partials(ptr(pc), nparts, stride, ptr(out.v), n, acc, stream()), "tavsr_sum_partials")
                    return dict(out=out)
                got = run()
                _same(got, run())
                r64, r32 = (RR.sum_partials(part, n, 0, dt, (o0, o0[:0]) if acc else None)[0] for dt in (F64, F32))
                bad += RR.check("sum_partials" + (" accum" if acc else ""), f"p={nparts} n={n} ld={stride}", "out", got["out"].v, r64, r32,
                                RR.FLOOR["colsum"])
    for n1, n2 in RR.SUM_SPLITS:
        n = n1 + n2
        for stride in (n, n + RR.SUM_PAD):
            part = torch.full((nparts, stride), NAN)
            part[:, :n] = RR.host_randn(nparts + n + 7, nparts, n) - 0.5
            pc, o1, o2 = part.cuda(), RR.host_randn(n1 + 1, max(n1, 1))[:n1], RR.host_randn(n2 + 2, max(n2, 1))[:n2]
            for acc in (0, 1):
                def run():
                    a, b = part_vec(n1, o1 if acc else None), part_vec(n2, o2 if acc else None)
                    check(lib.tavsr_sum_partials2(ptr(pc), nparts, stride, ptr(a.v), n1, ptr(b.v), n2, acc, stream()), "tavsr_sum_partials2")
                    return dict(out1=a, out2=b)
                got = run()
                _same(got, run())
                (a64, b64), (a32, b32) = (RR.sum_partials(part, n1, n2, dt, (o1, o2) if acc else None) for dt in (F64, F32))
                shape = f"p={nparts} {n1}+{n2} ld={stride}"
                if n1:
                    bad += RR.check("sum_partials2" + (" accum" if acc else ""), shape, "out1", got["out1"].v[:n1], a64, a32, RR.FLOOR["colsum"])
                if n2:
                    bad += RR.check("sum_partials2" + (" accum" if acc else ""), shape, "out2", got["out2"].v[:n2], b64, b32, RR.FLOOR["colsum"])
    _finish(bad)


# ================================================================================================ empty inputs
@pytest.mark.parametrize("N", [1, 65])
def test_colsum_of_no_rows_is_the_empty_sum(N):
    """M = 0: out = scale * 0, or out as it was under ``accumulate``; tavsr_colsum_ws(0, N) is 0 floats and none is written"""
    lib, ptr, stream, check = _api()
    assert lib.tavsr_colsum_ws(0, N) == 0
    x = torch.full((4, N), NAN, device="cuda")                        # a real address; no row of it belongs to the input
    o0 = RR.host_randn(N, N)
    for acc in (0, 1):
        ws, out = G(1, 2 * N + 64), vec(N, init=o0 if acc else None)
        check(lib.tavsr_colsum(ptr(x), N, 0, N, 0.5, ptr(out.v), acc, ptr(ws.v), stream()), "tavsr_colsum")
        out.ok("out"), ws.untouched("workspace")
        assert torch.equal(out.v, o0.cuda() if acc else torch.zeros(N, device="cuda"))


@pytest.mark.parametrize("D", [64, 512])
def test_layernorm_backward_of_no_rows_gives_zero_parameter_gradients(D):
    lib, ptr, stream, check = _api()
    assert lib.tavsr_layernorm_bwd_ws(0, D) == 0
    from tavsr._lib import ACT
    w = dev_vec(R.affine(D)[0])
    g0, b0 = RR.host_randn(D, D), RR.host_randn(D + 1, D)
    for act in (False, True):
        for acc in (0, 1):
            rows, stat = G(2, D), vec(8)                               # real addresses for dy / x / z / dx and mean / rstd: never touched
            dg, db, ws = vec(D, init=g0 if acc else None), vec(D, init=b0 if acc else None), G(1, 4 * D)
            p, ld = ptr(rows.v), D + 8
            if act:
                rc = lib.tavsr_layernorm_bwd_act(p, ld, p, ld, ptr(stat.v), ptr(stat.v), ptr(w), p, ld, ptr(dg.v), ptr(db.v), acc, ptr(ws.v), 0, D,
                                                 p, ld, ACT["gelu"], stream())
            else:
                rc = lib.tavsr_layernorm_bwd(p, ld, p, ld, ptr(stat.v), ptr(stat.v), ptr(w), None, 0, p, ld, ptr(dg.v), ptr(db.v), acc, ptr(ws.v),
                                             0, D, stream())
            check(rc, "tavsr_layernorm_bwd, M = 0")
            dg.ok("dgamma"), db.ok("dbeta"), rows.untouched("dx"), ws.untouched("workspace"), stat.untouched("statistics")
            zero = torch.zeros(D, device="cuda")
            assert torch.equal(dg.v, g0.cuda() if acc else zero) and torch.equal(db.v, b0.cuda() if acc else zero)


# ================================================================================================ softmax
def _rows_padded(t, ld, fill=NAN):
    """host [..., n] -> device [rows, ld] with ``fill`` in the padding columns"""
    n = t.shape[-1]
    b = torch.full((t.numel() // n, ld), fill)
    b[:, :n] = t.reshape(-1, n)
    return b.cuda()


def _softmax_geometry(c, padded):
    T1, T2 = c["T1"], c["T2"]
    W = 2 * T1 - 1 if c["rel"] else 0
    ld_s = RR.pad4(T2) + 4 if padded else T2
    ld_w = (RR.pad4(W) + 4 if padded else W) if c["rel"] else 0
    return c["H"], c["B"], T1, T2, W, ld_s, ld_w


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("key", range(len(RR.SOFTMAX_CASES)), ids=[RR.softmax_id(c) for c in RR.SOFTMAX_CASES])
def test_softmax_forward_and_backward(key, padded):
    """header contract of the padding columns: attn, ds and ds_skew leave theirs untouched (the NaN stays); the inputs' hold NaN"""
    lib, ptr, stream, check = _api()
    c = RR.SOFTMAX_CASES[key]
    H, B, T1, T2, W, ld_s, ld_w = _softmax_geometry(c, padded)
    rows = H * B * T1
    ac, bd, da = RR.softmax_inputs(key)
    acc, dac = _rows_padded(ac, ld_s), _rows_padded(da, ld_s)
    bdc = _rows_padded(bd, ld_w) if c["rel"] else None
    kl = torch.tensor(c["klens"], dtype=torch.int64, device="cuda")
    scale = RR.SOFTMAX_SCALE

    def run():
        attn = G(rows, T2, ld=ld_s, off=0)
        check(lib.tavsr_softmax_fwd(ptr(acc), ptr(bdc), ptr(kl), ptr(attn.v), H, B, T1, T2, W, ld_s, ld_w, scale, int(c["causal"]), stream()),
              "tavsr_softmax_fwd")
        out = dict(attn=attn)
        for skew in ((True, False) if c["rel"] else (False,)):
            ds = G(rows, T2, ld=ld_s, off=0)
            sk = G(rows, W, ld=ld_w, off=0) if skew else None
            check(lib.tavsr_softmax_bwd(ptr(attn.v), ptr(dac), ptr(ds.v), ptr(sk.v) if skew else None, H, B, T1, T2, W if skew else 0, ld_s,
                                        ld_w if skew else 0, scale, stream()), "tavsr_softmax_bwd")
            out["ds_skewed" if skew else "ds"] = ds
            if skew:
                out["ds_skew"] = sk
        return out
    got = run()
    _same(got, run())
    ref = RR.softmax_refs(key)
    attn = got["attn"].v.reshape(H, B, T1, T2)
    dead = ~RR.softmax_valid(c["klens"], T1, T2, c["causal"])[None].expand(H, B, T1, T2)
    assert bool((attn.cpu()[dead] == 0).all())                                      # exactly 0 on masked keys; klens = 0: a row of zeros
    shape = f"{RR.softmax_id(c)}{' pad' if padded else ''}"
    bad = RR.check("softmax_fwd", shape, "attn", attn, ref[F64][0], ref[F32][0], RR.FLOOR["softmax_fwd"])
    bad += RR.check("softmax_bwd", shape, "ds", got["ds"].v.reshape(H, B, T1, T2), ref[F64][1], ref[F32][1], RR.FLOOR["softmax_bwd"])
    if c["rel"]:
        assert torch.equal(got["ds_skewed"].v, got["ds"].v)
        bad += RR.check("softmax_bwd", shape, "ds_skew", got["ds_skew"].v.reshape(H, B, T1, W), ref[F64][2], ref[F32][2], RR.FLOOR["softmax_bwd"])
    _finish(bad)


@pytest.mark.parametrize("rel", [True, False], ids=["rel", "plain"])
@pytest.mark.parametrize("T1,T2,ld_s", RR.SOFTMAX_DROP_SHAPES)
def test_softmax_with_fused_dropout_on_padded_rows(T1, T2, ld_s, rel):
    """tavsr_softmax_dropout_fwd / _bwd == softmax_fwd -> dropout and dropout -> softmax_bwd with the same token, bit for bit, on rows
    padded by 3, 3, 3 and 8 floats; pv's padding columns come back 0, attn's / ds's / ds_skew's untouched"""
    from tavsr import ops
    lib, ptr, stream, check = _api()
    H, B, p, scale = 2, 3, 0.1, RR.SOFTMAX_SCALE
    W = 2 * T1 - 1 if rel else 0
    ld_w = RR.pad4(W) + 4 if rel else 0
    rows = H * B * T1
    acc = _rows_padded(RR.host_randn(T1 + ld_s, H, B, T1, T2) * 4, ld_s)
    bdc = _rows_padded(RR.host_randn(T1 + ld_s + 1, H, B, T1, W) * 4, ld_w) if rel else None
    dpv = _rows_padded(RR.host_randn(T1 + ld_s + 2, H, B, T1, T2), ld_s)
    kl = torch.tensor([T2, T2 - 1, T2 + 5], dtype=torch.int64, device="cuda")[[2, 1, 0]]      # (T2 + 5 first; T2 = 1: a klens of 0)
    nanbuf = lambda ld: torch.full((rows, ld), NAN, device="cuda")
    ops.manual_seed(77)
    tok = ops._new_token(p, rows * ld_s, acc.device)

    attn = nanbuf(ld_s)
    check(lib.tavsr_softmax_fwd(ptr(acc), ptr(bdc), ptr(kl), ptr(attn), H, B, T1, T2, W, ld_s, ld_w, scale, 0, stream()), "tavsr_softmax_fwd")
    pv = ops.dropout(attn, p, token=tok)[0]

    def fwd():
        a, v = nanbuf(ld_s), nanbuf(ld_s)
        check(lib.tavsr_softmax_dropout_fwd(ptr(acc), ptr(bdc), ptr(kl), ptr(a), ptr(v), H, B, T1, T2, W, ld_s, ld_w, scale, 0, tok[0],
                                            ptr(tok[2]), tok[1], stream()), "tavsr_softmax_dropout_fwd")
        return dict(attn=a, pv=v)
    got = fwd()
    _same(got, fwd())
    assert bool(torch.isfinite(attn[:, :T2]).all())
    assert torch.equal(got["attn"][:, :T2], attn[:, :T2]) and torch.equal(got["pv"][:, :T2], pv[:, :T2])
    assert bool((got["attn"][:, T2:].view(torch.int32) == NAN_BITS).all()) and bool((got["pv"][:, T2:] == 0).all())
    if rows * T2 >= 1000:
        kept = float((pv[:, :T2] != 0).sum()) / float((attn[:, :T2] != 0).sum())
        assert 0.85 < kept < 0.95

    def bwd(fused):
        ds, sk = nanbuf(ld_s), nanbuf(ld_w) if rel else None
        if fused:
            check(lib.tavsr_softmax_dropout_bwd(ptr(attn), ptr(dpv), ptr(ds), ptr(sk), H, B, T1, T2, W, ld_s, ld_w, scale, tok[0], ptr(tok[2]),
                                                tok[1], stream()), "tavsr_softmax_dropout_bwd")
        else:
            check(lib.tavsr_softmax_bwd(ptr(attn), ptr(ops.dropout(dpv, p, token=tok)[0]), ptr(ds), ptr(sk), H, B, T1, T2, W, ld_s, ld_w, scale,
                                        stream()), "tavsr_softmax_bwd")
        return dict(ds=ds, **(dict(ds_skew=sk) if rel else {}))
    got, want = bwd(True), bwd(False)
    _same(got, bwd(True))
    _same(got, want)                                                                # live columns and padding alike
    assert bool(torch.isfinite(got["ds"][:, :T2]).all()) and bool((got["ds"][:, T2:].view(torch.int32) == NAN_BITS).all())
    if rel:
        assert bool(torch.isfinite(got["ds_skew"][:, :W]).all()) and bool((got["ds_skew"][:, W:].view(torch.int32) == NAN_BITS).all())


# ================================================================================================ elementwise glue
def _guarded_vec(t, off):
    """host vector -> device view ``off`` floats into a NaN-filled buffer (off = 4: 16-byte aligned, 5: one float past)"""
    b = torch.full((t.numel() + 12,), NAN)
    b[off:off + t.numel()] = t
    return b.cuda()[off:off + t.numel()]


@pytest.mark.parametrize("n", RR.AXPBY_N)
def test_axpby_vector_kernel_tail_and_scalar_kernel(n):
    from tavsr import ops
    x, y = RR.host_randn(n, n), RR.host_randn(n + 1, n)
    bad = []
    for off in (4, 5):                                                              # aligned: float4 lanes + scalar tail; else the scalar kernel
        xc, yc = _guarded_vec(x, off), _guarded_vec(y, 4)
        assert (xc.data_ptr() % 16 == 0) == (off == 4) and yc.data_ptr() % 16 == 0
        for with_y in (True, False):
            def run():
                out = vec(n)
                assert out.v.data_ptr() % 16 == 0
                ops.axpby(xc, yc if with_y else None, 0.75, -1.5, out=out.v)
                return dict(out=out)
            got = run()
            _same(got, run())
            r64, r32 = (RR.axpby(x, y if with_y else None, 0.75, -1.5, dt) for dt in (F64, F32))
            bad += RR.check("axpby" + ("" if with_y else " no y"), f"n={n} off={off - 4}", "out", got["out"].v, r64, r32, RR.FLOOR["elementwise"])
    _finish(bad)


def _act_bwd_names():
    """the activations tavsr_act_bwd accepts: _lib.ACT's names, less those the entry itself refuses (which must write nothing)"""
    from tavsr import _lib
    lib, ptr, stream, _ = _api()
    z, names = torch.zeros(8, device="cuda"), []
    for name, code in _lib.ACT.items():
        if name is None:
            continue
        out = vec(8)
        rc = lib.tavsr_act_bwd(ptr(z), ptr(z), ptr(out.v), 8, code, stream())
        if rc == 0:
            names.append(name)
        else:
            assert rc == _lib.ENUMS["TAVSR_EUNSUPPORTED"], (name, rc)
            out.untouched(name)
    return names


@pytest.mark.parametrize("n", RR.AXPBY_N)
def test_act_bwd_every_accepted_activation(n):
    from tavsr import _lib, ops
    lib, ptr, stream, check = _api()
    names = _act_bwd_names()
    assert {"none", "relu", "swish", "gelu"} <= set(names)
    dh, z = RR.act_inputs(n)
    dhc, zc = _guarded_vec(dh, 4), _guarded_vec(z, 4)
    bad = []
    for act in names:
        def run():
            out = vec(n)
            check(lib.tavsr_act_bwd(ptr(dhc), ptr(zc), ptr(out.v), n, _lib.ACT[act], stream()), "tavsr_act_bwd")
            return dict(out=out)
        got = run()
        _same(got, run())
        assert torch.equal(ops.act_bwd_(dhc.clone(), zc.clone(), act), got["out"].v)    # the wrapper's in-place form
        bad += RR.check(f"act_bwd {act}", f"n={n}", "dz", got["out"].v, RR.act_bwd(dh, z, act, F64), RR.act_bwd(dh, z, act, F32),
                        RR.FLOOR["elementwise"])
    _finish(bad)


@pytest.mark.parametrize("n", RR.SCALE_DEV_N)
def test_scale_dev_up_to_and_beyond_its_grid_cap(n):
    lib, ptr, stream, check = _api()
    x, s = RR.host_randn(n % 1000, n) + 3.0, torch.tensor([0.37])                   # |x| away from 0: an element left unscaled shows
    xc, sc = _guarded_vec(x, 4), s.cuda()

    def run():
        out = vec(n)
        check(lib.tavsr_scale_dev(ptr(xc), ptr(sc), 2.0, ptr(out.v), n, stream()), "tavsr_scale_dev")
        return dict(out=out)
    got = run()
    _same(got, run())
    _finish(RR.check("scale_dev", f"n={n}", "out", got["out"].v, RR.scale_dev(x, s, 2.0, F64), RR.scale_dev(x, s, 2.0, F32),
                     RR.FLOOR["elementwise"]))


@pytest.mark.parametrize("N", RR.ROWS2D_N)
@pytest.mark.parametrize("M", RR.ROWS2D_M)
def test_axpby2d_and_add_head_bias_on_strided_rows(M, N):
    from tavsr import ops
    lib, ptr, stream, check = _api()
    x, y = RR.host_randn(M + N, M, N), RR.host_randn(M + N + 1, M, N)
    u, v = RR.host_randn(N, N), RR.host_randn(N + 1, N)
    xc, yc, uc, vc = dev_window(x, pad=4), dev_window(y, pad=8), dev_vec(u), dev_vec(v)

    def run():
        o, o1 = G(M, N, off=12), G(M, N)
        ops.axpby2d(xc, yc, 0.75, -1.5, o.v)
        ops.axpby2d(xc, None, 3.0, 0.0, o1.v)
        qu, qv = G(M, N, off=0), G(M, N, off=0)                                     # contiguous [M, N]: guard rows above and below
        check(lib.tavsr_add_head_bias(ptr(xc), xc.stride(0), ptr(uc), ptr(vc), ptr(qu.v), ptr(qv.v), M, N, stream()), "tavsr_add_head_bias")
        return dict(axpby2d=o, ax=o1, qu=qu, qv=qv)
    got = run()
    _same(got, run())
    shape, f, bad = f"M={M} N={N}", RR.FLOOR["elementwise"], []
    bad += RR.check("axpby2d", shape, "out", got["axpby2d"].v, RR.axpby(x, y, 0.75, -1.5, F64), RR.axpby(x, y, 0.75, -1.5, F32), f)
    bad += RR.check("axpby2d no y", shape, "out", got["ax"].v, RR.axpby(x, None, 3.0, 0.0, F64), RR.axpby(x, None, 3.0, 0.0, F32), f)
    (qu64, qv64), (qu32, qv32) = RR.add_head_bias(x, u, v, F64), RR.add_head_bias(x, u, v, F32)
    bad += RR.check("add_head_bias", shape, "qu", got["qu"].v, qu64, qu32, f)
    bad += RR.check("add_head_bias", shape, "qv", got["qv"].v, qv64, qv32, f)
    _finish(bad)


# ================================================================================================ refusals
def _refused(code, rc, *outputs):
    """the argument check's documented code, and nothing written (the check returns before any launch)"""
    from tavsr import _lib
    assert rc == _lib.ENUMS[code], (code, rc)
    torch.cuda.synchronize()
    for o in outputs:
        o.untouched(code)


def test_refusals_return_their_code_and_write_nothing():
    lib, ptr, stream, _ = _api()
    M, N = 3, 8
    src = torch.zeros(M + 1, 1048, device="cuda")
    s, p1 = ptr(src), ptr(src.view(-1)[1:])                                         # aligned, and one float past
    for n, ldx, ldo, xp in ((6, 16, 24, s), (8, 18, 24, s), (8, 16, 18, s), (8, 16, 24, p1)):      # N % 4, ld % 4 (in, out), pointer
        o = G(M, 16, ld=24, off=0)
        _refused("TAVSR_EALIGN", lib.tavsr_axpby2d(xp, ldx, s, 16, 1.0, 1.0, ptr(o.v), ldo, M, n, stream()), o)
    for n, ldq, qp in ((6, 16, s), (8, 18, s), (8, 16, p1)):
        qu, qv = G(M, 16, off=0), G(M, 16, off=0)
        _refused("TAVSR_EALIGN", lib.tavsr_add_head_bias(qp, ldq, s, s, ptr(qu.v), ptr(qv.v), M, n, stream()), qu, qv)
    o = G(1, 16, off=0)
    _refused("TAVSR_EALIGN", lib.tavsr_axpby2d(s, 16, s, 16, 1.0, 1.0, ptr(o.v) + 4, 24, 1, N, stream()), o)          # a misaligned output
    _refused("TAVSR_EALIGN", lib.tavsr_act_bwd(p1, s, ptr(o.v), N, 1, stream()), o)
    for D in RR.LN_REFUSED_D:
        y, dx, mean, rstd, dg, db, ws = G(M, 1040, off=0), G(M, 1040, off=0), vec(M), vec(M), vec(1040), vec(1040), G(1, 8 * 1040)
        _refused("TAVSR_EUNSUPPORTED", lib.tavsr_layernorm_fwd(s, 1048, s, s, R.EPS, ptr(y.v), 1040, ptr(mean.v), ptr(rstd.v), M, D, stream()),
                 y, mean, rstd)
        _refused("TAVSR_EUNSUPPORTED", lib.tavsr_layernorm_bwd(s, 1048, s, 1048, s, s, s, None, 0, ptr(dx.v), 1040, ptr(dg.v), ptr(db.v), 0,
                                                              ptr(ws.v), M, D, stream()), dx, dg, db, ws)
        _refused("TAVSR_EUNSUPPORTED", lib.tavsr_layernorm_bwd_act(s, 1048, s, 1048, s, s, s, ptr(dx.v), 1040, ptr(dg.v), ptr(db.v), 0, ptr(ws.v),
                                                                  M, D, s, 1048, 3, stream()), dx, dg, db, ws)
    y, mean, rstd = G(M, 64, off=0), vec(M), vec(M)
    for xp, ldx, ldy in ((p1, 1048, 64), (s, 1046, 64), (s, 1048, 66)):
        _refused("TAVSR_EALIGN", lib.tavsr_layernorm_fwd(xp, ldx, s, s, R.EPS, ptr(y.v), ldy, ptr(mean.v), ptr(rstd.v), M, 64, stream()),
                 y, mean, rstd)
