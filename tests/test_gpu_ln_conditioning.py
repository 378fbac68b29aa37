"""GPU: every kernel that forms LayerNorm statistics, on rows whose mean dwarfs their spread (tests/ln_stats_ref.py: row m =
(randn + r) * s, |r| up to 1000, s from 1e-6 to 1e3, var ~ eps included), each against the float64 reference:
  a. tavsr_layernorm_fwd / _bwd / _bwd_act        csrc/norm.hip      two-pass
  b. tavsr_gemm_ln                                csrc/gemm.hip      the LayerNorm tail, K split and not
  c. tavsr_rowlin with the LayerNorm prologue     csrc/decode.hip    per-wave (mean, M2) of x - pivot, Chan merge
  d. tavsr_ffn2_fwd                               csrc/ffn2.hip      prologue and the ln2 outputs
  e. tavsr_csgu_fwd                               csrc/cgmlp.hip     statistics from the producing GEMM's (sum, M2) tile pairs
                                                                     (csrc/gemm_glds.h; a partial last tile too) and from the
                                                                     statistics launch
  f. tavsr_cgmlp_fwd / _bwd                       csrc/blocks.hip    the production route; what a saved rstd does to gradients
The suite's other LayerNorm inputs are randn (|mean| / std <= 0.3), where every variance formula agrees to rounding.

Every compared quantity is held to max(floor, 4 * e32) in max |a - b| / max |b| per condition group of rows (``R.check``): floor
is the tolerance of the op's existing test, e32 the same measure of the float32 CPU restatement of the REFERENCE against float64
on the same inputs.  Sums over all rows (parameter gradients) have one figure for the tensor.  Each line is printed
(profiles/ln_conditioning.txt keeps a run).  Outputs and workspaces are pre-filled with NaN and must come back finite; a second
identical call is bit-equal."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import ln_stats_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(autouse=True)
def _nan_filled_allocations(monkeypatch):
    """every tensor the ops wrappers allocate (outputs, saved state, workspaces) starts as NaN"""
    def nan_empty(*shape, like=None, dtype=torch.float32, device=None):
        dev = like.device if like is not None else (device if device is not None else "cuda")
        t = torch.empty(shape, dtype=dtype, device=dev)
        return t.fill_(NAN) if t.is_floating_point() else t
    for name in ("tavsr.ops", "tavsr.ops.base", "tavsr.ops.norm", "tavsr.ops.matmul", "tavsr.ops.blocks", "tavsr.ops.search"):
        mod = importlib.import_module(name)
        if hasattr(mod, "empty"):
            monkeypatch.setattr(mod, "empty", nan_empty)


def _host_randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _finish(bad):
    assert not bad, "\n" + "\n".join(line for _, line in bad)


def _same(a, b):
    for p, q in zip(a, b):
        if p is None:
            assert q is None
        else:
            assert bool(torch.isfinite(p).all()) and torch.equal(p, q)


def _gelu_grad(z, dtype):
    zz = z.detach().cpu().to(dtype).requires_grad_(True)
    F.gelu(zz).sum().backward()
    return zz.grad


# ------------------------------------------------------------------------------------------------ a. norm.hip
@pytest.mark.parametrize("D", [64, 256, 1024])       # NV = 1 with idle lanes, 1, 4
def test_layernorm_fwd_bwd_bwd_act(D):
    from tavsr import ops
    M = R.M_ROWS
    buf = _host_randn(D, M, 2 * D)
    buf[:, D:] = R.family(D)
    x = buf.cuda()[:, D:]                              # strided rows: a column window of a [M, 2D] buffer
    gam, bet = R.affine(D)
    dy, z = _host_randn(D + 1, M, D), _host_randn(D + 2, M, D)
    w, b, dyc, zc = gam.cuda(), bet.cuda(), dy.cuda(), z.cuda()

    def run():
        y, mean, rstd = ops.layernorm_fwd(x, w, b, R.EPS)
        dx, dg, db = ops.layernorm_bwd(dyc, x, mean, rstd, w)
        dz, dg2, db2 = ops.layernorm_bwd_act(dyc, x, mean, rstd, w, zc, "gelu")
        return y, mean, rstd, dx, dg, db, dz, dg2, db2
    got = run()
    _same(got, run())
    y, mean, rstd, dx, dg, db, dz, dg2, db2 = got
    xh = buf[:, D:]
    y64, m64, r64 = R.ln_ref64(xh, gam, bet)
    y32, m32, r32 = R.ln_ref32(xh, gam, bet)
    dx64, dg64, db64 = R.ln_bwd_ref(xh, gam, bet, dy, torch.float64)
    dx32, dg32, db32 = R.ln_bwd_ref(xh, gam, bet, dy, torch.float32)
    op, bad = f"layernorm D={D}", []
    for name, a, r64_, r32_, floor, rows in (
            ("y", y, y64, y32, 2e-5, True), ("mean", mean, m64, m32, 2e-5, True), ("rstd", rstd, r64, r32, 2e-5, True),
            ("dx", dx, dx64, dx32, 1e-4, True), ("dgamma", dg, dg64, dg32, 1e-4, False), ("dbeta", db, db64, db32, 1e-4, False),
            ("dz(act)", dz, dx64 * _gelu_grad(z, torch.float64), dx32 * _gelu_grad(z, torch.float32), 1e-4, True),
            ("dgamma2", dg2, dg64, dg32, 1e-4, False), ("dbeta2", db2, db64, db32, 1e-4, False)):
        bad += R.check(op, name, a, r64_, r32_, floor, rows=rows)
    _finish(bad)


# ------------------------------------------------------------------------------------------------ b. gemm.hip LayerNorm tail
@pytest.mark.parametrize("M,N,K", [(35, 128, 2048), (35, 256, 256)])      # K split (LayerNorm in the finishing launch); not split
def test_gemm_layernorm_tail(M, N, K):
    """the conditioning enters through the residual (the family); x W^T is O(1) times the row's own scale s, so that the small-scale
    rows keep their ratio"""
    from tavsr import ops
    res = R.family(N, M=M)
    s = torch.tensor([R.CONDS[int(c)][1] for c in R.cond_of_rows(M)])[:, None]
    x, w = _host_randn(M + K, M, K) * s, _host_randn(N + K, N, K) / K ** 0.5
    gam, bet = R.affine(N)
    xc, wc, rc, gc, bc = x.cuda(), w.cuda(), res.cuda(), gam.cuda(), bet.cuda()
    run = lambda: ops.linear(xc, wc, None, res=rc, ln=(gc, bc, R.EPS))
    got = run()
    _same(got, run())
    y64 = res.double() + x.double() @ w.double().t()
    y32 = res + x @ w.t()
    n64, n32 = R.ln_ref64(y64, gam, bet)[0], R.ln_ref32(y32, gam, bet)[0]
    ratio = R.achieved_ratio(y64)
    for m in range(M):
        r = abs(R.CONDS[m % 8][0])
        assert r == 0 or float(ratio[m]) >= 0.5 * r, (m, float(ratio[m]))
    op = f"gemm_ln M={M} N={N} K={K}"
    _finish(R.check(op, "y", got[0], y64, y32, 2e-6) + R.check(op, "ln(y)", got[1], n64, n32, 5e-6))


# ------------------------------------------------------------------------------------------------ c. decode.hip rowlin prologue
# K = 64: one wave, nothing to merge; 1024: the largest prologue, which the library plans for up to 16 rows (tavsr_rowlin_ok), so
# the 32-row tile is met at K = 64 and 512
@pytest.mark.parametrize("N,K", [(10, 64), (30, 64), (10, 512), (30, 512), (10, 1024), (16, 1024)])
def test_rowlin_layernorm_prologue(N, K):
    from tavsr import ops
    Nout = 96
    x = R.family(K, M=N)
    gam, bet = R.affine(K)
    w, b = _host_randn(N + K, Nout, K) / K ** 0.5, _host_randn(N + K + 1, Nout)
    xc, wc, bc, gc, ec = x.cuda(), w.cuda(), b.cuda(), gam.cuda(), bet.cuda()
    assert ops.rowlin_ok(xc, wc, ln=True)
    run = lambda: (ops.rowlin(xc, wc, bc, ln=(gc, ec, R.EPS)),)
    got = run()
    _same(got, run())
    y64 = R.ln_ref64(x, gam, bet)[0] @ w.double().t() + b.double()
    y32 = R.ln_ref32(x, gam, bet)[0] @ w.t() + b
    _finish(R.check(f"rowlin N={N} K={K}", "y", got[0], y64, y32, 2e-6))


# ------------------------------------------------------------------------------------------------ d. ffn2.hip
def test_ffn2_prologue_and_ln2_outputs():
    from tavsr import ops
    M, N1, D = 32, 1024, 256
    x = R.family(D, M=M)
    ln_w, ln_b = R.affine(D)
    (g2, c2), (g3, c3) = R.affine(D, seed=2), R.affine(D, seed=3)
    w1, b1 = _host_randn(1, N1, D) / D ** 0.5, 0.1 * _host_randn(2, N1)
    w2, b2 = _host_randn(3, D, N1) / N1 ** 0.5, 0.1 * _host_randn(4, D)
    cu = [t.cuda() for t in (x, ln_w, ln_b, w1, b1, w2, b2, g2, c2, g3, c3)]

    def run():
        y, (n, mean, rstd, z, h, _, _), outs, (m2, r2) = ops.ffn2_fwd(cu[0], cu[1], cu[2], R.EPS, cu[3], cu[4], cu[5], cu[6], "relu", 0.5,
                                                                     save=True, ln2=((cu[7], cu[8]), (cu[9], cu[10])), ln2_stats=True)
        return y, n, mean, rstd, outs[0], outs[1], m2, r2
    got = run()
    _same(got, run())

    def ref(dt):
        if dt == torch.float64:
            n, mean, rstd = R.ln_ref64(x, ln_w, ln_b)
        else:
            n, mean, rstd = R.ln_ref32(x, ln_w, ln_b)
        y = x.to(dt) + 0.5 * (torch.relu(n @ w1.to(dt).t() + b1.to(dt)) @ w2.to(dt).t() + b2.to(dt))
        f = R.ln_ref64 if dt == torch.float64 else R.ln_ref32
        o2, m2, r2 = f(y, g2, c2)
        return y, n, mean, rstd, o2, f(y, g3, c3)[0], m2, r2
    r64, r32 = ref(torch.float64), ref(torch.float32)
    bad = []
    for name, floor, a, p, q in zip(("y", "n", "mean", "rstd", "ln2[0]", "ln2[1]", "m2", "r2"),
                                    (5e-6, 2e-6, 2e-6, 2e-6, 1e-5, 1e-5, 1e-5, 1e-5), got, r64, r32):
        bad += R.check("ffn2 M=32 N1=1024", name, a, p, q, floor)
    _finish(bad)


# ------------------------------------------------------------------------------------------------ e. cgmlp.hip CSGU, both routes
def _csgu_ref(g, Cn, B, T, lw, lb, cw, cb, dt):
    """from the g the GEMM produced: gn, conv, u, mean, rstd on the CPU in ``dt``"""
    g = g.detach().cpu().to(dt)
    f = R.ln_ref64 if dt == torch.float64 else R.ln_ref32
    gn, mean, rstd = f(g[:, Cn:], lw, lb)
    conv = F.conv1d(gn.view(B, T, Cn).transpose(1, 2), cw.to(dt), cb.to(dt), 1, 15, 1, Cn).transpose(1, 2).reshape(B * T, Cn)
    return gn, conv, g[:, :Cn] * conv, mean, rstd


@pytest.mark.parametrize("B,T", [(2, 1), (1, 129)])      # one-row utterances; the second time tile of one row
@pytest.mark.parametrize("Cn", [256, 1024])              # 4 and 16 gate tiles per row
def test_csgu_statistics_from_the_gemm_and_from_the_launch(B, T, Cn):
    from tavsr import ops
    M, Kin, K = B * T, 256, 31
    x, w1, b1 = R.cgmlp_inputs(M, Kin, Cn)
    lw, lb = R.affine(Cn)
    cw, cb = _host_randn(Cn, Cn, 1, K) / 5, _host_randn(Cn + 1, Cn)
    xc, w1c, b1c, lwc, lbc, cwc, cbc = (t.cuda() for t in (x, w1, b1, lw, lb, cw, cb))

    def run():
        rst = torch.full((M, 2 * Cn // 64, 2), NAN, device="cuda")
        g = ops.linear(xc, w1c, b1c, act="gelu", rowstat=rst)
        a = ops.csgu_fwd(g, lwc, lbc, R.EPS, cwc.view(Cn, K), cbc, B, T, save=True, rowstat=rst)[:5]
        b = ops.csgu_fwd(g, lwc, lbc, R.EPS, cwc.view(Cn, K), cbc, B, T, save=True, rowstat=None)[:5]
        return (g, rst) + tuple(a) + tuple(b)
    got = run()
    _same(got, run())
    g, rst = got[:2]
    ratio = R.achieved_ratio(g[:, Cn:])
    for m in range(M):                                   # the inputs did not quietly degrade to randn
        r = abs(R.CONDS[m % 8][0])
        assert r == 0 or float(ratio[m]) >= 0.5 * r, (m, float(ratio[m]))
    r64, r32 = _csgu_ref(g, Cn, B, T, lw, lb, cw, cb, torch.float64), _csgu_ref(g, Cn, B, T, lw, lb, cw, cb, torch.float32)
    op, bad = f"csgu B={B} T={T} Cn={Cn}", []
    # the documented pair (include/tavsr.h, tavsr_gemm_desc.rowstat) of every tile
    p64, p32 = R.rowstat_pairs(g, torch.float64), R.rowstat_pairs(g)
    bad += R.check(op, "pair.sum", rst[..., 0], p64[..., 0], p32[..., 0], 1e-5)
    bad += R.check(op, "pair.M2", rst[..., 1], p64[..., 1], p32[..., 1], 1e-5)
    names = ("u", "conv", "gn", "mean", "rstd")          # csgu_fwd's order
    order = dict(gn=0, conv=1, u=2, mean=3, rstd=4)      # _csgu_ref's
    for route, outs in (("gemm", got[2:7]), ("launch", got[7:12])):
        for name, a in zip(names, outs):
            bad += R.check(f"{op} {route}", name, a, r64[order[name]], r32[order[name]], 2e-5)
    for name, a, b in zip(names, got[2:7], got[7:12]):   # the two routes against each other
        bad += R.check(f"{op} gemm~launch", name, a, r64[order[name]], r32[order[name]], 2e-5, against=b)
    _finish(bad)


def test_rowstat_pair_of_a_partial_last_tile():
    """N = 200: three whole tiles and one of 8 columns, whose M2 is about the mean of those 8 (the general-count form of the
    pair; tavsr_csgu_fwd itself takes whole tiles only, C % 64 == 0)"""
    from tavsr import ops
    M, N, K = R.M_ROWS, 200, 64
    res = R.family(N)
    s = torch.tensor([R.CONDS[int(c)][1] for c in R.cond_of_rows(M)])[:, None]
    x, w = _host_randn(3, M, K) * s, _host_randn(4, N, K) / K ** 0.5
    xc, wc, rc = x.cuda(), w.cuda(), res.cuda()

    def run():
        rst = torch.full((M, 4, 2), NAN, device="cuda")
        return ops.linear(xc, wc, None, res=rc, rowstat=rst), rst
    got = run()
    _same(got, run())
    y, rst = got
    assert torch.equal(y, ops.linear(xc, wc, None, res=rc))
    p64, p32 = R.rowstat_pairs(y, torch.float64), R.rowstat_pairs(y)
    op = "gemm rowstat N=200"
    _finish(R.check(op, "pair.sum", rst[..., 0], p64[..., 0], p32[..., 0], 1e-5) + R.check(op, "pair.M2", rst[..., 1], p64[..., 1], p32[..., 1], 1e-5))


# ------------------------------------------------------------------------------------------------ f. blocks.hip cgMLP block
def test_cgmlp_block_forward_backward():
    from tavsr import ops
    B, T, D, C2 = 2, 20, 256, 2048
    Cn, M = C2 // 2, B * T
    x, w1, b1 = R.cgmlp_inputs(M, D, Cn)
    lw, lb = R.affine(Cn)
    cw, cb = 0.2 * _host_randn(5, Cn, 1, 31), 1 + 0.1 * _host_randn(6, Cn)
    w2, b2 = _host_randn(7, D, Cn) / Cn ** 0.5, 0.1 * _host_randn(8, D)
    res, dy = _host_randn(9, M, D), _host_randn(10, M, D)
    prm_h = [w1, b1, lw, lb, cw, cb, w2, b2]
    prm = [t.cuda() for t in prm_h]
    xc, rc, dyc = x.cuda(), res.cuda(), dy.cuda()

    def run():
        out, kept, desc = ops.cgmlp_fwd(xc, *prm, B, T, alpha=0.7, res=rc)
        dx, grads = ops.cgmlp_bwd(desc, dyc, prm)
        return (out, dx, kept[0], kept[3], kept[4]) + tuple(grads)
    got = run()
    _same(got, run())

    def ref(dt):
        P = [q.to(dt).requires_grad_(True) for q in prm_h]
        X = x.to(dt).requires_grad_(True)
        g = F.gelu(X @ P[0].t() + P[1])
        xg = F.layer_norm(g[:, Cn:], (Cn,), P[2], P[3], R.EPS)
        xg = F.conv1d(xg.view(B, T, Cn).transpose(1, 2), P[4], P[5], 1, 15, groups=Cn).transpose(1, 2).reshape(M, Cn)
        out = res.to(dt) + 0.7 * ((g[:, :Cn] * xg) @ P[6].t() + P[7])
        out.backward(dy.to(dt))
        gate = g[:, Cn:].detach()
        return [out.detach(), X.grad, gate] + [q.grad for q in P]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    ratio = R.achieved_ratio(r64[2])
    for m in range(M):
        r = abs(R.CONDS[m % 8][0])
        assert r == 0 or float(ratio[m]) >= 0.5 * r, (m, float(ratio[m]))
    op = "cgmlp block B=2 T=20"
    bad = R.check(op, "out", got[0], r64[0], r32[0], 2e-5) + R.check(op, "dx", got[1], r64[1], r32[1], 1e-4)
    # the saved statistics the backward pass consumed, against the float64 statistics of the float64 gate
    m64, s64 = r64[2].mean(1), 1 / torch.sqrt(r64[2].var(1, unbiased=False) + R.EPS)
    _, m32, s32 = R.ln_ref32(r32[2], lw, lb)
    bad += R.check(op, "g_mean", got[3], m64, m32, 2e-5) + R.check(op, "g_rstd", got[4], s64, s32, 2e-5)
    for name, a, p, q in zip(("g_w1", "g_b1", "g_ln_w", "g_ln_b", "g_cw", "g_cb", "g_w2", "g_b2"), got[5:], r64[3:], r32[3:]):
        bad += R.check(op, name, a, p, q, 2e-4, rows=False)
    _finish(bad)
