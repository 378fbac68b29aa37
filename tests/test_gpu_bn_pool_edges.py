"""The memory-bound half of the lip front-end (csrc/vision.hip: BatchNorm statistics / apply / backward, the max-pool, the fused stem
kernels, the average pool, rsqrt_eps, copy2d, and sum_partials_kernel of csrc/norm.hip) through ``tavsr.ops``, each against the
float64 formulas of tests/bn_pool_ref.py (validated on the host by tests/test_bn_pool_host.py) at the sizes where these kernels
take another path:

1. BatchNorm at every branch of ``chunks = min(max(1, M // 256), 1024)``: fewer rows than the 16 row lanes, one chunk, two, one
   past the 16 groups of the finalize / partial-sum kernels, either side of their four-deep unrolled loops, the 1024-chunk clamp;
   C below one 64-channel block, a block plus four (the dbeta | dgamma split of sum_partials2 inside a block), up to 8 blocks.
   Bars: the project's (y 1e-5 max_rel, running_mean 1e-6, running_var 1e-5, gradients 1e-4 rel_err; mean / rstd 1e-6 / 1e-5).
2. The statistics under bad conditioning (mean >> sigma, a constant column, one row k sigma away - row 0, the kernel's shift sample
   before the accumulators became double, and another row as the control): kernel error <= max(bar, 4 e32), e32 = the error of
   torch's own fp32 BatchNorm1d on the device against the same reference.  Every figure is printed (profiles/bn_pool_edges.txt).
3. Max-pool forward / backward with tied maxima, NaN and maps down to 1 x 1: values, taps and gradients exact.
4. The fused stem kernels against the float64 composition, not against the unfused launches.
5. Eval-mode BatchNorm from the running buffers, rsqrt_eps, the average pool (vector and scalar backward), copy2d.

Two bounds are not the plain bar, both where the reference gradient is a cancellation to (almost) nothing:
- dx of a TWO-row batch: xhat = +-sqrt(var / (var + eps)), so dx = gamma rstd (dz - dbeta/2 - xhat dgamma/2) is eps / var (~1e-6)
  of its terms and fp32 keeps one digit of it, in torch's fp32 BatchNorm as well: max(1e-4, 4 e32), the form of section 2.
- dx of a ONE-row batch (fused stem at N = H = W = 1) is exactly 0 and torch refuses the shape: |dx| <= 1e-4 of the cancelling
  terms gamma rstd |dz|."""
import math

import pytest
import torch

import bn_pool_ref as R
from helpers import max_rel, rel_err

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
BAR = dict(mean=1e-6, rstd=1e-5, y=1e-5, rm=1e-6, rv=1e-5, dz=1e-4, dx=1e-4, dg=1e-4, db=1e-4)
ERR = dict(y=max_rel)                 # everything else: rel_err


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _errors(got, want):
    return {k: ERR.get(k, rel_err)(got[k], want[k]) for k in want if got.get(k) is not None}


# ------------------------------------------------------------------------------------------------ 1. BatchNorm at the block edges
def _bn_inputs(M, C, with_res, seed, x=None):
    g = _gen(seed)
    if x is None:
        x = torch.randn(M, C, generator=g) * 2 + 0.7
    res = torch.randn(M, C, generator=g) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, (torch.rand(C, generator=g) - 0.5) * 0.6
    r = torch.randn(M, C, generator=g)
    return [None if t is None else t.cuda() for t in (x, res, gamma, beta, r)]


def _bn_reference(x, res, gamma, beta, r, act):
    d = [None if t is None else t.double() for t in (x, res, gamma, beta, r)]
    C = x.shape[1]
    rm0, rv0 = torch.zeros(C, dtype=torch.float64, device=x.device), torch.ones(C, dtype=torch.float64, device=x.device)
    y, (mean, var, rstd), (rm, rv, nbt) = R.bn_train_fwd(d[0], d[2], d[3], EPS, MOM, rm0, rv0, 0, d[1], act)
    dz, dx, dg, db = R.bn_bwd(d[4], d[0], mean, rstd, d[2], d[3], d[1], act)
    return dict(mean=mean, rstd=rstd, y=y, rm=rm, rv=rv, dz=dz, dx=dx, dg=dg, db=db), nbt


def _bn_kernels(x, res, gamma, beta, r, act, need_dz=True):
    from tavsr import ops
    C = x.shape[1]
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    mean, rstd = ops.bn_stats(x, EPS, MOM, rm, rv, nbt)
    y = ops.bn_apply_fwd(x, mean, rstd, gamma, beta, res, act)
    dz, dx, dg, db = ops.bn_bwd(r, x, mean, rstd, gamma, beta, res, act, need_dz=need_dz)
    return dict(mean=mean, rstd=rstd, y=y, rm=rm, rv=rv, dz=dz, dx=dx, dg=dg, db=db), int(nbt)


def _bn_torch_fp32(x, res, gamma, beta, r, act):
    """torch's own fp32 BatchNorm1d on the device (+ residual, activation) under autograd: its error against the reference is e32"""
    C = x.shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        _, mean, rstd = torch.native_batch_norm(x, gamma, beta, None, None, True, MOM, EPS)
    xs = x.clone().requires_grad_(True)
    rs = None if res is None else res.clone().requires_grad_(True)
    z = bn(xs) if rs is None else bn(xs) + rs
    y = R.act_fwd(z, act)
    (y * r).sum().backward()
    return dict(mean=mean, rstd=rstd, y=y.detach(), rm=bn.running_mean, rv=bn.running_var, dz=None if rs is None else rs.grad,
                dx=xs.grad, dg=bn.weight.grad, db=bn.bias.grad)


def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if a[k] is not None)


ACTS = [("swish", True), ("swish", False), (None, False)]
SMALL_M, LARGE_M = (2, 9, 511, 513), (4363, 12601, 16411, 16649, 28967, 263001)
BN_CASES = ([(M, 64, a, w) for M in SMALL_M for a, w in ACTS] + [(M, 64, "swish", True) for M in LARGE_M]
            + [(M, C, a, w) for C in (8, 68, 128, 512) for M in (9, 513) for a, w in ACTS]
            + [(M, C, "swish", True) for C in (8, 68, 128, 512) for M in (4363, 16649)])


@pytest.mark.parametrize("M,C,act,with_res", BN_CASES)
def test_batchnorm_at_block_and_partial_edges(M, C, act, with_res):
    inp = _bn_inputs(M, C, with_res, seed=M + C)
    want, nbt_want = _bn_reference(*inp, act)
    got, nbt = _bn_kernels(*inp, act)
    err = _errors(got, want)
    bar = dict(BAR)
    if M == 2:          # dx cancels to eps / var of its terms (module docstring): the e32 form
        e32 = _errors(_bn_torch_fp32(*inp, act), want)
        bar["dx"] = max(BAR["dx"], 4 * e32["dx"])
        print(f"bn M=2 C={C} {act} res={with_res}: dx err {err['dx']:.2e}, e32 {e32['dx']:.2e}")
    print(f"bn M={M} C={C} {act} res={with_res}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    bad = {k: (v, bar[k]) for k, v in err.items() if not v <= bar[k]}
    assert not bad, bad
    assert nbt == nbt_want == 1
    again, _ = _bn_kernels(*inp, act)
    assert _same_bits(got, again)                                   # fixed summation order: run-to-run bit-equal
    if not with_res:    # the pre-activation gradient need not be materialised: same sums, dx from the recomputed dz
        lean, _ = _bn_kernels(*inp, act, need_dz=False)
        assert lean["dz"] is None and torch.equal(lean["dg"], got["dg"]) and torch.equal(lean["db"], got["db"])
        e = rel_err(lean["dx"], want["dx"])
        assert e <= bar["dx"], e


@pytest.mark.parametrize("C", [4, 64, 68])
def test_batchnorm_of_one_row(C):
    """M = 1 (torch refuses it): mean = x, var = 0, rstd = 1 / sqrt(eps), running_var blended with 0, y = act(beta + res)"""
    x, res, gamma, beta, r = _bn_inputs(1, C, True, seed=C)
    want, _ = _bn_reference(x, res, gamma, beta, r, "swish")
    got, nbt = _bn_kernels(x, res, gamma, beta, r, "swish")
    assert torch.equal(got["mean"], x[0]) and nbt == 1
    assert rel_err(got["rstd"], torch.full((C,), 1 / math.sqrt(EPS), dtype=torch.float64, device="cuda")) <= 1e-6
    assert rel_err(got["rm"], MOM * x[0].double()) <= BAR["rm"]
    assert rel_err(got["rv"], torch.full((C,), 1 - MOM, dtype=torch.float64, device="cuda")) <= 1e-6
    assert max_rel(got["y"], want["y"]) <= BAR["y"] and max_rel(got["y"], R.act_fwd((beta + res).double(), "swish")) <= BAR["y"]
    assert rel_err(got["dz"], want["dz"]) <= BAR["dz"] and rel_err(got["db"], want["db"]) <= BAR["db"]
    assert torch.equal(got["dg"], torch.zeros_like(got["dg"])) and bool(torch.isfinite(got["dx"]).all())


# ------------------------------------------------------------------------------------------------ 2. conditioning
def _cond_input(M, C, kind, g):
    """-> x [M, C] fp32 on the host, and the constant columns (or None)"""
    if kind == "mean100_sigma0.01":
        return 100 + 0.01 * torch.randn(M, C, generator=g), None
    x = torch.randn(M, C, generator=g) * 2 + 0.7
    if kind == "constant_columns":
        cols = torch.arange(0, C, 4)
        x[:, cols] = (torch.rand(len(cols), generator=g) * 8 - 4)[None, :]
        return x, cols
    where, k = kind.split("_k")
    row = 0 if where == "row0" else M // 3 + 5
    x[row] = 0.7 + float(k) * 2.0                          # mean + k sigma in every channel
    return x, None


COND_KINDS = (["mean100_sigma0.01", "constant_columns"] + [f"row0_k{k}" for k in (10, 100, 1000)]
              + [f"other_k{k}" for k in (10, 100, 1000)])


@pytest.mark.parametrize("kind", COND_KINDS)
@pytest.mark.parametrize("M", [3001, 16411, 263001])
def test_batchnorm_statistics_under_bad_conditioning(M, kind):
    C = 64
    g = _gen(M)
    x, const_cols = _cond_input(M, C, kind, g)
    inp = _bn_inputs(M, C, True, seed=M + 1, x=x)
    want, _ = _bn_reference(*inp, "swish")
    got, nbt = _bn_kernels(*inp, "swish")
    err, e32 = _errors(got, want), _errors(_bn_torch_fp32(*inp, "swish"), want)
    bad = {}
    for k, v in err.items():
        bound = max(BAR[k], 4 * e32[k])
        ok = v <= bound
        print(f"cond M={M:<6d} {kind:<18s} {k:<4s} kernel {v:.2e}  e32 {e32[k]:.2e}  ratio {v / max(e32[k], 1e-30):9.2f}  "
              f"bound {bound:.1e}  {'ok' if ok else 'FAIL'}")
        if not ok:
            bad[k] = (v, bound)
    assert not bad, bad
    assert nbt == 1 and bool(torch.isfinite(got["dx"]).all())
    if const_cols is not None:          # variance exactly 0: mean is the constant, rstd = 1 / sqrt(eps), running_var = (1 - momentum) * 1
        c = const_cols.cuda()
        assert torch.equal(got["mean"][c], inp[0][0, c])
        assert rel_err(got["rstd"][c], torch.full((len(c),), 1 / math.sqrt(EPS), dtype=torch.float64, device="cuda")) <= 1e-6
        assert float((got["rv"][c].double() - (1 - MOM)).abs().max()) <= 2.0 ** -23
    assert _same_bits(got, _bn_kernels(*inp, "swish")[0])


# ------------------------------------------------------------------------------------------------ 3. max-pool
def _pool_sets(N, H, W, C, g):
    """(name, x, dy is integer): inputs of one map size"""
    yield "randn", torch.randn(N, H, W, C, generator=g), False
    yield "ties", torch.randint(-1, 2, (N, H, W, C), generator=g).float(), True
    yield "relu", torch.randn(N, H, W, C, generator=g).clamp(min=0), False
    x = torch.randn(N, H, W, C, generator=g)
    x[N - 1, H // 2, W // 2, C - 1] = float("nan")
    yield "nan", x, False


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (2, 3), (3, 3), (5, 4), (7, 9), (44, 44)])
def test_maxpool_ties_nan_and_small_maps(H, W):
    from tavsr import ops
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    g = _gen(100 * H + W)
    for N in (1, 3):
        for C in (4, 64, 68):
            for name, x, int_dy in _pool_sets(N, H, W, C, g):
                tag = (name, N, C)
                want, tap = R.maxpool3x3s2_fwd(x.double())
                y, idx_d, ho, wo = ops.maxpool3x3s2_fwd(x.cuda().view(-1, C), N, H, W, C)
                assert (ho, wo) == (Ho, Wo), tag
                y, idx = y.cpu().view(N, Ho, Wo, C), idx_d.cpu().view(N, Ho, Wo, C)
                assert torch.equal(idx.long(), tap), tag
                if name == "nan":       # the NaN is the value of every window that holds it, and those windows select its tap
                    h, w = H // 2, W // 2
                    hit = [(a, b) for a in range(Ho) for b in range(Wo) if abs(2 * a - h) <= 1 and abs(2 * b - w) <= 1]
                    assert hit and int(torch.isnan(y).sum()) == len(hit), tag
                    for a, b in hit:
                        assert math.isnan(float(y[N - 1, a, b, C - 1])) and int(idx[N - 1, a, b, C - 1]) == (h - 2 * a + 1) * 3 + (w - 2 * b + 1), tag
                    assert torch.equal(torch.isnan(y), torch.isnan(want)), tag
                    assert torch.equal(y.double().nan_to_num(nan=0.0), want.nan_to_num(nan=0.0)), tag
                else:
                    assert torch.equal(y.double(), want), tag
                dy = (torch.randint(-3, 4, (N, Ho, Wo, C), generator=g).float() if int_dy else torch.randn(N, Ho, Wo, C, generator=g))
                dwant = R.maxpool3x3s2_bwd(dy.double(), tap, H, W)
                dx = ops.maxpool3x3s2_bwd(dy.cuda().view(-1, C), idx_d, N, H, W, C).cpu().view(N, H, W, C)
                if int_dy:
                    assert torch.equal(dx.double(), dwant), tag
                else:
                    assert max_rel(dx, dwant) <= 1e-6, tag


# ------------------------------------------------------------------------------------------------ 4. fused stem kernels
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 64), (2, 2, 3, 8), (3, 3, 3, 68), (2, 9, 7, 128), (1, 44, 44, 64), (6, 44, 44, 64)])
def test_fused_stem_kernels_against_the_float64_composition(N, H, W, C):
    """bn_act_maxpool3x3s2_fwd against maxpool(swish(BN(x))) in float64; bn_bwd_pooled, with the kernel's own taps, against the
    float64 backward that routes each pooled gradient to that tap.  (6, 44, 44, 64): 45 chunks over 2904 2x2 blocks - blocks_per_wg
    has a tail and the last workgroups are empty."""
    from tavsr import ops
    g = _gen(N * H * W + C)
    M = N * H * W
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.2).cuda()
    mean, rstd = ops.bn_stats(x, EPS, MOM)
    y, idx, Ho, Wo = ops.bn_act_maxpool3x3s2_fwd(x, mean, rstd, gamma, beta, "swish", N, H, W, C)
    x64, g64, b64 = x.double().view(N, H, W, C), gamma.double(), beta.double()
    mean64, _, rstd64 = R.bn_stats(x64.view(-1, C), EPS)
    want, _, amap = R.bn_act_maxpool_fwd(x64, mean64, rstd64, g64, b64, "swish")
    assert (Ho, Wo) == tuple(want.shape[1:3])
    e_y = max_rel(y.view(N, Ho, Wo, C), want)
    # the float64 activation at the tap the kernel chose (out-of-map taps read -inf) against the window's float64 maximum
    tap = idx.view(N, Ho, Wo, C).long()
    assert int(tap.max()) <= 8
    ap = torch.nn.functional.pad(amap, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    chosen = torch.full_like(want, float("nan"))
    for k in range(9):
        kh, kw = divmod(k, 3)
        chosen = torch.where(tap == k, ap[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :], chosen)
    e_tap = float((chosen - want).abs().max() / want.abs().max())
    print(f"stem N={N} H={H} W={W} C={C}: pooled {e_y:.2e}, chosen tap {e_tap:.2e}")
    assert e_y <= 1e-5 and e_tap <= 1e-5
    dp = torch.randn(N, Ho, Wo, C, generator=g).cuda()
    dx, dg, db = ops.bn_bwd_pooled(dp.view(-1, C), idx, x, mean, rstd, gamma, beta, N, H, W, "swish")
    dx_w, dg_w, db_w = R.bn_act_maxpool_bwd(dp.double(), tap, x64, mean64, rstd64, g64, b64, "swish")
    e = dict(dg=rel_err(dg, dg_w), db=rel_err(db, db_w))
    if M == 1:      # dx is exactly 0 (module docstring): against the size of the terms that cancel
        e["dx"] = float(dx.double().abs().max() / (g64 * rstd64 * dp.double().view(-1, C).abs()).max())
    else:
        e["dx"] = rel_err(dx.view(N, H, W, C), dx_w)
    print(f"stem N={N} H={H} W={W} C={C}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= 1e-4 for v in e.values()), e


# ------------------------------------------------------------------------------------------------ 5. eval path, small ops
@pytest.mark.parametrize("C", [8, 64, 512])
def test_eval_batchnorm_from_the_running_buffers(C):
    from tavsr import ops
    g = _gen(C)
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).cuda().double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for M in (300, 517):
        xb = (torch.randn(M, C, generator=g) * 3 - 1).cuda()
        bn(xb.double())
        ops.bn_stats(xb, EPS, MOM, rm, rv, nbt)
    assert int(nbt) == int(bn.num_batches_tracked) == 2
    assert rel_err(rm, bn.running_mean) <= BAR["rm"] and rel_err(rv, bn.running_var) <= BAR["rv"]
    x = torch.randn(129, C, generator=g).cuda()
    y = ops.bn_apply_fwd(x, rm, ops.rsqrt_eps(rv, EPS), bn.weight.detach().float(), bn.bias.detach().float())
    with torch.no_grad():
        want = bn.eval()(x.double())
    assert max_rel(y, want) <= BAR["y"]
    assert max_rel(y, R.bn_eval_fwd(x.double(), bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), EPS)) <= BAR["y"]


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_rsqrt_eps(n):
    """1 / sqrt(v + eps) with correctly rounded fp32 sqrt and division is ~1e-7 off float64; v = 0 and v << eps included"""
    from tavsr import ops
    v = torch.rand(n, generator=_gen(n)) * 3
    v[0] = 0.0
    if n > 1:
        v[1] = 1e-12
    out = ops.rsqrt_eps(v.cuda(), EPS).cpu().double()
    want = 1.0 / torch.sqrt(v.double() + torch.tensor(EPS, dtype=torch.float32).double())
    assert float(((out - want).abs() / want).max()) <= 1e-6


@pytest.mark.parametrize("N,P,C,offset", [(1, 1, 4, 0), (3, 9, 512, 0), (5, 36, 64, 0), (2, 9, 6, 0), (7, 4, 68, 0), (3, 9, 512, 1)])
def test_avgpool_vector_and_scalar_backward(N, P, C, offset):
    """C = 6 and a gradient that starts 4 bytes into its buffer take the scalar backward kernel, the others the 16-byte one;
    the backward is one fp32 division, so it is exact"""
    from tavsr import ops
    g = _gen(N * P * C + offset)
    x = torch.randn(N, P, C, generator=g)
    y = ops.avgpool_fwd(x.cuda().view(-1, C), N, P, C)
    assert y.shape == (N, C) and max_rel(y.cpu(), R.avgpool_fwd(x.double())) <= 1e-6
    buf = torch.randn(N * C + offset, generator=g).cuda()
    dy = buf[offset:].view(N, C)
    assert dy.is_contiguous() and dy.data_ptr() % 16 == 4 * offset
    dx = ops.avgpool_bwd(dy, N, P, C)
    assert torch.equal(dx.view(N, P, C).cpu(), R.avgpool_bwd(dy.cpu().double(), P).float())


@pytest.mark.parametrize("M,N,lds,ldd", [(64, 245, 245, 256), (64, 245, 256, 245), (1, 1, 1, 1), (3, 257, 300, 259)])
def test_copy2d_leaves_the_padding_columns_alone(M, N, lds, ldd):
    from tavsr import ops
    src = torch.randn(M, lds, generator=_gen(M + N)).cuda()
    dst = torch.full((M, ldd), -7.0, device="cuda")
    ops.copy2d(src[:, :N], dst[:, :N])
    assert torch.equal(dst[:, :N], src[:, :N])
    assert bool((dst[:, N:] == -7.0).all())
