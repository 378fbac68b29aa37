"""The row-reduction and glue kernels of csrc/norm.hip and csrc/attn.hip at their edges: plain torch restatements in a chosen dtype
(float64 = the reference, float32 = the restatement whose own error sets the bound), the dispatch arithmetic of the entry points
restated next to the case tables that are meant to straddle it, and the seeded host inputs.  Reference of
tests/test_rowred_host.py (restatements against autograd; tables against the arithmetic) and tests/test_gpu_rowred_edges.py.

Bound: every comparison against float64 is held to max(floor, 4 * e32); floor is the bar of the op's existing test (FLOOR), e32 the
error of the float32 restatement against float64 on the same inputs in the same measure (max |a - b| / max |b|; per condition group
of rows through ln_stats_ref.check where the rows are ln_stats_ref.family's), 4 the project's allowance for another summation order.
Nothing in a bound comes from a kernel under test."""
import functools

import torch

import ln_stats_ref as R

FLOOR = {"ln_fwd": 2e-5, "ln_bwd": 1e-4, "softmax_bwd": 1e-4, "softmax_fwd": 1e-5, "colsum": 1e-5, "elementwise": 1e-6}
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


def pad4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ dispatch arithmetic (csrc/norm.hip, attn.hip)
LN_MAX_D = 1024          # LN_MAXV * 256
LN_ROWS_PER_BLOCK = 8    # 4 waves x LN_RPW = 2 rows
LN_MAX_BLOCKS = 1024
COLSUM_ROWS = 64         # colsum_chunks(M) = min(cdiv(M, 64), 64)
COLSUM_MAX_CHUNKS = 64
SUM_WAVES = 16           # kSumWaves: partial rows are dealt to 16 waves; the first loop takes 4 deals per trip
SCALE_DEV_MAX_BLOCKS = 2048
SCALE_DEV_THREADS = 256


def ln_nv(D):
    """the backward's instantiation: float4 chunks per lane"""
    assert 0 < D <= LN_MAX_D and D % 4 == 0
    return 1 if D <= 256 else (2 if D <= 512 else 4)


def ln_chunk_lanes(D, nv=None):
    """active lanes (of 64) of each of the ``nv`` chunks (default: the backward's NV; the forward always walks 4)"""
    return [max(0, min(64, (D - 256 * i) // 4)) for i in range(ln_nv(D) if nv is None else nv)]


def ln_chunk_states(D, nv=None):
    return {"full" if n == 64 else ("idle" if n == 0 else "partial") for n in ln_chunk_lanes(D, nv)}


def ln_blocks(M):
    return min(cdiv(M, LN_ROWS_PER_BLOCK), LN_MAX_BLOCKS)


def ln_trips(M):
    """trips of the backward's grid-stride loop taken by block 0"""
    return cdiv(M, ln_blocks(M) * LN_ROWS_PER_BLOCK)


def ln_last_trip_rows(M):
    return M - (ln_trips(M) - 1) * ln_blocks(M) * LN_ROWS_PER_BLOCK


def colsum_chunks(M):
    return min(cdiv(M, COLSUM_ROWS), COLSUM_MAX_CHUNKS)


def colsum_rpc(M):
    """rows per chunk"""
    return cdiv(M, colsum_chunks(M))


def sum_partials_trips(nparts, w):
    """wave ``w`` of sum_partials_kernel: (trips of the 4x unrolled loop, trips of the remainder loop)"""
    q, unrolled, rest = w, 0, 0
    while q + 3 * SUM_WAVES < nparts:
        q += 4 * SUM_WAVES
        unrolled += 1
    while q < nparts:
        q += SUM_WAVES
        rest += 1
    return unrolled, rest


def scale_dev_blocks(n):
    return min(cdiv(n, SCALE_DEV_THREADS), SCALE_DEV_MAX_BLOCKS)


def scale_dev_trips(n):
    """trips of thread 0's stride loop"""
    return cdiv(n, scale_dev_blocks(n) * SCALE_DEV_THREADS)


# ------------------------------------------------------------------------------------------------ case tables
LN_WIDTHS = (4, 60, 64, 68, 252, 256, 260, 320, 508, 512, 516, 768, 1020, 1024)      # at M = ln_stats_ref.M_ROWS
LN_FAMILY_WIDTHS = (320, 512, 768)                                                    # also on the ill-conditioned rows
LN_SHORT = tuple((M, D) for M in (1, 2, 3, 8, 9) for D in (64, 512))
LN_TALL_M = 8203                                                                      # a second trip of 11 rows
LN_TALL = tuple((LN_TALL_M, D) for D in (64, 512, 1024))
LN_DROP = ((9, 512), (LN_TALL_M, 256), (LN_TALL_M, 512))
LN_REFUSED_D = (0, 6, 1028)
# each M with two N, each N with (at least) two M
COLSUM_CASES = ((1, 1), (1, 64), (3, 41), (3, 65), (63, 63), (63, 256), (64, 64), (64, 1), (65, 65), (65, 41), (130, 63), (130, 256),
                (4032, 1), (4032, 64), (4033, 41), (4033, 65), (4097, 63), (4097, 256), (20000, 41), (20000, 64))
COLSUM_M = (1, 3, 63, 64, 65, 130, 4032, 4033, 4097, 20000)
COLSUM_N = (1, 41, 63, 64, 65, 256)
SUM_NPARTS = (1, 15, 16, 17, 63, 64, 65, 1024)
SUM_N = (1, 64, 65, 200)
SUM_SPLITS = ((41, 23), (64, 64), (0, 5), (5, 0))
SUM_PAD = 12             # stride = n and n + SUM_PAD
AXPBY_N = (1, 3, 4, 5, 1023, 1024, 1025, 1027)
SCALE_DEV_N = (1, 524288, 524289, 600001)
ROWS2D_M = (1, 65)
ROWS2D_N = (4, 252, 256)


def _sm(H, B, T1, T2, rel, causal, klens):
    return dict(H=H, B=B, T1=T1, T2=T2, rel=rel, causal=causal, klens=tuple(klens))


# klens from {0, 1, T - 1, T, T + 5}.  A length above T2 never sits on the LAST utterance: a kernel that forgot min(T2, klens) then
# reads the next utterance's scores (wrong values, which the test sees) and nothing outside the buffer.
SOFTMAX_CASES = (
    _sm(1, 1, 1, 1, True, False, [1]),               # one row: a block with three idle waves
    _sm(2, 3, 2, 2, True, False, [7, 0, 2]),
    _sm(1, 1, 63, 63, True, False, [62]),            # 63 rows: the last block part-filled
    _sm(2, 2, 64, 64, True, False, [69, 63]),
    _sm(3, 1, 65, 65, True, False, [65]),            # 195 rows
    _sm(1, 3, 127, 127, True, False, [132, 0, 126]),
    _sm(2, 2, 128, 128, True, False, [1, 128]),
    _sm(1, 2, 129, 129, True, False, [134, 128]),
    _sm(1, 2, 257, 257, True, False, [0, 257]),
    _sm(2, 3, 1, 300, False, False, [305, 0, 299]),
    _sm(1, 3, 65, 1, False, False, [6, 0, 1]),       # 195 rows of one key
    _sm(2, 2, 13, 129, False, False, [134, 128]),
    _sm(1, 2, 64, 64, False, False, [63, 64]),
    _sm(1, 2, 1, 1, False, True, [0, 1]),
    _sm(2, 2, 65, 65, False, True, [65, 1]),         # utterance 1: rows 1.. see fewer keys than their diagonal allows
)
SOFTMAX_DROP_SHAPES = ((1, 1, 4), (5, 5, 8), (65, 65, 68), (64, 64, 72))      # (T1, T2, ld_s)
SOFTMAX_SCALE = 0.125


def softmax_id(c):
    return f"{'rel' if c['rel'] else ('causal' if c['causal'] else 'plain')}-H{c['H']}B{c['B']}-{c['T1']}x{c['T2']}"


# ------------------------------------------------------------------------------------------------ restatements
def dact(z, act, dtype):
    """act'(z) of the activations tavsr_act_bwd takes (None / 'none', relu, swish, gelu), closed forms"""
    z = z.detach().cpu().to(dtype)
    if act in (None, "none"):
        return torch.ones_like(z)
    if act == "relu":
        return (z > 0).to(dtype)
    if act == "swish":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == "gelu":
        return 0.5 * (1 + torch.erf(z * 0.5 ** 0.5)) + z * torch.exp(-0.5 * z * z) * (1 / (2 * torch.pi) ** 0.5)
    raise KeyError(act)


def ln_fwd(x, gamma, beta, dtype, eps=R.EPS):
    """-> y, mean, rstd (ln_stats_ref's two references)"""
    return R.ln_ref64(x, gamma, beta, eps) if dtype == torch.float64 else R.ln_ref32(x, gamma, beta, eps)


def ln_bwd(x, gamma, beta, dy, dtype, dx_add=None, z=None, act=None, eps=R.EPS):
    """dx (+ dx_add, or * act'(z) for the ``act`` variant: the gradient w.r.t. z of LayerNorm(act(z))), dgamma, dbeta"""
    dx, dg, db = R.ln_bwd_ref(x, gamma, beta, dy, dtype, eps)
    if dx_add is not None:
        dx = dx + dx_add.detach().cpu().to(dtype)
    if z is not None:
        dx = dx * dact(z, act, dtype)
    return dx, dg, db


def colsum(x, dtype, scale=1.0, out0=None):
    """scale * column sums (+ out0 under ``accumulate``)"""
    s = x.detach().cpu().to(dtype).sum(0) * scale
    return s if out0 is None else out0.detach().cpu().to(dtype) + s


def add2_colsum(x, y, dtype):
    """x + y and the column sums of each"""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    return x + y, x.sum(0), y.sum(0)


def sum_partials(part, n1, n2, dtype, out0=None):
    """part [nparts, stride >= n1 + n2] -> (sum over the rows of columns [0, n1), of columns [n1, n1 + n2)); out0 = (o1, o2) to
    accumulate into"""
    s = part.detach().cpu().to(dtype)[:, :n1 + n2].sum(0)
    o1, o2 = s[:n1], s[n1:]
    if out0 is not None:
        o1, o2 = out0[0].detach().cpu().to(dtype) + o1, out0[1].detach().cpu().to(dtype) + o2
    return o1, o2


def _skew_index(T):
    return T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]


def softmax_valid(klens, T1, T2, causal):
    """[B, T1, T2] bool: key j of row i is live"""
    kl = torch.as_tensor(klens)
    v = (torch.arange(T2)[None, None, :] < kl[:, None, None]).expand(len(kl), T1, T2)
    if causal:
        v = v & (torch.arange(T2)[None, :] <= torch.arange(T1)[:, None])[None]
    return v


def softmax_fwd(ac, bd, klens, scale, causal, dtype):
    """ac [H, B, T1, T2], bd [H, B, T, 2T - 1] or None (live columns only) -> attn: the reference's
    masked_fill(min) -> softmax -> masked_fill(0) on (ac + rel_shift(bd)) * scale, the shift as a gather; a row without a live key
    (klens = 0) comes out as zeros"""
    H, B, T1, T2 = ac.shape
    sc = ac.detach().cpu().to(dtype)
    if bd is not None:
        sc = sc + torch.gather(bd.detach().cpu().to(dtype), 3, _skew_index(T1).expand(H, B, T1, T2))
    dead = ~softmax_valid(klens, T1, T2, causal)[None]
    return torch.softmax((sc * scale).masked_fill(dead, torch.finfo(dtype).min), -1).masked_fill(dead, 0.0)


def softmax_bwd(attn, dattn, scale, skew, dtype):
    """ds = attn * (dattn - <attn, dattn>) * scale and, with ``skew``, ds_skew[i, T - 1 - i + j] = ds[i, j], 0 elsewhere"""
    a, g = attn.detach().cpu().to(dtype), dattn.detach().cpu().to(dtype)
    ds = a * (g - (a * g).sum(-1, keepdim=True)) * scale
    if not skew:
        return ds, None
    H, B, T, _ = ds.shape
    sk = torch.zeros(H, B, T, 2 * T - 1, dtype=dtype)
    sk.scatter_(3, _skew_index(T).expand(H, B, T, T), ds)
    return ds, sk


def axpby(x, y, a, b, dtype):
    """a x + b y (y may be None); the strided 2-D form is the same formula on the live columns"""
    r = a * x.detach().cpu().to(dtype)
    return r if y is None else r + b * y.detach().cpu().to(dtype)


def act_bwd(dh, z, act, dtype):
    return dh.detach().cpu().to(dtype) * dact(z, act, dtype)


def scale_dev(x, s, c, dtype):
    """x * (c * s), s a one-element tensor"""
    return x.detach().cpu().to(dtype) * (torch.as_tensor(c, dtype=dtype) * s.detach().cpu().to(dtype).reshape(()))


def add_head_bias(q, u, v, dtype):
    q = q.detach().cpu().to(dtype)
    return q + u.detach().cpu().to(dtype), q + v.detach().cpu().to(dtype)


# ------------------------------------------------------------------------------------------------ the measure and the bound
def err(a, b):
    """max |a - b| / max |b| (0 where both are all zero)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    d, m = float((a - b).abs().max()), float(b.abs().max())
    return 0.0 if d == 0.0 else d / max(m, 1e-300)


def check(op, shape, name, got, ref64, ref32, floor):
    """prints one line (op, shape, e32, error, bound); returns the violations as ln_stats_ref.check does"""
    assert bool(torch.isfinite(got).all()), f"{op} {shape} {name}: not finite"
    e32, e = err(ref32, ref64), err(got, ref64)
    bound = max(floor, 4 * e32)
    line = f"{op:22s} {shape:22s} {name:8s} e32 {e32:9.2e}  err {e:9.2e}  bound {bound:9.2e}  {'ok' if e <= bound else 'FAIL'}"
    print(line)
    return [] if e <= bound else [(name, line)]


# ------------------------------------------------------------------------------------------------ host inputs (seeded; cached: shared, never modified)
def host_randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def row_tags(M):
    """(offset, scale) [M, 1] that identify row m (periods 13 and 5 rows: a row read twice, or another row in its place, or none,
    changes every column sum by O(1) of a term - nothing cancels)"""
    m = torch.arange(M, dtype=torch.float32)[:, None]
    return (m % 13 - 6) * 0.25, 1 + (m % 5) * 0.5


@functools.lru_cache(maxsize=None)
def ln_inputs(M, D, family=False):
    """x [M, D] (randn rows tagged by ``row_tags``, or ln_stats_ref.family), gamma, beta, dy (tagged too), dx_add, z: float32, host"""
    off, sc = row_tags(M)
    x = R.family(D, M=M) if family else (host_randn(11 * M + D, M, D) + off) * sc
    gamma, beta = R.affine(D)
    dy = host_randn(11 * M + D + 1, M, D) * sc.flip(0) + 0.1 * off
    return x, gamma, beta, dy, host_randn(11 * M + D + 2, M, D), host_randn(11 * M + D + 3, M, D)


@functools.lru_cache(maxsize=None)
def ln_refs(M, D, family=False):
    """{dtype: dict of every reference quantity} for ``ln_inputs(M, D, family)``"""
    x, gamma, beta, dy, add, z = ln_inputs(M, D, family)
    out = {}
    for dt in (torch.float64, torch.float32):
        y, mean, rstd = ln_fwd(x, gamma, beta, dt)
        dx, dg, db = ln_bwd(x, gamma, beta, dy, dt)
        out[dt] = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db, dx_add=dx + add.to(dt), dz=dx * dact(z, "gelu", dt))
    return out


ACT_Z_LADDER = (1.0, -0.3, 2.0, -2.5, 0.6)


@functools.lru_cache(maxsize=None)
def act_inputs(n):
    """dh, z [n].  The measure max |a - b| / max |b| over a handful of elements is a pointwise relative error, and at a z where act'
    is nearly 0 (gelu' crosses 0 at z = -0.7518) no float32 formula has one - the restatement's own e32 is above the floor there.
    So below 8 elements z walks a fixed ladder away from that point instead of a draw that may land on it; from 8 on, randn * 2."""
    z = host_randn(n + 3, n) * 2
    if n < 8:
        z = torch.tensor(ACT_Z_LADDER[:n])
    return host_randn(n + 2, n), z


@functools.lru_cache(maxsize=None)
def colsum_inputs(M, N):
    """x, y [M, N]: randn + 0.5 and randn - 0.25 scaled by the row's tag - column sums of O(M), far from cancelling"""
    _, sc = row_tags(M)
    return (host_randn(3 * M + N, M, N) + 0.5) * sc, (host_randn(3 * M + N + 1, M, N) - 0.25) * sc


@functools.lru_cache(maxsize=None)
def softmax_inputs(key):
    """(ac [H,B,T1,T2], bd [H,B,T,2T-1] or None, dattn like ac) of SOFTMAX_CASES[key], live columns only"""
    c = SOFTMAX_CASES[key]
    H, B, T1, T2 = c["H"], c["B"], c["T1"], c["T2"]
    ac = host_randn(100 + key, H, B, T1, T2) * 4
    bd = host_randn(200 + key, H, B, T1, 2 * T1 - 1) * 4 if c["rel"] else None
    return ac, bd, host_randn(300 + key, H, B, T1, T2)


@functools.lru_cache(maxsize=None)
def softmax_refs(key):
    """{dtype: (attn, ds, ds_skew or None)}: the backward of each dtype runs on that dtype's own attn (the whole chain restated)"""
    c = SOFTMAX_CASES[key]
    ac, bd, da = softmax_inputs(key)
    out = {}
    for dt in (torch.float64, torch.float32):
        attn = softmax_fwd(ac, bd, c["klens"], SOFTMAX_SCALE, c["causal"], dt)
        out[dt] = (attn,) + softmax_bwd(attn, da, SOFTMAX_SCALE, c["rel"], dt)
    return out
