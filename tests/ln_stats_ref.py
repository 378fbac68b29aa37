"""LayerNorm on rows whose mean dwarfs their spread: the input family, the float64 reference, the float32 restatement of the
reference that sets the error bound, and a float32 restatement of how the cgMLP route gets its statistics (per-tile pairs from
the producing GEMM's epilogue, merged in csrc/cgmlp.hip:csgu_fwd_kernel).  Reference of tests/test_ln_stats_host.py (which shows
on the host that the bound can be met, and by which form it cannot) and of tests/test_gpu_ln_conditioning.py.

Input family: row m = (randn(D) + r) * s with (r, s) = CONDS[m % 8], drawn on the host from a seeded generator (the same numbers
wherever the file runs).  r = |mean| / std of the row: at r = 0 every variance formula agrees to rounding, at r = 1000 one that
subtracts raw moments has lost six digits.  (0, 1e-6) has var ~ eps = 1e-12.  There are no exactly constant rows: their float64
answer is 0 and a float32 one rounding noise times 1e6, so they have no usable reference.

Bound: every compared quantity is held to max(floor, 4 * e32) in max |a - b| / max |b| PER CONDITION GROUP of rows - e32 is that
same measure of torch's own float32 LayerNorm (CPU) against float64 on the same inputs, 4 the project's allowance for another
summation order (tests/test_gpu_attn_edges.py, tests/test_gpu_vocab.py).  Nothing in the bound comes from a kernel under test."""
import torch
import torch.nn.functional as F

CONDS = ((0.0, 1.0), (10.0, 1.0), (-10.0, 1.0), (100.0, 1.0), (-100.0, 1e-3), (100.0, 1e3), (1000.0, 1.0), (0.0, 1e-6))
M_ROWS = 19          # odd: the backward kernel's row pairs and 4-row blocks end in a partial pair and a partial block
EPS = 1e-12
TILE = 64            # columns per GEMM tile = per (sum, M2) pair


def cond_of_rows(M):
    return torch.arange(M) % len(CONDS)


def label(c):
    r, s = CONDS[c]
    return f"r={r:g},s={s:g}"


SEED = 4             # see ``family``


def family(D, M=M_ROWS, seed=SEED):
    """[M, D] float32 on the host.  A condition group is two or three rows, so its e32 is itself a small sample: at r = 1000 it
    lies between 4e-6 and 3e-5 from draw to draw (the rounding of a mean of 1000 to float32, up to 3e-5, against a spread of 1).
    SEED is a draw at which it is near the middle of that range, chosen on the host restatement alone, before any kernel ran."""
    g = torch.Generator().manual_seed(1000 * D + M + seed)
    c = cond_of_rows(M)
    r = torch.tensor([CONDS[i][0] for i in c], dtype=torch.float64)[:, None]
    s = torch.tensor([CONDS[i][1] for i in c], dtype=torch.float64)[:, None]
    return ((torch.randn(M, D, generator=g, dtype=torch.float64) + r) * s).float()


def affine(D, seed=1):
    """gamma, beta, float32 on the host"""
    g = torch.Generator().manual_seed(77 * D + seed)
    return 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


# ------------------------------------------------------------------------------------------------ references
def ln_ref64(x, gamma, beta, eps=EPS):
    """-> y, mean, rstd in float64 (two-pass, by the formula)"""
    x = x.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean, rstd


def ln_ref32(x, gamma, beta, eps=EPS):
    """torch's own float32 LayerNorm on the CPU (what F.layer_norm runs) -> y, mean, rstd"""
    x = x.detach().float().cpu().contiguous()
    y, mean, rstd = torch.native_layer_norm(x, (x.shape[1],), gamma.float().cpu(), beta.float().cpu(), eps)
    return y, mean.reshape(-1), rstd.reshape(-1)


def ln_bwd_ref(x, gamma, beta, dy, dtype, eps=EPS):
    """dx, dgamma, dbeta of F.layer_norm under autograd on the CPU in ``dtype``"""
    xr = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    gr, br = gamma.detach().cpu().to(dtype).requires_grad_(True), beta.detach().cpu().to(dtype).requires_grad_(True)
    F.layer_norm(xr, (x.shape[1],), gr, br, eps).backward(dy.detach().cpu().to(dtype))
    return xr.grad, gr.grad, br.grad


# ------------------------------------------------------------------------------------------------ the measure and the bound
def group_errs(a, b, M=None):
    """{condition: max |a - b| / max |b| over that condition's rows}; a, b [M, ...] with rows in family order"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    c = cond_of_rows(a.shape[0] if M is None else M)
    out = {}
    for k in range(len(CONDS)):
        rows = (c == k).nonzero().flatten()
        if len(rows):
            out[k] = float((a[rows] - b[rows]).abs().max() / b[rows].abs().max().clamp_min(1e-300))
    return out


def whole_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def check(op, name, got, ref64, ref32, floor, rows=True, against=None):
    """prints e32, the error and the bound per condition (``rows``: per condition group; else one figure for the tensor: sums
    over all rows, such as parameter gradients) and returns the list of violations (empty: within max(floor, 4 * e32)).
    ``against``: the error is taken against this tensor instead of ``ref64`` (two routes against each other); e32 stays."""
    assert bool(torch.isfinite(got).all()), f"{op} {name}: not finite"
    want = ref64 if against is None else against
    if rows:
        e32, err = group_errs(ref32, ref64), group_errs(got, want)
        items = [(label(k), e32[k], err[k]) for k in err]
    else:
        items = [("all rows", whole_err(ref32, ref64), whole_err(got, want))]
    bad = []
    for lab, e, g in items:
        bound = max(floor, 4 * e)
        line = f"{op:34s} {name:8s} {lab:16s} e32 {e:9.2e}  err {g:9.2e}  bound {bound:9.2e}  {'ok' if g <= bound else 'FAIL'}"
        print(line)
        if not g <= bound:
            bad.append((lab, line))
    return bad


# ------------------------------------------------------------------------------------------------ the cgMLP statistics route
def rowstat_pairs(y, dtype=torch.float32):
    """what tavsr_gemm_desc.rowstat documents, in ``dtype``: [M, ceil(N / 64), 2] = per row and 64-column tile (sum, M2 = sum of
    squared deviations from the tile's own mean over its min(64, N - 64 tile) columns)"""
    y = y.detach().cpu().to(dtype)
    out = []
    for n0 in range(0, y.shape[1], TILE):
        t = y[:, n0:n0 + TILE]
        s = t.sum(-1)
        out.append(torch.stack([s, ((t - (s / t.shape[1])[:, None]) ** 2).sum(-1)], -1))
    return torch.stack(out, 1)


def rowstat_pairs_raw(y):
    """the cancelling format this replaces: (sum, sum of squares) - kept to show that the bound tells the two apart"""
    t = y.detach().float().cpu().reshape(y.shape[0], -1, TILE)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1)


def merge_pairs(pairs, eps=EPS):
    """csgu_fwd_kernel's equal-count Chan merge of a row's C / 64 (sum, M2) pairs, float32 -> mean, rstd:
    mean = avg of the tile means, C var = sum M2_t + 64 sum (mean_t - mean)^2"""
    pairs = pairs.float()
    Cn = pairs.shape[1] * TILE
    mean = pairs[..., 0].sum(-1) / Cn
    dm = pairs[..., 0] * (1.0 / TILE) - mean[:, None]
    var = (pairs[..., 1] + TILE * dm * dm).sum(-1) / Cn
    return mean, 1 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def merge_pairs_raw(pairs, eps=EPS):
    """var = E[x^2] - mean^2 from raw moments, float32"""
    pairs = pairs.float()
    Cn = pairs.shape[1] * TILE
    mean = pairs[..., 0].sum(-1) / Cn
    var = (pairs[..., 1].sum(-1) / Cn - mean * mean).clamp_min(0)
    return mean, 1 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def normalise32(x, mean, rstd, gamma, beta):
    """(x - mean) * rstd * gamma + beta in float32, as the kernel applies given statistics"""
    x = x.detach().float().cpu()
    return (x - mean[:, None]) * rstd[:, None] * gamma.float().cpu() + beta.float().cpu()


# ------------------------------------------------------------------------------------------------ cgMLP inputs with conditioned gate rows
def cgmlp_inputs(M, K, Cn, seed=0):
    """x [M, K], w1 [2 Cn, K], b1 [2 Cn] (float32, host) such that row m of the gate half of x w1^T + b1 is (r + randn) * s' with
    (r, s) = CONDS[m % 8]: r != 0 -> s' = s * sign(r) where |r| s >= 6, else 6 / r, so that r s' >= 6 and gelu is the identity to
    float32 there (gelu lets no negative mean through: the r < 0 groups arrive as |r|); r = 0 -> s' = s.
    A per-column bias cannot give rows different offsets, so the offset r s' rides in the LAST input column against a unit weight
    column of the gate half (a per-row bias; last, so that a GEMM which walks K in order adds it once at the end, as it adds a bias,
    instead of rounding every later partial sum at the offset's magnitude - the test is about the statistics of g, not about how the
    GEMM that forms g rounds); columns 0 .. K/2 - 1 feed the linear half only, at O(1), columns K/2 .. K - 2 the gate half only,
    scaled by s'.  b1's gate half is zero (any spread there would drown the s' = 6e-3 and 1e-6 rows), its linear half 0.1 randn."""
    g = torch.Generator().manual_seed(31 * M + K + Cn + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = cond_of_rows(M)
    h = K // 2
    sp = []
    for i in c:
        r, s = CONDS[i]
        sp.append(s if r == 0 else (s * (1 if r > 0 else -1) if abs(r) * s >= 6 else 6 / r))
    sp = torch.tensor(sp, dtype=torch.float64)[:, None]
    r = torch.tensor([CONDS[i][0] for i in c], dtype=torch.float64)[:, None]
    x = torch.cat([rn(M, h), rn(M, K - h - 1) * sp, r * sp], 1)
    w1 = torch.zeros(2 * Cn, K, dtype=torch.float64)
    w1[:Cn, :h] = rn(Cn, h) / h ** 0.5
    w1[Cn:, h:K - 1] = rn(Cn, K - h - 1) / (K - h - 1) ** 0.5
    w1[Cn:, K - 1] = 1.0
    b1 = torch.cat([0.1 * rn(Cn), torch.zeros(Cn, dtype=torch.float64)])
    return x.float(), w1.float(), b1.float()


def achieved_ratio(gate):
    """|mean| / std per row, float64"""
    gd = gate.detach().double().cpu()
    return gd.mean(1).abs() / gd.std(1, unbiased=False)
