"""Host (no GPU): tests/rowred_ref.py - each restatement against torch autograd in float64 on small inputs, and each case table of
tests/test_gpu_rowred_edges.py against the restated dispatch arithmetic of csrc/norm.hip / attn.hip: a table that stopped covering a
branch fails here.  Also that no case's own float32 error (e32) is more than 10x its floor: the bound stays the floor's size."""
import pytest
import torch
import torch.nn.functional as F

import ln_stats_ref as R
import rowred_ref as RR

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert RR.err(a, b) <= tol, RR.err(a, b)


# ------------------------------------------------------------------------------------------------ restatements against autograd
@pytest.mark.parametrize("act", ["none", "relu", "swish", "gelu"])
def test_dact_is_autograds_derivative(act):
    z = RR.host_randn(1, 300).double() * 3
    zz = z.clone().requires_grad_(True)
    {"none": lambda t: t, "relu": F.relu, "swish": F.silu, "gelu": F.gelu}[act](zz).sum().backward()
    _close(RR.dact(z, act, F64), zz.grad)
    dh = RR.host_randn(2, 300)
    _close(RR.act_bwd(dh, z, act, F64), dh.double() * zz.grad)


def test_layernorm_backward_with_residual_and_with_activation():
    M, D = 5, 12
    z, gamma, beta, dy, add = (RR.host_randn(s, *sh).double() for s, sh in ((1, (M, D)), (2, (D,)), (3, (D,)), (4, (M, D)), (5, (M, D))))
    zz, g, b = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    x = F.gelu(zz)
    y = F.layer_norm(x, (D,), g, b, R.EPS)
    _close(RR.ln_fwd(x, gamma, beta, F64)[0], y)
    (y * dy).sum().backward()                                  # gradient w.r.t. z of LayerNorm(gelu(z))
    dz, dg, db = RR.ln_bwd(x, gamma, beta, dy, F64, z=z, act="gelu")
    _close(dz, zz.grad, 1e-10), _close(dg, g.grad, 1e-10), _close(db, b.grad, 1e-10)
    xx = x.detach().clone().requires_grad_(True)                # dx_add: a second path from x to the loss
    (F.layer_norm(xx, (D,), gamma, beta, R.EPS) * dy + xx * add).sum().backward()
    _close(RR.ln_bwd(x, gamma, beta, dy, F64, dx_add=add)[0], xx.grad, 1e-10)


def test_column_sums_and_partial_slab_sums():
    x, y = RR.host_randn(1, 7, 5).double(), RR.host_randn(2, 7, 5).double()
    out0 = RR.host_randn(3, 5).double()
    xx = x.clone().requires_grad_(True)
    (xx * 0.5).sum(0).backward(torch.ones(5, dtype=F64))       # d/dx of the scaled column sums is the scale: the sum is linear
    assert bool((xx.grad == 0.5).all())
    _close(RR.colsum(x, F64, 0.5), torch.stack([0.5 * sum(x[m, n] for m in range(7)) for n in range(5)]))
    _close(RR.colsum(x, F64, 0.5, out0), out0 + 0.5 * x.sum(0))
    assert bool((RR.colsum(x[:0], F64, 0.5) == 0).all())        # the empty sum
    o, sx, sy = RR.add2_colsum(x, y, F64)
    _close(o, x + y), _close(sx, x.sum(0)), _close(sy, y.sum(0))
    part = RR.host_randn(4, 9, 11).double()                     # stride 11 > n1 + n2 = 8
    o1, o2 = RR.sum_partials(part, 5, 3, F64)
    _close(o1, part[:, :5].sum(0)), _close(o2, part[:, 5:8].sum(0))
    a1, a2 = RR.sum_partials(part, 5, 3, F64, out0=(out0[:5], out0[:3]))
    _close(a1, out0[:5] + o1), _close(a2, out0[:3] + o2)
    assert RR.sum_partials(part, 0, 5, F64)[0].numel() == 0 and RR.sum_partials(part, 5, 0, F64)[1].numel() == 0


@pytest.mark.parametrize("key", [1, 3, 9, 14])                # rel with klens 0 and > T; rel at 64; plain 1 x 300; causal 65
def test_softmax_restatement_against_autograd(key):
    c = RR.SOFTMAX_CASES[key]
    ac, bd, da = RR.softmax_inputs(key)
    H, B, T1, T2 = ac.shape
    acr = ac.double().requires_grad_(True)
    bdr = bd.double().requires_grad_(True) if bd is not None else None
    sc = acr
    if bd is not None:                                         # espnet's rel_shift by pad-and-view instead of the gather
        zero = torch.zeros(H, B, T1, 1, dtype=F64)
        full = torch.cat([zero, bdr], -1).view(H, B, 2 * T1, T1)[:, :, 1:].reshape(H, B, T1, 2 * T1 - 1)[..., :T1]
        sc = acr + full
    dead = ~RR.softmax_valid(c["klens"], T1, T2, c["causal"])[None]
    ref = torch.softmax((sc * RR.SOFTMAX_SCALE).masked_fill(dead, torch.finfo(F64).min), -1).masked_fill(dead, 0.0)
    attn = RR.softmax_fwd(ac, bd, c["klens"], RR.SOFTMAX_SCALE, c["causal"], F64)
    _close(attn, ref)
    for b, k in enumerate(c["klens"]):
        if k == 0:
            assert bool((attn[:, b] == 0).all())                # no live key: a row of zeros
        else:
            _close(attn[:, b].sum(-1), torch.ones(H, T1, dtype=F64))
    ref.backward(da.double())
    ds, sk = RR.softmax_bwd(attn, da, RR.SOFTMAX_SCALE, c["rel"], F64)
    _close(ds, acr.grad, 1e-10)
    if c["rel"]:
        _close(sk, bdr.grad, 1e-10)


def test_elementwise_restatements():
    x, y = RR.host_randn(1, 6, 8).double(), RR.host_randn(2, 6, 8).double()
    _close(RR.axpby(x, y, 0.5, -2.0, F64), 0.5 * x - 2.0 * y), _close(RR.axpby(x, None, 3.0, 7.0, F64), 3.0 * x)
    s = torch.tensor([0.37])
    _close(RR.scale_dev(x, s, 2.0, F64), x * (2.0 * float(s.double())))
    u, v = RR.host_randn(3, 8).double(), RR.host_randn(4, 8).double()
    qu, qv = RR.add_head_bias(x, u, v, F64)
    _close(qu, x + u[None]), _close(qv, x + v[None])


# ------------------------------------------------------------------------------------------------ case tables against the dispatch arithmetic
def test_layernorm_widths_reach_every_instantiation_and_every_chunk_state():
    assert {RR.ln_nv(D) for D in RR.LN_WIDTHS} == {1, 2, 4}
    # NV = 1 and 2 cannot leave a chunk of the backward idle (D > 256 (NV - 1)); NV = 4 can (512 < D <= 768)
    want = {1: {"full", "partial"}, 2: {"full", "partial"}, 4: {"full", "partial", "idle"}}
    for nv in (1, 2, 4):
        seen = set().union(*(RR.ln_chunk_states(D) for D in RR.LN_WIDTHS if RR.ln_nv(D) == nv))
        assert seen == want[nv], (nv, seen)
        # ... and one width of that NV fills every chunk, one leaves its LAST chunk part-filled
        assert any(RR.ln_chunk_states(D) == {"full"} for D in RR.LN_WIDTHS if RR.ln_nv(D) == nv)
        assert any(0 < RR.ln_chunk_lanes(D)[-1] < 64 for D in RR.LN_WIDTHS if RR.ln_nv(D) == nv)
    assert RR.ln_chunk_lanes(320) == [64, 16] and RR.ln_chunk_lanes(768) == [64, 64, 64, 0] and RR.ln_chunk_lanes(4) == [1]
    assert RR.ln_chunk_lanes(1020) == [64, 64, 64, 63] and RR.ln_chunk_lanes(516) == [64, 64, 1, 0]
    assert "idle" in RR.ln_chunk_states(4, nv=4)                # the forward walks four chunks at every width
    assert {RR.ln_nv(D) for D in RR.LN_FAMILY_WIDTHS} == {2, 4}
    assert set(RR.LN_FAMILY_WIDTHS) <= set(RR.LN_WIDTHS)
    assert R.M_ROWS % 2 == 1 and R.M_ROWS % 4 != 0 and RR.ln_trips(R.M_ROWS) == 1
    for D in RR.LN_REFUSED_D:
        assert D <= 0 or D % 4 or D > RR.LN_MAX_D


def test_layernorm_heights_take_one_trip_or_two_and_end_in_a_partial_pair():
    for M, D in RR.LN_SHORT:
        assert RR.ln_trips(M) == 1
    assert {RR.ln_blocks(M) for M, _ in RR.LN_SHORT} == {1, 2}
    assert {M % 2 for M, _ in RR.LN_SHORT} == {0, 1}
    for M, D in RR.LN_TALL + tuple(c for c in RR.LN_DROP if c[0] > 8192):
        assert RR.ln_blocks(M) == RR.LN_MAX_BLOCKS and RR.ln_trips(M) == 2
        last = RR.ln_last_trip_rows(M)
        assert last == 11 and last % 2 == 1 and last % RR.LN_ROWS_PER_BLOCK != 0 and last < RR.LN_MAX_BLOCKS * RR.LN_ROWS_PER_BLOCK
        assert RR.sum_partials_trips(RR.ln_blocks(M), 0)[0] > 0                    # the 1024 partial rows take the unrolled loop
    assert {RR.ln_nv(D) for _, D in RR.LN_TALL} == {1, 2, 4}
    assert {RR.ln_nv(D) for M, D in RR.LN_DROP if M > 8192} == {1, 2} and any(M <= 8192 and D not in (256, 1024) for M, D in RR.LN_DROP)


def test_colsum_cases_fall_on_both_sides_of_the_chunk_cap():
    assert {M for M, _ in RR.COLSUM_CASES} == set(RR.COLSUM_M) and {N for _, N in RR.COLSUM_CASES} == set(RR.COLSUM_N)
    for M in RR.COLSUM_M:
        assert sum(m == M for m, _ in RR.COLSUM_CASES) >= 2
    for N in RR.COLSUM_N:
        assert sum(n == N for _, n in RR.COLSUM_CASES) >= 2
    uncapped = {M: RR.cdiv(M, RR.COLSUM_ROWS) for M in RR.COLSUM_M}
    assert any(v < RR.COLSUM_MAX_CHUNKS for v in uncapped.values())
    assert RR.COLSUM_MAX_CHUNKS - 1 in uncapped.values() and RR.COLSUM_MAX_CHUNKS in uncapped.values()
    assert RR.COLSUM_MAX_CHUNKS + 1 in uncapped.values() and max(uncapped.values()) > 4 * RR.COLSUM_MAX_CHUNKS
    assert {RR.colsum_rpc(M) for M in RR.COLSUM_M} >= {1, 3, 63, 64, 65}            # below one chunk, the cap's 64, one past it
    assert RR.colsum_rpc(4097) == 65 and RR.colsum_chunks(4097) * 65 > 4097        # the last chunk of a capped grid is partial
    assert RR.colsum_rpc(20000) % 4 != 0 or RR.colsum_rpc(4097) % 4 != 0           # rows per chunk not a multiple of the 4 row lanes
    assert any(RR.colsum_chunks(M) == 1 and M < 4 for M in RR.COLSUM_M)             # fewer rows than row lanes
    assert {n % 64 for n in RR.COLSUM_N} >= {0, 1, 63} and any(n > 64 for n in RR.COLSUM_N)


def test_sum_partials_cases_fall_on_both_sides_of_the_deal_and_the_unroll():
    W = RR.SUM_WAVES
    assert {W - 1, W, W + 1, 4 * W - 1, 4 * W, 4 * W + 1} <= set(RR.SUM_NPARTS)
    trips = {p: [RR.sum_partials_trips(p, w) for w in range(W)] for p in RR.SUM_NPARTS}
    assert all(t == (0, 0) for t in trips[1][1:]) and trips[1][0] == (0, 1)         # fewer partials than waves: idle waves
    assert trips[W - 1][W - 1] == (0, 0) and trips[W][W - 1] == (0, 1) and trips[W + 1][0] == (0, 2)
    assert all(u == 0 for p in (1, W - 1, W, W + 1) for u, _ in trips[p])          # the remainder loop alone
    # wave w takes the unrolled trip from 3 W + w + 1 partials on: at 4 W - 1 the last wave still walks its three by the remainder loop
    assert all(t == (1, 0) for t in trips[4 * W - 1][:W - 1]) and trips[4 * W - 1][W - 1] == (0, 3)
    assert all(t == (1, 0) for t in trips[4 * W])                                   # exactly one unrolled trip, no remainder
    assert trips[4 * W + 1][0] == (1, 1) and trips[4 * W + 1][1] == (1, 0)
    assert all(t == (16, 0) for t in trips[1024])
    for p in RR.SUM_NPARTS:                                                         # the restated loops visit every partial once
        assert sum(4 * u + r for u, r in trips[p]) == p
    assert {n % 64 for n in RR.SUM_N} >= {0, 1} and any(n < 64 for n in RR.SUM_N) and any(n > 128 for n in RR.SUM_N)
    assert any(0 < n1 % 64 and n2 for n1, n2 in RR.SUM_SPLITS)                      # one 64-column block writes both outputs
    assert any(n1 % 64 == 0 and n1 and n2 for n1, n2 in RR.SUM_SPLITS) and (0, 5) in RR.SUM_SPLITS and (5, 0) in RR.SUM_SPLITS


def test_elementwise_cases_straddle_the_vector_tail_and_the_grid_cap():
    assert {n % 4 for n in RR.AXPBY_N} == {0, 1, 3} and any(n < 4 for n in RR.AXPBY_N)
    assert any(n > 1024 and n % 4 for n in RR.AXPBY_N)          # a second block whose last thread takes the scalar tail
    cap = RR.SCALE_DEV_MAX_BLOCKS * RR.SCALE_DEV_THREADS
    assert cap in RR.SCALE_DEV_N and cap + 1 in RR.SCALE_DEV_N
    assert [RR.scale_dev_trips(n) for n in RR.SCALE_DEV_N] == [1, 1, 2, 2]
    assert 600001 - cap < cap                                   # a part-filled second trip
    assert any(n % 256 == 0 for n in RR.ROWS2D_N) and any(n // 4 % 64 for n in RR.ROWS2D_N)


def test_softmax_cases_cover_the_row_tail_the_wave_steps_and_the_key_lengths():
    rel = [c for c in RR.SOFTMAX_CASES if c["rel"]]
    assert {c["T1"] for c in rel} == {1, 2, 63, 64, 65, 127, 128, 129, 257} and all(c["T1"] == c["T2"] for c in rel)
    for T, hb in ((1, (1, 1)), (63, (1, 1)), (65, (3, 1))):
        c = next(c for c in rel if c["T1"] == T)
        assert (c["H"], c["B"]) == hb
    assert sum((c["H"] * c["B"] * c["T1"]) % 4 != 0 for c in RR.SOFTMAX_CASES) >= 3
    plain = {(c["T1"], c["T2"]) for c in RR.SOFTMAX_CASES if not c["rel"] and not c["causal"]}
    assert plain == {(1, 300), (65, 1), (13, 129), (64, 64)}
    causal = [c for c in RR.SOFTMAX_CASES if c["causal"]]
    assert {c["T1"] for c in causal} == {1, 65} and all(c["T1"] == c["T2"] for c in causal)
    assert all(any(k < c["T1"] for k in c["klens"]) for c in causal)
    for c in RR.SOFTMAX_CASES:
        T = c["T2"]
        assert len(c["klens"]) == c["B"] and set(c["klens"]) <= {0, 1, T - 1, T, T + 5}
        assert c["klens"][-1] <= T                              # (see the table's comment)
    ks = [(k, c["T2"]) for c in RR.SOFTMAX_CASES for k in c["klens"]]
    assert any(k == 0 for k, _ in ks) and any(k > T for k, T in ks) and any(k == T for k, T in ks) and any(0 < k < T for k, T in ks)
    # padded rows of the fused-dropout forms: padding inside the row's last float4 of keys, and whole float4s of padding
    assert any(0 < ld - T2 < 4 for _, T2, ld in RR.SOFTMAX_DROP_SHAPES) and any(ld - T2 >= 8 for _, T2, ld in RR.SOFTMAX_DROP_SHAPES)
    assert all(ld % 4 == 0 and ld >= T2 for _, T2, ld in RR.SOFTMAX_DROP_SHAPES)


# ------------------------------------------------------------------------------------------------ e32 of the chosen inputs
def test_no_case_owes_its_bound_to_badly_chosen_inputs():
    """e32 <= 10 floor everywhere; the long sums (20000 rows, 8203 rows) are the candidates"""
    for M, N in RR.COLSUM_CASES:
        x, y = RR.colsum_inputs(M, N)
        for t in (x, y):
            assert RR.err(RR.colsum(t, torch.float32, 0.5), RR.colsum(t, F64, 0.5)) <= 10 * RR.FLOOR["colsum"], (M, N)
    for M, D in ((RR.LN_TALL_M, 64), (R.M_ROWS, 320), (9, 512)):
        r = RR.ln_refs(M, D)
        for k, floor in (("y", "ln_fwd"), ("dx", "ln_bwd"), ("dgamma", "ln_bwd"), ("dbeta", "ln_bwd"), ("dz", "ln_bwd")):
            assert RR.err(r[torch.float32][k], r[F64][k]) <= 10 * RR.FLOOR[floor], (M, D, k)
    for key in range(len(RR.SOFTMAX_CASES)):
        r = RR.softmax_refs(key)
        assert RR.err(r[torch.float32][0], r[F64][0]) <= 10 * RR.FLOOR["softmax_fwd"], key
        assert RR.err(r[torch.float32][1], r[F64][1]) <= 10 * RR.FLOOR["softmax_bwd"], key
    for n in RR.AXPBY_N:
        dh, z = RR.act_inputs(n)
        for act in ("none", "relu", "swish", "gelu"):
            assert RR.err(RR.act_bwd(dh, z, act, torch.float32), RR.act_bwd(dh, z, act, F64)) <= RR.FLOOR["elementwise"], (n, act)
    for D in RR.LN_FAMILY_WIDTHS:                               # per condition group, as the GPU test measures them
        r = RR.ln_refs(R.M_ROWS, D, True)
        for k, floor in (("y", 2e-5), ("dx", 1e-4)):
            assert max(R.group_errs(r[torch.float32][k], r[F64][k]).values()) <= 10 * floor, (D, k)
