"""Host (no GPU): the float32 restatement of the cgMLP statistics route (tests/ln_stats_ref.py: per-tile (sum, M2) pairs as
tavsr_gemm_desc.rowstat documents them, merged as csgu_fwd_kernel merges them) meets the bound of
tests/test_gpu_ln_conditioning.py - max(floor, 4 * e32) per condition group - on the whole input family, so the bound is known to
be satisfiable before a kernel is measured against it; the raw (sum, sum of squares) format it replaces does not, so the bound is
known to tell the two apart; and the float64 reference agrees with torch's own."""
import pytest
import torch
import torch.nn.functional as F

import ln_stats_ref as R

FLOOR = 2e-5        # the csgu_fwd floor of tests/test_gpu_ops.py:test_csgu_fused_forward_edge_shapes


def test_family_is_reproducible_and_has_every_condition():
    x = R.family(256)
    assert x.shape == (R.M_ROWS, 256) and x.dtype == torch.float32 and torch.equal(x, R.family(256))
    ratio = R.achieved_ratio(x)
    for m in range(R.M_ROWS):
        r, s = R.CONDS[m % 8]
        assert abs(float(ratio[m]) - abs(r)) <= 0.2 * max(abs(r), 1.0), (m, float(ratio[m]))
        assert float(x[m].double().std()) == pytest.approx(s, rel=0.2)
    assert not bool((x.max(1).values == x.min(1).values).any())        # no constant row


@pytest.mark.parametrize("D", [64, 256, 1024])
def test_reference_is_torchs_layer_norm_in_float64(D):
    x = R.family(D)
    gam, bet = R.affine(D)
    y, mean, rstd = R.ln_ref64(x, gam, bet)
    want = F.layer_norm(x.double(), (D,), gam.double(), bet.double(), R.EPS)
    assert float((y - want).abs().max()) <= 1e-9 * float(want.abs().max())
    _, m2, r2 = torch.native_layer_norm(x.double(), (D,), gam.double(), bet.double(), R.EPS)
    assert float((mean - m2.reshape(-1)).abs().max() / mean.abs().max()) < 1e-12
    assert float((rstd / r2.reshape(-1) - 1).abs().max()) < 1e-9


@pytest.mark.parametrize("Cn", [256, 1024])
def test_tile_pairs_merged_by_chan_meet_the_bound_on_the_whole_family(Cn):
    x = R.family(Cn)
    gam, bet = R.affine(Cn)
    y64, m64, r64 = R.ln_ref64(x, gam, bet)
    y32, m32, r32 = R.ln_ref32(x, gam, bet)
    mean, rstd = R.merge_pairs(R.rowstat_pairs(x))
    bad = []
    for name, got, a, b in (("mean", mean, m64, m32), ("rstd", rstd, r64, r32),
                            ("y", R.normalise32(x, mean, rstd, gam, bet), y64, y32)):
        bad += R.check(f"restated csgu rowstat Cn={Cn}", name, got, a, b, FLOOR)
    assert not bad, "\n".join(line for _, line in bad)


@pytest.mark.parametrize("Cn", [256, 1024])
def test_raw_second_moments_miss_the_bound_from_r_100_on(Cn):
    """(sum, sum of squares) pairs and var = E[x^2] - mean^2 in float32: rstd off by r^2 * 2^-24 and more"""
    x = R.family(Cn)
    gam, bet = R.affine(Cn)
    _, _, r64 = R.ln_ref64(x, gam, bet)
    _, _, r32 = R.ln_ref32(x, gam, bet)
    _, rstd = R.merge_pairs_raw(R.rowstat_pairs_raw(x))
    bad = R.check(f"raw moments Cn={Cn}", "rstd", rstd, r64, r32, FLOOR)
    failed = {lab for lab, _ in bad}
    for k, (r, s) in enumerate(R.CONDS):
        if abs(r) >= 100:
            assert R.label(k) in failed, (R.label(k), bad)


@pytest.mark.parametrize("Cn", [256, 1024])
def test_cgmlp_inputs_reach_their_ratios(Cn):
    M, K = 19, 256
    x, w1, b1 = R.cgmlp_inputs(M, K, Cn)
    gate = F.gelu(x.double() @ w1.double().t() + b1.double())[:, Cn:]
    ratio = R.achieved_ratio(gate)
    for m in range(M):
        r = abs(R.CONDS[m % 8][0])
        if r:
            assert float(ratio[m]) >= 0.5 * r, (m, float(ratio[m]))
    assert bool(torch.isfinite(gate).all()) and not bool((gate.max(1).values == gate.min(1).values).any())
