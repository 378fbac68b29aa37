"""Every vocabulary-sized kernel beyond one wavefront (V > 64: BPE vocabularies of 500 / 5000 units), each against a plain
high-precision or exact reference of the same operation:

1. tavsr_ctc_loss, both kernels (LDS-resident lattice / alpha in the workspace), on either side of the dispatch threshold, against
   torch's CTC loss in float64 on the host - the tolerance is measured in the test: four times the error torch's own fp32 loss has on
   the same inputs (never less than the project's 1e-5 / 1e-4);
2. the row-wise kernels (label-smoothing loss, greedy CTC, log-softmax rows, the two Mask-CTC kernels) with more than one 64-stride,
   a partial last stride and ties / NaN that straddle strides;
3. the pre-beam inside the CTC prefix launch (three regimes of V) and the one-launch beam update with its LDS tail (K V > 1024);
4. the search end to end at V = 200 / 1000 / 5000 against the oracle, replayed graph and eager launches;
5. one training step at V = 500 against the oracle.

Oracle searches of section 4 (beam 10, length bonus 0.5, the three utterances of tests/test_gpu_search_modes.py; 16 host threads,
0.3 - 4.2 s per scorer set).  Best score of the utterance with the smallest first-to-second gap, and that gap:
    V = 200:  hybrid + LM -140.48 / 1.66e-2, CTC only -72.49 / 1.79e-3, CTC + LM -139.12 / 4.47e-2, attention only -95.08 / 6.36e-2
    V = 1000: hybrid + LM -346.63 / 6.59e-3, CTC only -101.85 / 1.96e-3
    V = 5000: hybrid + LM (parameter seed 8) -440.28 / 5.02e-2, CTC only -135.01 / 1.72e-3
- on par with the 1.28e-3 at -100.8 that tests/test_gpu_search_modes.py compares token for token.  With parameter seed 5 the
hybrid + LM search at V = 5000 finds no token >= 4096 for two utterances (largest 3904 / 4038): that case takes seed 8."""
import argparse
import functools
from itertools import groupby

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskctc_ref as R
from helpers import asr_conf, grad_ok, max_rel, rel_err, relu_gated_tol
from oracle import beam_search as BS
from oracle.model import build_asr_oracle, fill_parameters_, synth

pytestmark = pytest.mark.gpu


def _err(a, b):
    """max |a - b| / max |b|: the measure of tests/test_gpu_ops.py:_close"""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _unsupported(fn):
    """``fn`` must be refused by the library's argument check with TAVSR_EUNSUPPORTED (the check returns before any launch)"""
    from tavsr import _lib
    with pytest.raises(_lib.TavsrError) as e:
        fn()
    assert f"rc={_lib.ENUMS['TAVSR_EUNSUPPORTED']})" in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ 1. CTC loss
LDS_WORDS = 150 * 1024 // 4       # tavsr_ctc_loss takes the LDS-resident kernel up to this many 4-byte words


def _ctc_words(T, V, Lmax):
    return T * (V + 2 * (2 * Lmax + 1)) + 2 * Lmax + 1


def _ctc_batch(T, V, Lmax, blank, scale, variant, seed):
    """five utterances: 0 - every frame, a transcript of Lmax labels among them the highest label, one >= 256 and one >= 64 where V
    has them; 1 - one label, on fewer frames than T (variant 0) or on ONE frame (variant 1); 2 - more frames claimed than there are
    (clamped to T), an empty transcript (variant 0) or two labels (variant 1); 3 - a transcript with r adjacent repeats on exactly
    L + r frames: one single path; 4 - the same on L + r - 1 frames: no path (a transcript fits T frames iff L + r <= T).
    Columns past tlens hold labels too (junk the kernel must not read)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(5, T, V, generator=g) * scale
    labels = torch.tensor([v for v in range(V) if v != blank])
    ys = labels[torch.randint(0, len(labels), (5, Lmax), generator=g)]
    ys[0, 0] = labels[-1]
    for col, lo in ((1, 256), (2, 64)):
        if V > lo + 1 and Lmax > col:
            ys[0, col] = labels[labels >= lo][col]
    a, b, c = (int(v) for v in labels[[0, len(labels) // 2, -1]])
    rep = [a, a, b] if Lmax < 6 else [c, c, c, b, b, a]
    r = len(rep) - len(set(rep))
    ys[3, : len(rep)] = ys[4, : len(rep)] = torch.tensor(rep)
    hl = torch.tensor([T, 1 if variant else T - T // 3, T + 5, len(rep) + r, len(rep) + r - 1])
    tl = torch.tensor([Lmax, 1, min(2, Lmax) if variant else 0, len(rep), len(rep)])
    return logits, hl, ys, tl


def _ctc_reference(logits, hl, ys, tl, blank):
    """torch's CTC loss on the host in float64 (hlens clamped to T, as the kernel does) -> (nll, grad, e32 of the loss, e32 of the
    gradient); e32: what torch's own fp32 loss differs from it by on these inputs, in the measure of ``_err``"""
    T = logits.shape[1]
    out = []
    for dt in (torch.float64, torch.float32):
        x = logits.to(dt).requires_grad_(True)
        nll = F.ctc_loss(x.log_softmax(2).transpose(0, 1), ys, hl.clamp(max=T), tl, blank=blank, reduction="none", zero_infinity=True)
        nll.sum().backward()
        out.append((nll.detach(), x.grad))
    (nll, grad), (nll32, grad32) = out
    return nll, grad, _err(nll32, nll), _err(grad32, grad)


def _ctc_check(tag, logits, hl, ys, tl, blank, ref=None):
    """``ops.ctc_loss`` against the float64 reference within max(project floor, 4 e32); bitwise zero gradient on the frames past
    an utterance's end; run-to-run bit-equal.  Prints kernel error / e32 (profiles/r11_notes.md)."""
    from tavsr import ops
    T = logits.shape[1]
    nll_r, grad_r, e_l, e_g = ref or _ctc_reference(logits, hl, ys, tl, blank)
    dev = [t.cuda() for t in (logits, hl, ys, tl)]
    nll, g = ops.ctc_loss(*dev, blank=blank)
    k_l, k_g = _err(nll, nll_r), _err(g, grad_r)
    print(f"ctc {tag}: words {_ctc_words(T, logits.shape[2], ys.shape[1])}, loss err {k_l:.2e} (e32 {e_l:.2e}, ratio {k_l / max(e_l, 1e-30):.2f}), "
          f"grad err {k_g:.2e} (e32 {e_g:.2e}, ratio {k_g / max(e_g, 1e-30):.2f})")
    assert k_l <= max(1e-5, 4 * e_l), (k_l, e_l)
    assert k_g <= max(1e-4, 4 * e_g), (k_g, e_g)
    for b in range(logits.shape[0]):
        end = min(T, int(hl[b]))
        assert int((g[b, end:].view(torch.int32) != 0).sum()) == 0, b            # bitwise +0.0
    nll2, g2 = ops.ctc_loss(*dev, blank=blank)
    assert torch.equal(nll, nll2) and torch.equal(g, g2)
    return nll, g


@pytest.mark.parametrize("T,V,Lmax,blank,scale,variant,lds", [
    (188, 41, 40, 0, 2.0, 0, True),           # 38245 words: the last T that fits the LDS-resident kernel
    (189, 41, 40, 40, 8.0, 1, False),         # 38448: the first T that does not
    (7, 5000, 3, 0, 8.0, 1, True),            # 35105: a large vocabulary flips the dispatch at a tiny T
    (8, 5000, 3, 2500, 2.0, 0, False),        # 40119
    (61, 500, 20, 499, 2.0, 1, True),         # 35543
    (99, 300, 40, 150, 8.0, 0, False),        # 45819
])
def test_ctc_loss_both_kernels_match_float64(T, V, Lmax, blank, scale, variant, lds):
    assert (_ctc_words(T, V, Lmax) <= LDS_WORDS) == lds
    logits, hl, ys, tl = _ctc_batch(T, V, Lmax, blank, scale, variant, seed=T + V)
    assert blank not in ys.tolist()[0] and int(ys[0].max()) == max(v for v in range(V) if v != blank)
    assert V <= 65 or int((ys[0, : int(tl[0])] >= 64).sum()) >= 2
    assert V <= 257 or int((ys[0, : int(tl[0])] >= 256).sum()) >= 2
    nll_r, grad_r, e_l, e_g = ref = _ctc_reference(logits, hl, ys, tl, blank)
    # the reference side of the feasibility rows: one path / none
    assert float(nll_r[3]) > 0 and float(nll_r[4]) == 0.0 and float(grad_r[4].abs().max()) == 0.0 and float(grad_r[3].abs().max()) > 0
    nll, g = _ctc_check(f"T {T} V {V} Lmax {Lmax} blank {blank} scale {scale}", logits, hl, ys, tl, blank, ref)
    assert float(nll[4]) == 0.0 and int((g[4].view(torch.int32) != 0).sum()) == 0      # infeasible: loss and the whole row exactly 0
    assert float(nll[3]) > 0 and float(nll[2]) > 0


def test_ctc_loss_one_problem_through_both_kernels():
    """T = 99, V = 41, transcripts of up to 40 labels: as ``targets`` of width 40 the lattice fits LDS (20178 words); the same rows
    padded to width 200 with junk past tlens (Smax = 401: 83858 words) take the general kernel.  Both within the tolerance of the
    float64 reference and of each other; the junk columns change nothing, bit for bit."""
    T, V, blank = 99, 41, 0
    logits, hl, ys, tl = _ctc_batch(T, V, 40, blank, 2.0, 0, seed=99)
    assert _ctc_words(T, V, 40) <= LDS_WORDS < _ctc_words(T, V, 200) == 83858
    ref = _ctc_reference(logits, hl, ys, tl, blank)
    g = torch.Generator().manual_seed(1)
    wide = [torch.cat([ys, torch.randint(1, V, (5, 160), generator=g)], dim=1) for _ in range(2)]
    assert not torch.equal(wide[0], wide[1])
    nll_a, g_a = _ctc_check("T 99 V 41 width 40", logits, hl, ys, tl, blank, ref)
    nll_b, g_b = _ctc_check("T 99 V 41 width 200", logits, hl, wide[0], tl, blank, ref)
    nll_c, g_c = _ctc_check("T 99 V 41 width 200, other junk", logits, hl, wide[1], tl, blank, ref)
    assert torch.equal(nll_b, nll_c) and torch.equal(g_b, g_c)
    assert _err(nll_a, nll_b) <= max(1e-5, 4 * ref[2]) and _err(g_a, g_b) <= max(1e-4, 4 * ref[3])


def test_ctc_loss_refuses_a_lattice_beyond_the_general_kernels_lds():
    """T + 3 Smax floats beyond 64000 bytes (T = 15998, V = 2, Lmax = 0: 16001 floats) and too many words for the LDS-resident
    kernel: TAVSR_EUNSUPPORTED from the argument check, nothing launched - the outputs keep what they held.  Called at the C entry
    point (a [B, 0] tensor has no address to hand to ``ops.ctc_loss``)."""
    from tavsr import _lib
    T = 15998
    assert (T + 3) * 4 > 64000 and _ctc_words(T, 2, 0) > LDS_WORDS
    logits = torch.zeros(1, T, 2, device="cuda")
    hl, tl, ys = torch.tensor([T], device="cuda"), torch.tensor([0], device="cuda"), torch.zeros(1, 1, dtype=torch.int64, device="cuda")
    loss, grad, ws = torch.full((1,), 7.0, device="cuda"), torch.full((1, T, 2), 7.0, device="cuda"), torch.zeros(T, device="cuda")
    assert _lib.lib().tavsr_ctc_loss_ws(1, T, 0) == T
    rc = _lib.lib().tavsr_ctc_loss(_lib.ptr(logits), 2, T * 2, _lib.ptr(hl), _lib.ptr(ys), 1, _lib.ptr(tl), 0, 1, _lib.ptr(loss), _lib.ptr(grad),
                                   _lib.ptr(ws), 1, T, 2, 0, _lib.stream())
    assert rc == _lib.ENUMS["TAVSR_EUNSUPPORTED"], (rc, _lib.lib().tavsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((grad == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2. row-wise kernels
def _first_max(x):
    """index of the first maximum of every row, spelt out (no library arg-max): the lowest index wins among equal values"""
    V = x.shape[-1]
    top = x.max(-1, keepdim=True).values
    return torch.where(x == top, torch.arange(V), torch.full((), V)).min(-1).values


@pytest.mark.parametrize("V", [41, 64, 65, 500, 5000])
def test_lsm_loss_rows_wider_than_a_wavefront(V):
    """rows that are no multiple of the four waves of a block; smoothing 0 (the td > 0 guard); targets at V - 1 and >= 64; ignored
    rows; two equal maxima in different 64-strides AND different lanes: ``correct`` follows the lower index"""
    from tavsr import ops
    lo_i, hi_i = (3, 64 * ((V - 11) // 64) + 10) if V > 75 else (3, V - 1)          # different lanes; different strides where V > 64
    assert lo_i % 64 != hi_i % 64 and hi_i < V and (V <= 64 or lo_i // 64 != hi_i // 64)
    for rows in (1, 5, 42):
        for smoothing in (0.0, 0.1):
            g = torch.Generator().manual_seed(V + rows)
            x = torch.randn(rows, V, generator=g) * 2
            tg = torch.randint(0, V, (rows,), generator=g)
            tg[0] = lo_i                                    # the tie's lower member is the target: correct
            x[0, lo_i] = x[0, hi_i] = 30.0
            if rows > 1:
                x[1, lo_i] = x[1, hi_i] = 30.0
                tg[1] = hi_i                                # its higher member: not correct
                tg[2], tg[3], tg[4] = V - 1, min(V - 1, 64), -1
                x[3, tg[3]] += 20.0                         # a correct row with the maximum past the first stride
                tg[7::5] = -1
            row, gr, correct = ops.lsm_loss(x.cuda(), tg.cuda(), -1, smoothing)
            ign = tg == -1
            xr = x.double().requires_grad_(True)
            td = torch.full((rows, V), smoothing / (V - 1), dtype=torch.float64)
            td.scatter_(1, tg.masked_fill(ign, 0).unsqueeze(1), 1.0 - smoothing)
            lp = torch.log_softmax(xr, 1)
            kl = torch.where(td > 0, td * (td.clamp_min(1e-300).log() - lp), torch.zeros_like(lp)).masked_fill(ign.unsqueeze(1), 0).sum(1)
            kl.sum().backward()
            assert _err(row, kl.detach()) < 1e-5 and _err(gr, xr.grad) < 1e-5, (rows, smoothing)
            assert float(gr.cpu()[ign].abs().sum()) == 0.0 and float(row.cpu()[ign].abs().sum()) == 0.0
            want = torch.where(ign, torch.full_like(tg, -1), (_first_max(x) == tg).long())
            assert torch.equal(correct.cpu().long(), want), (rows, smoothing)
            assert int(want[0]) == 1 and (rows == 1 or (int(want[1]) == 0 and int(want[3]) == 1))


@pytest.mark.parametrize("T", [1, 99])
@pytest.mark.parametrize("V", [65, 500, 5000])
def test_ctc_greedy_rows_wider_than_a_wavefront(V, T):
    """ids bit-equal to the host's argmax: exact ties across strides and lanes (the lowest index), a NaN (the maximum, the rule
    tests/test_gpu_maskctc.py states), the last column; with and without lengths; the collapse against itertools.groupby"""
    from tavsr import ops
    B = 5
    x = torch.randn(B, T, V, generator=torch.Generator().manual_seed(V + T))
    if T > 3:
        x[:, ::3] = x[:, 1::3][:, : x[:, ::3].size(1)]                  # repeated frames -> repeats to collapse
    t = min(5, T - 1)
    hi_i = 64 * ((V - 11) // 64) + 10 if V > 75 else 64
    x[0, t, 3] = x[0, t, hi_i] = 50.0                                   # tie: lanes 3 / 10 (0 at V = 65), strides 0 / last
    x[1, t, V - 1] = x[1, t, 0] = 50.0                                  # ... against blank, from the last column
    x[2, t, 64 + (V > 200) * 200] = float("nan")                        # NaN past the first stride
    x[2, t, 7] = 60.0
    x[3, t, V - 1] = 50.0                                               # the last column alone
    ref = x.argmax(-1)
    assert ref[:4, t].tolist() == [3, 0, 64 + (V > 200) * 200, V - 1] and torch.equal(ref[0], _first_max(x[0]))
    hl = torch.tensor([T, max(1, (4 * T) // 5), 1, max(1, T // 2), T])
    for lens in (None, hl):
        ids, hyp, n = ops.ctc_greedy(x.cuda(), None if lens is None else lens.cuda(), 0)
        assert torch.equal(ids.cpu(), ref)
        for b in range(B):
            want = [k for k, _ in groupby(ref[b, : T if lens is None else int(lens[b])].tolist()) if k != 0]
            assert hyp[b, : int(n[b])].tolist() == want and bool((hyp[b, int(n[b]):] == -1).all())


@pytest.mark.parametrize("V", [65, 500, 5000])
def test_log_softmax_rows_wider_than_a_wavefront(V):
    """out = [out +] alpha log_softmax(x[:, :V]) [+ add] against float64.  Bound: the row's log-partition is an fp32 sum of V terms
    in 64 lanes (V / 64 + 6 additions deep) and the result goes through up to six more roundings, each 2^-24 relative to the
    largest magnitude involved: (16 + V / 64) 2^-24 max(|x|, |out|) |alpha|.  A row stride larger than V gives the same bits."""
    from tavsr import ops
    for M in (1, 5, 42):
        g = torch.Generator().manual_seed(V + M)
        x = torch.randn(M, V + 7, generator=g) * 3
        y0 = torch.randn(M, V, generator=g) * 5
        xs, xc = x.cuda(), x[:, :V].contiguous().cuda()
        lsm = torch.log_softmax(x[:, :V].double(), -1)
        for alpha, add, acc in ((1.0, 0.0, False), (0.6, 0.5, False), (0.6, 0.5, True), (1.0, 0.0, True)):
            want = (y0.double() if acc else 0.0) + alpha * lsm + add
            tol = (16 + V / 64) * 2.0 ** -24 * float(max(x.abs().max(), want.abs().max(), y0.abs().max()))
            got = ops.log_softmax_rows(xc, out=y0.clone().cuda() if acc else None, alpha=alpha, add=add, accumulate=acc)
            assert got.shape == (M, V) and float((got.cpu().double() - want).abs().max()) <= tol, (M, alpha, add, acc)
            wide = torch.full((M, V + 3), 7.0, device="cuda")
            wide[:, :V] = y0.cuda()
            out = ops.log_softmax_rows(xs, V=V, out=wide[:, :V], alpha=alpha, add=add, accumulate=acc)       # both strides > V
            assert torch.equal(out, got) and bool((wide[:, V:] == 7.0).all()), (M, alpha, add, acc)


def _maskctc_init_check(logits, hlens, thr, K, mask_token):
    """the assertions of tests/test_gpu_maskctc.py:_check_init"""
    from tavsr import ops
    B, T, V = logits.shape
    y_in, y_hat, prob, y_len, plan = (t.cpu() for t in ops.maskctc_init(logits.cuda(), hlens.cuda(), 0, mask_token, thr, K))
    for b in range(B):
        _, rh, rp = R.ctc_tokens(logits[b, : int(hlens[b])]) if int(hlens[b]) > 0 else (None, torch.zeros(0, dtype=torch.int64), torch.zeros(0))
        masked = rp.double() < thr
        n = len(rh)
        assert int(y_len[b]) == n, (b, int(y_len[b]), n)
        assert torch.equal(y_hat[b, :n], rh) and torch.equal(y_in[b, :n], torch.where(masked, torch.full_like(rh, mask_token), rh)), b
        assert plan[b].tolist() == list(R.plan_of(int(masked.sum()), K)), b
        assert np.allclose(prob[b, :n].numpy(), rp.numpy(), rtol=1e-6, atol=0), b
        assert int(y_in[b, n:].abs().sum()) == 0 and int(y_hat[b, n:].abs().sum()) == 0 and float(prob[b, n:].abs().sum()) == 0.0
    return y_len


@pytest.mark.parametrize("V", [65, 500])
def test_maskctc_init_kernel_rows_wider_than_a_wavefront(V):
    B, T = 5, 99
    logits = 3.0 * synth((B, T, V), seed=170 + V)
    logits = logits[:, torch.repeat_interleave(torch.arange(T), synth((T,), seed=71, kind="int", lo=1, hi=5))[:T]].contiguous()
    hlens = torch.tensor([T, (3 * T) // 4, T // 2, 1, T])
    logits[4, :, 0] += 30.0                                     # all blank
    logits[0, 5, V - 1] = logits[0, 5, 3] = 40.0                # a tie across strides: the lower index
    logits[1, 2, 64] = logits[1, 2, 0] = 40.0                   # ... against blank
    logits[2, 3, V - 1] = float("nan")                          # NaN is the maximum
    logits[3, 0, 64] = 40.0                                     # a one-frame utterance: token 64
    assert int(logits[0, 5].argmax()) == 3 and int(logits[1, 2].argmax()) == 0 and int(logits[2, 3].argmax()) == V - 1
    ids = torch.cat([R.ctc_tokens(logits[b, : int(hlens[b])])[1] for b in range(4)])
    assert int((ids >= 64).sum()) >= 1 and (V < 500 or (int((ids >= 64).sum()) > 10 and int((ids >= 256).sum()) > 10))
    probs = np.sort(np.concatenate([R.ctc_tokens(logits[b, : int(hlens[b])])[2].numpy() for b in (0, 1, 3)]).astype(np.float64))
    mid = len(probs) // 2
    i = mid - 3 + int(np.argmax(np.diff(probs[mid - 3: mid + 4])))
    assert probs[i + 1] - probs[i] > 1e-5                       # a threshold far from fp32 rounding of either side's probability
    for thr, K in (((probs[i] + probs[i + 1]) / 2, 10), (0.0, 10), (2.0, 3)):
        y_len = _maskctc_init_check(logits, hlens, float(thr), K, V)
    assert int(y_len[4]) == 0


@pytest.mark.parametrize("V", [65, 500])
def test_maskctc_step_kernel_rows_wider_than_a_wavefront(V):
    """decoder logits [B, L, V + 1], <mask> = V (a column past the first stride): every pass against maskctc_ref.fill_pass"""
    from tavsr import ops
    B, L, mask = 4, 61, V
    logits = synth((B, L, V + 1), seed=180 + V)
    y_in = synth((B, L), seed=81, kind="int", lo=1, hi=V)
    y_in[synth((B, L), seed=82, kind="uniform") > 0.0] = mask
    y_len = torch.tensor([61, 40, 17, 5])
    y_in[3, :5] = mask
    logits[0, int((y_in[0] == mask).nonzero()[0]), mask] = 20.0            # <mask> wins a position: it stays masked
    m1 = (y_in[1, :40] == mask).nonzero().flatten()
    logits[1, m1[0], 11] = logits[1, m1[0], V - 1] = 9.5                    # a tie inside a row across strides: the lower column
    logits[1, m1[1], 70 % V] = logits[1, m1[2], 5] = 9.5                    # equal row maxima: the lower position first
    logits[2, int((y_in[2, :17] == mask).nonzero()[0]), V - 3] = float("nan")
    logits[3, 1, V - 1] = 15.0                                              # the last token wins a position
    counts = [int((y_in[b, : int(y_len[b])] == mask).sum()) for b in range(B)]
    plans = [list(R.plan_of(counts[0], 10)), [counts[1], 3, 1000], list(R.plan_of(counts[2], 4)), list(R.plan_of(5, 10))]
    plan = torch.tensor(plans, dtype=torch.int32)
    seen_high = 0
    for it in range(0, 11):
        got = ops.maskctc_step(logits.cuda(), y_in.clone().cuda(), y_len.cuda(), plan.cuda(), it, mask).cpu()
        for b in range(B):
            n = int(y_len[b])
            want, _, _ = R.fill_pass(logits[b, :n], y_in[b, :n], mask, it, plans[b][1], min(plans[b][2], counts[b]))
            assert torch.equal(got[b, :n], want), (it, b, got[b, :n].tolist(), want.tolist())
            assert torch.equal(got[b, n:], y_in[b, n:]), (it, b)
            seen_high += int(((want != y_in[b, :n]) & (want >= 64)).sum())
    assert seen_high >= 1 and (V < 500 or seen_high > 10)                    # tokens past the first stride were filled in


# ------------------------------------------------------------------------------------------------ 3. pre-beam and beam update
@pytest.mark.parametrize("V,Cn", [(65, 1), (65, 64), (512, 15), (513, 15), (4096, 64)])
@pytest.mark.parametrize("step", [0, 2])
def test_prebeam_in_the_ctc_prefix_launch_beyond_one_wavefront(V, Cn, step):
    """tavsr_ctc_prefix_step_topk (V <= 64 / rows in registers up to 512 / rows re-read with a 64-stride ``taken`` mask up to 4096)
    against tavsr_ctc_prefix_step on the reference's candidates - a STABLE descending sort of ``full`` (torch.topk leaves the order
    of equal scores open): identical candidate lists, bit-identical forward variables and scores.  The overall winner sits in the
    last column (the partial last stride at 513, stride 63 at 4096), an exact tie has its members in different strides."""
    from tavsr import ops
    U, K, T = 2, 3, 11
    N = U * K
    g = torch.Generator().manual_seed(V + Cn)
    logp = torch.log_softmax(torch.randn(U, T, V, generator=g), -1).cuda()
    lens = torch.tensor([T, T - 4]).cuda()
    full = torch.randn(N, V, generator=g)
    lo_i, top = 5, V - 1
    if V > 128:
        hi_i = 64 * ((V - 2) // 64) - 64 + 7                                # the stride before the last one
        full[:, top] = 9.0
        full[:, lo_i] = full[:, hi_i] = 8.0
        full[1, lo_i] = full[1, hi_i] = 9.0                                 # a three-way tie at the top
        heads = [[top, lo_i, hi_i], [lo_i, hi_i, top]]
    else:
        hi_i = top                                                          # V = 65: the second stride has this one column
        full[:, lo_i] = full[:, hi_i] = 9.0
        heads = [[lo_i, hi_i], [lo_i, hi_i]]
    first = 64 * ((V - 1) // 64)                                            # first column of the last stride, where it is free
    if first not in (lo_i, hi_i, top):
        full[2, first] = 7.0
        heads.append(heads[0] + [first])
    r_prev = (-torch.rand(N, T, 2, generator=g) * 5).cuda()
    s_prev = (-torch.rand(N, generator=g) * 3).cuda()
    tok = torch.randint(1, V, (N,), generator=g).cuda()
    cand0 = torch.sort(full, dim=-1, descending=True, stable=True)[1][:, :Cn]
    assert lo_i // 64 != hi_i // 64 and top // 64 >= min(8, (V - 1) // 64)
    for row, head in enumerate(heads):
        assert cand0[row, : len(head)].tolist() == head[:Cn], (row, cand0[row, :4].tolist(), head)
    want = ops.ctc_prefix_step(logp, lens, r_prev, s_prev, tok, cand0.cuda(), K, step)
    got = ops.ctc_prefix_step_topk(logp, lens, r_prev, s_prev, tok, full.cuda(), Cn, K, step)
    assert torch.equal(got[0].cpu(), cand0)
    for a, b in zip(got[1:], want):
        assert torch.equal(a, b)


def test_prebeam_in_the_ctc_prefix_launch_refuses_what_it_cannot_select():
    from tavsr import ops
    U, K, T = 1, 2, 5
    for V, Cn in ((4097, 15), (100, 65)):
        logp = torch.log_softmax(torch.randn(U, T, V), -1).cuda()
        state = (logp, torch.tensor([T]).cuda(), torch.zeros(K, T, 2).cuda(), torch.zeros(K).cuda(), torch.ones(K, dtype=torch.int64).cuda())
        _unsupported(lambda: ops.ctc_prefix_step_topk(*state, torch.randn(K, V).cuda(), Cn, K, 1))
    torch.cuda.synchronize()


def _beam_inputs(U, K, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    N = U * K
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(full=r(N, V) * 3 - 5, cand=torch.stack([torch.randperm(V, generator=g)[:C] for _ in range(N)]), psi=r(N, C) * 4 - 20,
             psi_abs=r(N, C) * 4 - 40, eos_s=r(N) * 3 - 10, eos_abs=r(N) * 3 - 30, s_prev=r(N) * 3 - 20, score=r(N) * 5 - 30)
    return t


def _beam_weighted(t, eos, w_ctc, ctc):
    """the torch expression of ``BatchBeamSearch._beam_update_eager`` (on the device: separately rounded fp32 operations)"""
    d = {k: v.cuda() for k, v in t.items()}
    if not ctc:
        return d["full"] + d["score"].unsqueeze(1), None
    is_eos_c = d["cand"] == eos
    psi = torch.where(is_eos_c, d["eos_s"].unsqueeze(1), d["psi"])
    ctc_full = torch.full(d["full"].shape, -10000000000.0, device="cuda") - d["s_prev"].unsqueeze(1)
    ctc_full[:, eos] = d["eos_s"]
    ctc_full.scatter_(1, d["cand"], psi)
    return d["full"] + w_ctc * ctc_full + d["score"].unsqueeze(1), torch.where(is_eos_c, d["eos_abs"].unsqueeze(1), d["psi_abs"])


@pytest.mark.parametrize("ctc", [True, False])
@pytest.mark.parametrize("K,V", [(10, 103), (10, 200), (16, 512), (3, 2730)])
def test_one_launch_beam_update_with_scores_left_in_lds(K, V, ctc):
    """tavsr_beam_combine_topk with K V = 1030 / 2000 / 8192 / 8190 > 1024: a lane keeps 16 scores in registers, the rest stay in LDS.
    Reference: the torch expression and a stable descending sort.  Input conditions, asserted on the reference: at least two winners
    at flat index >= 1024, two winners of one lane (index % 64) of which at least one is an LDS element - both LDS elements where
    K V leaves room for that (K V = 1030 has only lanes 0-5 past 1024, once each) - and, in utterance 0, an exact tie with one member
    below 1024 and one above, both of lane 3 (at K = 3 the upper member is the first loser: the tie decides the last winner).  ``weighted`` bit-equal; then tavsr_beam_reorder's slot arithmetic on these indices."""
    from tavsr import ops
    U, C, eos, w_ctc = 2, 15, V - 1, 0.2
    N, KV = U * K, K * V
    t = _beam_inputs(U, K, V, C, seed=K + V + ctc)
    t["cand"][K + 1, 2] = eos                                               # (utterance 1: not a row the winners below take)
    # winners of utterance 0, best first: b, c >= 1024, then a < 1024 tied with d >= 1024 - a register and an LDS element of ONE
    # lane (3), so the lane's own scan has to keep the lower index too.  b and c share a lane where K V has room for that
    a, d = 64 * 3 + 3, KV - 1 - (KV - 4) % 64
    b, c = (1024 + 2, 1024 + 4) if KV < 1024 + 70 else (1024 + 64 * 2 + 9, 1024 + 64 * 5 + 9)
    assert a % 64 == d % 64 == 3 and d >= 1024 and d not in (b, c)
    rows = {}
    for flat, value in ((b, 40.0), (c, 38.0), (a, 36.0), (d, 36.0)):
        assert flat % V != eos
        t["full"][flat // V, flat % V] = value
        rows.setdefault(flat // V, []).append(flat % V)
    for k, toks in rows.items():                                            # their slots: one score, the winners among the candidates
        t["score"][k] = -20.0
        t["cand"][k] = torch.tensor(toks + [v for v in range(V - 1) if v not in toks][: C - len(toks)])
        t["psi"][k, : len(toks)] = -5.0
    want, pa_want = _beam_weighted(t, eos, w_ctc, ctc)
    vals, order = torch.sort(want.view(U, KV).cpu(), dim=-1, descending=True, stable=True)
    top_i, top_s = order[:, :K], vals[:, :K]
    w0 = top_i[0].tolist()
    assert w0[:4] == [b, c, a, d][:K] and float(want.view(U, KV)[0, a]) == float(want.view(U, KV)[0, d]) and a < 1024 <= d      # (K = 3: d is the first loser)
    high = [i for i in w0 if i >= 1024]
    assert len(high) >= 2 and any(i % 64 == j % 64 for i in high for j in w0 if i != j)
    assert KV < 1024 + 70 or any(i % 64 == j % 64 for i in high for j in high if i != j)
    d_ = {k_: v_.cuda() for k_, v_ in t.items()}

    def operands():
        return (d_["cand"], d_["psi"], d_["psi_abs"].clone(), d_["eos_s"], d_["eos_abs"], d_["s_prev"]) if ctc else (None,) * 6

    o = operands()
    ts, ti, w = ops.beam_combine_topk(d_["full"], *o, d_["score"], eos, w_ctc, K, keep_weighted=True)
    assert torch.equal(w, want)
    assert ti.cpu().tolist() == top_i.tolist() and torch.equal(ts.cpu(), top_s)
    if ctc:
        assert torch.equal(o[2], pa_want) and not torch.equal(pa_want, d_["psi_abs"])
    ts2, ti2 = ops.beam_combine_topk(d_["full"], *operands(), d_["score"], eos, w_ctc, K)          # without the ``weighted`` output
    assert torch.equal(ti2, ti) and torch.equal(ts2, ts)
    # re-ordering on these indices (no CTC state): slot = top_i / V, token = top_i % V
    steps, i = 6, 3
    g = torch.Generator().manual_seed(3)
    yseq = torch.randint(0, V, (N, steps + 2), generator=g).cuda()
    anc = torch.randint(0, 1000, (N, steps), dtype=torch.int32, generator=g).cuda()
    ctr = torch.tensor([i, i + 1], dtype=torch.int64).cuda()
    outs = (None, None, torch.empty_like(yseq), torch.empty_like(anc), torch.empty(N, dtype=torch.int64).cuda(), torch.empty(N).cuda())
    ops.beam_reorder(ti, ts, None, None, None, yseq, anc, outs, K, V, ctr.view(torch.int32)[0:1])
    prev = (ti // V + (torch.arange(U).cuda() * K).view(U, 1)).view(N)
    new_tok = (ti % V).view(N)
    y_want = yseq[prev]
    y_want[:, i + 1] = new_tok
    for got, exp in zip(outs[2:], (y_want, anc[prev], new_tok, ts.view(N))):
        assert torch.equal(got, exp)
    assert int(new_tok.max()) >= 64 and int(prev.max()) > 0


@pytest.mark.parametrize("ctc", [True, False])
def test_beam_update_too_large_for_one_launch_is_refused_and_its_first_half_equals_torch(ctc):
    """K V = 10000 > 8192: tavsr_beam_combine_topk refuses; the search then runs tavsr_beam_combine + torch.topk"""
    from tavsr import ops
    U, K, V, C, w_ctc = 2, 10, 1000, 15, 0.2
    eos = V - 1
    t = _beam_inputs(U, K, V, C, seed=7)
    t["cand"][3, 2] = eos
    t["score"][5] = -float("inf")
    assert not ops.beam_combine_topk_ok(K, V) and ops.beam_combine_topk_ok(16, 512) and ops.beam_combine_topk_ok(10, 819)
    want, pa_want = _beam_weighted(t, eos, w_ctc, ctc)
    d_ = {k_: v_.cuda() for k_, v_ in t.items()}
    args = lambda: (d_["cand"], d_["psi"], d_["psi_abs"].clone(), d_["eos_s"], d_["eos_abs"], d_["s_prev"]) if ctc else (None,) * 6
    _unsupported(lambda: ops.beam_combine_topk(d_["full"], *args(), d_["score"], eos, w_ctc, K))
    a = args()
    assert torch.equal(ops.beam_combine(d_["full"], *a, d_["score"], eos, w_ctc), want)
    assert not ctc or torch.equal(a[2], pa_want)


# ------------------------------------------------------------------------------------------------ 4. search end to end
LM_KW = dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0)
BEAM, PEN = 10, 0.5
# scorer sets: name -> (decoder, ctc, lm weight, ctc_weight of the product model's conf, ctc_weight of the search)
SCORERS = {"hybrid_lm": (True, True, 0.6, None, 0.3), "ctc": (False, True, 0.0, 1.0, 1.0), "ctc_lm": (False, True, 0.6, 1.0, 1.0),
           "attention": (True, False, 0.0, 0.0, 0.0)}


def _tokens(V):
    return ["<blank>", "<unk>"] + [f"u{i}" for i in range(2, V - 1)] + ["<sos/eos>"]


@functools.lru_cache(maxsize=None)
def _oracle(V, seed):
    m = build_asr_oracle(asr_conf(num_blocks=2, dec_blocks=2), _tokens(V)).eval()
    fill_parameters_(m, seed=seed)
    lm = BS.TransformerLMOracle(V, **LM_KW).eval()
    fill_parameters_(lm, seed=seed + 1)
    x = synth((3, 160, 80), seed=7)
    with torch.no_grad():
        enc, olens = m.encode(x, torch.tensor([160, 120, 88]))
    return m, lm, enc, olens


@functools.lru_cache(maxsize=None)
def _product(V, seed, model_ctc_weight):
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=2, dec_blocks=2)
    if model_ctc_weight is not None:
        conf["model_conf"]["ctc_weight"] = model_ctc_weight
    conf["token_list"] = _tokens(V)
    pm = ASRTask.build_model(argparse.Namespace(**conf)).eval()
    fill_parameters_(pm, seed=seed)
    return pm.cuda()


@functools.lru_cache(maxsize=None)
def _product_lm(V, seed):
    from tavsr.lm.transformer_lm import TransformerLM
    plm = TransformerLM(V, **LM_KW).eval()
    fill_parameters_(plm, seed=seed + 1)
    return plm.cuda()


@functools.lru_cache(maxsize=None)
def _reference(V, seed, name):
    """the oracle's search with the reduced scorer dict, one utterance at a time (tests/test_gpu_search_modes.py:_reference)"""
    decoder, ctc, lm_w, _, ctc_w = SCORERS[name]
    m, lm, enc, olens = _oracle(V, seed)
    scorers = dict(decoder=BS.DecoderScorer(m.decoder) if decoder else None, ctc=BS.CTCPrefixScorer(ctc=m.ctc, eos=m.eos) if ctc else None,
                   length_bonus=BS.LengthBonus(V), lm=lm if lm_w else None)
    weights = dict(decoder=1.0 - ctc_w, ctc=ctc_w, lm=lm_w, length_bonus=PEN)
    out = []
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))         # one-token steps on [10, 256] rows: more host threads only add wake-ups
    try:
        with torch.no_grad():
            for u in range(3):
                bs = BS.BatchBeamSearch(scorers, weights, BEAM, V, m.sos, m.eos, pre_beam_score_key=None if ctc_w == 1.0 else "full")
                hyps = bs.forward(enc[u, : int(olens[u])], maxlenratio=0.0)
                out.append([(h.yseq.tolist(), float(h.score)) for h in hyps])
    finally:
        torch.set_num_threads(nthreads)
    return out


def _check_against_reference(hip, ref):
    """tests/test_gpu_search_modes.py:_check_against_reference"""
    for u in range(3):
        assert len(hip[u]) > 0 and len(ref[u]) > 0
        assert hip[u][0][0] == ref[u][0][0], (u, hip[u][0], ref[u][0])
        print(f"utterance {u}: best score {hip[u][0][1]:.6f}, oracle {ref[u][0][1]:.6f}, rel {abs(hip[u][0][1] - ref[u][0][1]) / abs(ref[u][0][1]):.2e}")
        assert abs(hip[u][0][1] - ref[u][0][1]) < 2e-4 * abs(ref[u][0][1])
        top_h = {tuple(h[0]) for h in hip[u][:3]}
        top_r = {tuple(h[0]) for h in ref[u][:3]}
        assert len(top_h & top_r) >= 2, (u, top_h, top_r)


@pytest.mark.parametrize("V,seed,name", [(200, 5, "hybrid_lm"), (200, 5, "ctc"), (200, 5, "ctc_lm"), (200, 5, "attention"),
                                         (1000, 5, "hybrid_lm"), (1000, 5, "ctc"), (5000, 8, "hybrid_lm"), (5000, 5, "ctc")])
def test_search_with_a_large_vocabulary_matches_oracle(monkeypatch, V, seed, name):
    """the route of every BPE model: no one-launch CTC search and no one-launch beam update behind the scorers (both V <= 64), so a
    captured step for every scorer set; the pre-beam inside the CTC launch up to V = 4096, behind torch.topk above; the beam update
    in one launch while K V <= 8192, tavsr_beam_combine + torch.topk above.  Replayed graph and eager launches give the same lists."""
    from tavsr import ops
    from tavsr.inference import beam_search as PBS
    decoder, ctc, lm_w, model_w, ctc_w = SCORERS[name]
    ref = _reference(V, seed, name)
    # input conditions: every best hypothesis of the oracle holds tokens a kernel blind past a stride / a register row would miss
    for u in range(3):
        toks = [t for t in ref[u][0][0] if t != V - 1]
        for bar in (64, 512, 4096):
            assert bar >= V or any(t >= bar for t in toks), (u, bar, toks)
        print(f"utterance {u}: oracle score {ref[u][0][1]:.3f}, gap to the second hypothesis {ref[u][0][1] - ref[u][1][1]:.3e}, {len(toks)} tokens, max {max(toks)}")
    _, _, enc, olens = _oracle(V, seed)
    T = enc.shape[1]
    assert not ops.ctc_beam_search_ok(BEAM, V, T) and not ops.beam_select_topk_ok(BEAM, V)
    assert ops.beam_combine_topk_ok(BEAM, V) == (V == 200) and PBS.PREBEAM_FUSED and PBS.CTC_SEARCH_FUSED and PBS.CTC_BESIDE_SCORERS
    pm, plm = _product(V, seed, model_w), _product_lm(V, seed) if lm_w else None
    outs = []
    for graph in (True, False):
        monkeypatch.setattr(PBS, "GRAPH_STEP", graph)
        search = PBS.BatchBeamSearch(pm, plm, BEAM, ctc_w, lm_w, PEN)
        assert search.has_dec == decoder and search.has_ctc == ctc and search.has_lm == bool(lm_w)
        assert search.pre_beam == (name == "hybrid_lm") and (not ctc or search.C == (15 if search.pre_beam else V))
        outs.append(search.decode(enc.cuda(), olens.cuda()))
        assert (search._captured is not None and search._captured.graph is not None) == graph       # even CTC only: a captured step
        _check_against_reference(outs[-1], ref)
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ 5. a training step
def test_training_step_at_500_units_matches_oracle():
    """2 + 2 blocks, B = 3, ragged, T = 39 / 29 / 21 frames behind the subsampling: loss, its CTC and attention parts, accuracy and
    every parameter gradient against the oracle at the tolerances of tests/test_gpu_parity.py:test_full_size_vs_oracle_cfg2 - the one
    place where the output projections, the embedding's backward and both loss heads meet at N = V = 500.  Greedy CTC ids of the same
    model are bit-exact where the oracle's top-2 logit gap is binding (1e-4)."""
    from tavsr.tasks.asr import ASRTask
    V = 500
    oracle = build_asr_oracle(asr_conf(num_blocks=2, dec_blocks=2), _tokens(V)).train()
    fill_parameters_(oracle, seed=21)
    conf = asr_conf(num_blocks=2, dec_blocks=2)
    conf["token_list"] = _tokens(V)
    model = ASRTask.build_model(argparse.Namespace(**conf))
    model.load_state_dict(oracle.state_dict())
    model = model.cuda().train()
    speech, slens = synth((3, 160, 80), seed=22), torch.tensor([160, 120, 88])
    text, tlens = synth((3, 9), seed=23, kind="int", lo=1, hi=V - 1), torch.tensor([9, 6, 4])
    text[0, :3] = torch.tensor([V - 2, 300, 64])
    for i, l in enumerate(tlens):
        text[i, int(l):] = -1
    lo, so, _ = oracle(speech, slens, text, tlens)
    lo.backward()
    lg, sg, _ = model(speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda())
    lg.backward()
    assert rel_err(lg.detach().cpu(), lo.detach()) < 1e-4
    for key in ("loss_ctc", "loss_att"):
        assert rel_err(torch.as_tensor(sg[key]).cpu(), torch.as_tensor(so[key])) < 1e-4, key
    assert abs(float(sg["acc"]) - float(so["acc"])) < 1e-6
    po = dict(oracle.named_parameters())
    worst = 0.0
    for n, p in model.named_parameters():
        assert grad_ok(p.grad.cpu(), po[n].grad, relu_gated_tol(n, 5e-3)), n
        if float(po[n].grad.abs().max()) > 1e-6:
            worst = max(worst, rel_err(p.grad.cpu(), po[n].grad))
    print("worst grad rel err", worst)
    for n in ("ctc.ctc_lo.weight", "decoder.output_layer.weight", "decoder.embed.0.weight"):
        assert po[n].shape[0] == V and float(po[n].grad[64:].abs().max()) > 0, n
    with torch.no_grad():
        eo, _ = oracle.eval().encode(speech, slens)
        eg, ol = model.eval().encode(speech.cuda(), slens.cuda())
        logits = oracle.ctc.ctc_lo(eo)
        top2 = logits.topk(2, -1).values
        binding = (top2[..., 0] - top2[..., 1]) > 1e-4
        ids, hyp, hl = model.ctc.greedy(eg, ol)
    assert max_rel(eg.cpu(), eo) < 1e-4 and float(binding.float().mean()) > 0.98
    assert torch.equal(ids.cpu()[binding], logits.argmax(-1)[binding]) and int(logits.argmax(-1).max()) >= 256
    if bool(binding.all()):
        want = oracle.ctc_greedy(speech, slens)
        assert [hyp[b, : int(hl[b])].tolist() for b in range(3)] == want
