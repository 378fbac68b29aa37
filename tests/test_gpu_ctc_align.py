"""CTC forced alignment on the device (tavsr_ctc_align, ops.ctc_align and the layers above it) against the float64 reference of
tests/ctc_align_ref.py.  Random inputs are checked for validity and optimality (a near-tie may resolve differently in fp32);
planted, tied and tight inputs, whose path the rule fixes, are checked path for path.  One workgroup per problem: every case
is a few small launches."""
import argparse
import functools

import numpy as np
import pytest
import torch

import ctc_align_ref as R

pytestmark = pytest.mark.gpu

PLANTED = [(16, 7, 5), (17, 8, 41), (40, 15, 41), (64, 16, 65), (99, 40, 41), (300, 127, 65), (300, 128, 41), (499, 200, 500)]
INF = float("inf")


def _close(a, b, tol):
    """tests/test_gpu_ops.py:_close - the largest error over the largest reference magnitude"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    err = (a - b).abs().max() / b.abs().max().clamp_min(1e-30)
    print(f"relative error {float(err):.3e} (bound {tol:g})")
    assert err < tol, float(err)


def _close_planted(a, b, logits, T):
    """scores of planted inputs: the path's log-probabilities are ~ -1e-4 each, formed as logit - logsumexp of numbers near 12, so
    fp32 leaves an ABSOLUTE error of a few ulp(max |logit|) per frame whatever the sum's size (the relative bound above is for
    scores that are not a cancellation).  Bound: 4 ulp per frame (logsumexp 3, the subtraction 1), T frames."""
    bound = 4.0 * T * 2.0 ** -23 * float(np.abs(logits).max())
    err = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    print(f"absolute error {err:.3e} (bound {bound:.3e})")
    assert err < bound, err


def _pad(targets, Lmax=None, fill=-1):
    Lmax = max([len(t) for t in targets] + [0]) if Lmax is None else Lmax
    ys = np.full((len(targets), Lmax), fill, np.int64)
    for n, t in enumerate(targets):
        ys[n, : len(t)] = t
    return ys


def _run(logits, hlens, targets, blank=0, rows=None, route=None, Lmax=None):
    """logits: numpy [B, T, V] or a CUDA tensor (possibly a strided view); -> numpy (align, frame_lp, span, score)"""
    from tavsr import ops
    lg = logits if torch.is_tensor(logits) else torch.from_numpy(np.ascontiguousarray(logits, np.float32)).cuda()
    out = ops.ctc_align(lg, torch.tensor(hlens, dtype=torch.int64).cuda(), torch.from_numpy(_pad(targets, Lmax)).cuda(),
                        torch.tensor([len(t) for t in targets], dtype=torch.int64).cuda(), blank,
                        rows=None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda(), route=route)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _check(out, logits, hlens, targets, rows=None, exact=(), blank=0, planted=False):
    """every problem: padding, validity (align collapses to the target, span is the span of align, frame_lp is lp at align) and
    optimality (the returned path's float64 score and the returned score against the reference optimum, _close 1e-5 over the
    batch; ``planted``: _close_planted instead); problems listed in ``exact`` (or all, with exact=True): align and span equal the
    reference's"""
    align, frame_lp, span, score = out
    N, T = align.shape
    V = logits.shape[2]
    Lmax = span.shape[1]
    assert align.dtype == np.int64 and span.dtype == np.int32 and frame_lp.dtype == np.float32 and score.dtype == np.float32
    assert frame_lp.shape == (N, T) and span.shape == (N, Lmax, 2) and score.shape == (N,) and N == len(targets)
    got_path, got_score, want = [], [], []
    for n in range(N):
        r = n if rows is None else rows[n]
        Tb, tgt = max(0, min(T, int(hlens[r]))), list(targets[n])
        lp = R.log_softmax(logits[r])
        ref = R.align_ref(lp, Tb, tgt, blank, Lmax=Lmax)
        assert (align[n, Tb:] == -1).all() and (frame_lp[n, Tb:] == 0).all() and (span[n, len(tgt):] == -1).all(), n
        if ref[3] == -INF:
            assert score[n] == -INF and (align[n] == -1).all() and (frame_lp[n] == 0).all() and (span[n] == -1).all(), n
            continue
        assert R.collapse(align[n, :Tb], blank) == tgt, (n, align[n, :Tb], tgt)
        assert np.array_equal(span[n, : len(tgt)], R.spans_of_align(align[n], Tb, tgt, blank).reshape(len(tgt), 2)), n
        if Tb:
            assert np.abs(frame_lp[n, :Tb] - lp[np.arange(Tb), align[n, :Tb]]).max() < 1e-5 * max(1.0, np.abs(lp).max()), n
        got_path.append(R.path_score(lp, align[n], Tb))
        got_score.append(float(score[n]))
        want.append(ref[3])
        if exact is True or n in exact:
            assert np.array_equal(align[n], ref[0]) and np.array_equal(span[n], ref[2]), (n, align[n], ref[0])
    if want and planted:
        _close_planted(got_path, want, logits, T)
        _close_planted(got_score, want, logits, T)
    elif want:
        _close(got_path, want, 1e-5)
        _close(got_score, want, 1e-5)


@functools.lru_cache(maxsize=None)
def _planted(T, L, V):
    """three planted problems (seeds 0-2) of one shape as a batch: (logits [3, T, V], targets, planted paths)"""
    items = [R.planted(seed, T, L, V) for seed in range(3)]
    return np.stack([i[0] for i in items]), [i[1] for i in items], [i[2] for i in items]


def _planted_want(T, L, V):
    logits, targets, paths = _planted(T, L, V)
    align = np.array([[0 if s % 2 == 0 else tgt[s // 2] for s in p] for p, tgt in zip(paths, targets)], np.int64)
    span = np.stack([R.spans_of_path(p, L) for p in paths])
    return logits, targets, align, span


# ------------------------------------------------------------------------------------------------ optimality and validity
@pytest.mark.parametrize("T,L,V", [(37, 12, 41), (99, 40, 41), (130, 50, 65), (300, 128, 41), (64, 20, 500)])
def test_random_logits_give_a_valid_optimal_path(T, L, V):
    rng = np.random.default_rng(T + L + V)
    B = 4
    logits = rng.standard_normal((B, T, V)).astype(np.float32)
    hlens = [T, T - 3, max(2 * L + 1, T // 2 + L), T + 5]      # (hlens beyond T count as T)
    targets = [rng.integers(1, V, size=l).tolist() for l in (L, L - 1, L // 2, L)]
    targets[1][3] = targets[1][2]
    targets[3][1] = targets[3][0]
    _check(_run(logits, hlens, targets), logits, hlens, targets)


# ------------------------------------------------------------------------------------------------ exact paths
@pytest.mark.parametrize("T,L,V", PLANTED + [(99, 40, 5000)])
def test_planted_path_is_returned_exactly(T, L, V):
    logits, targets, want_align, want_span = _planted_want(T, L, V)
    for n in range(3):      # the reference itself returns the planted path
        ref = R.align_ref(R.log_softmax(logits[n]), T, targets[n])
        assert np.array_equal(ref[0], want_align[n]) and np.array_equal(ref[2], want_span[n])
    out = _run(logits, [T] * 3, targets)
    assert np.array_equal(out[0], want_align)
    assert np.array_equal(out[2], want_span)
    _check(out, logits, [T] * 3, targets, exact=True, planted=True)


@pytest.mark.parametrize("T,L", [(9, 3), (40, 8)])
def test_tie_rule(T, L):
    """all-zero logits: every path ties bit for bit, the rule alone decides"""
    V = 7
    logits = np.zeros((2, T, V), np.float32)
    targets = [list(range(1, L + 1)), [2] * (L // 2) + [3] * (L - L // 2)]
    out = _run(logits, [T, T - 2], targets)
    for n, Tb in enumerate((T, T - 2)):
        ref = R.align_ref(R.log_softmax(logits[n]), Tb, targets[n], T=T)
        assert np.array_equal(out[0][n], ref[0]) and np.array_equal(out[2][n], ref[2])
    _check(out, logits, [T, T - 2], targets, exact=True)


# ------------------------------------------------------------------------------------------------ edges
# (name, hlen, target): each has exactly one valid path, or none
UNIQUE = [
    ("one frame, one token", 1, [4]),
    ("one frame, no token", 1, []),
    ("Tb = L, no repeats: no blank possible", 6, [1, 2, 3, 4, 5, 6]),
    ("Tb = L + repeats: tight", 7, [1, 1, 2, 2, 3]),
    ("one frame short of tight", 6, [1, 1, 2, 2, 3]),
    ("one token five times in nine frames", 9, [3, 3, 3, 3, 3]),
    ("no frames, no token", 0, []),
    ("no frames, one token", 0, [2]),
    ("label == V", 9, [1, 7, 2]),
    ("label far beyond V", 9, [1, 2 ** 40, 2]),
    ("negative label", 9, [1, -5, 2]),
    ("blank as a label", 9, [1, 0, 2]),
]


@pytest.mark.parametrize("name,hlen,target", UNIQUE, ids=[u[0] for u in UNIQUE])
def test_edges_one_problem(name, hlen, target):
    T, V = max(hlen, 1), 7
    logits = np.random.default_rng(len(name)).standard_normal((1, T, V)).astype(np.float32)
    out = _run(logits, [hlen], [target])
    _check(out, logits, [hlen], [target], exact=True)
    assert (out[3][0] == -INF) == (not R.feasible(hlen, target, V))


def test_no_tokens_many_frames():
    logits = np.random.default_rng(0).standard_normal((2, 5, 7)).astype(np.float32)
    out = _run(logits, [5, 3], [[], []])
    assert out[2].shape == (2, 0, 2) and (out[0][0] == 0).all() and out[0][1].tolist() == [0, 0, 0, -1, -1]
    _check(out, logits, [5, 3], [[], []], exact=True)


def test_ragged_batch_mixes_every_edge():
    """all the single cases in one batch with hlens < T, random ones between them: the padding values, and an infeasible
    problem leaves its neighbours exact"""
    T, V = 12, 7
    rng = np.random.default_rng(5)
    hlens = [u[1] for u in UNIQUE] + [12, 11, 10]
    targets = [u[2] for u in UNIQUE] + [[1, 2, 3], [4, 4], [5, 6, 5, 6]]
    B = len(hlens)
    logits = rng.standard_normal((B, T, V)).astype(np.float32)
    out = _run(logits, hlens, targets)
    _check(out, logits, hlens, targets, exact=range(len(UNIQUE)))
    for n in range(B):      # every problem bit for bit what it gives alone
        alone = _run(logits[n:n + 1], hlens[n:n + 1], targets[n:n + 1], Lmax=out[2].shape[1])
        for a, b in zip(out, alone):
            assert np.array_equal(a[n:n + 1], b), n


def test_frame_counts_around_the_emission_chunk():
    from tavsr import ops
    C = ops.CTC_ALIGN_CHUNK
    for T in (C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1):
        logits, target, path = R.planted(T, T, 5, 11)
        out = _run(logits[None], [T], [target])
        assert out[0][0].tolist() == [0 if s % 2 == 0 else target[s // 2] for s in path], T
        _check(out, logits[None], [T], [target], exact=True, planted=True)
    # the utterance ends inside / at the end of a chunk of a longer batch
    logits, targets, _ = _planted(40, 15, 41)
    hlens = [C, C + 1, 2 * C]
    _check(_run(logits, hlens, [t[:5] for t in targets]), logits, hlens, [t[:5] for t in targets])


# ------------------------------------------------------------------------------------------------ strides and rows
def test_padded_rows_with_nan_in_the_padding():
    from tavsr import ops
    logits, targets, want_align, _ = _planted_want(17, 8, 41)
    V, Vp = 41, ops.pad4(41)
    assert Vp > V
    buf = torch.full((3, 17, Vp), float("nan"), device="cuda")
    buf[:, :, :V] = torch.from_numpy(logits).cuda()
    view = buf[:, :, :V]
    assert view.stride(1) == Vp and not view.is_contiguous()
    out = _run(view, [17, 15, 17], targets)
    dense = _run(logits, [17, 15, 17], targets)
    for a, b in zip(out, dense):
        assert np.array_equal(a, b)
    assert np.array_equal(out[0][0], want_align[0]) and np.isfinite(out[1]).all() and np.isfinite(out[3]).all()


def test_rows_map_problems_to_utterances():
    rng = np.random.default_rng(9)
    T, V = 30, 41
    logits = rng.standard_normal((2, T, V)).astype(np.float32)
    hlens, rows = [T, 21], [1, 1, 0]
    targets = [[3, 4, 4, 9], [7] * 12, [1, 2, 3, 4, 5, 6]]      # the second needs 23 frames of utterance 1's 21: infeasible
    out = _run(logits, hlens, targets, rows=rows)
    _check(out, logits, hlens, targets, rows=rows)
    assert out[3][1] == -INF and np.isfinite(out[3][[0, 2]]).all()
    for n, r in enumerate(rows):
        alone = _run(logits[r:r + 1], hlens[r:r + 1], [targets[n]], Lmax=12)
        for a, b in zip(out, alone):
            assert np.array_equal(a[n:n + 1], b), n


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("T,L,V", PLANTED)
def test_workspace_route_equals_lds_route(T, L, V):
    logits, targets, want_align, _ = _planted_want(T, L, V)
    hlens = [T, T - 1, T]
    lds = _run(logits, hlens, targets, route="lds")
    ws = _run(logits, hlens, targets, route="ws")
    for a, b in zip(lds, ws):
        assert np.array_equal(a, b)
    assert np.array_equal(ws[0][0], want_align[0])


def test_long_utterance_takes_the_workspace_route():
    from tavsr import ops
    from tavsr._lib import TavsrError
    T, L, V = 2000, 400, 41
    assert ops.ctc_align_lds_ok(499, 200) and not ops.ctc_align_lds_ok(T, L)
    logits, target, path = R.planted(0, T, L, V)
    out = _run(logits[None], [T], [target])
    assert out[0][0].tolist() == [0 if s % 2 == 0 else target[s // 2] for s in path]
    assert np.array_equal(out[2][0], R.spans_of_path(path, L))
    _close_planted(out[3], [R.path_score(R.log_softmax(logits), out[0][0], T)], logits, T)
    with pytest.raises(TavsrError, match="does not fit"):
        _run(logits[None], [T], [target], route="lds")


# ------------------------------------------------------------------------------------------------ capture
def test_capture_and_replay():
    from tavsr import ops
    logits, targets, want_align, _ = _planted_want(40, 15, 41)
    other = np.ascontiguousarray(logits[::-1])      # new logits for the replay: the planted paths of the batch, reversed
    static = torch.from_numpy(logits).cuda()
    hl = torch.tensor([40, 40, 40], dtype=torch.int64).cuda()
    ys, yl = torch.from_numpy(_pad(targets)).cuda(), torch.tensor([15] * 3, dtype=torch.int64).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_align(static, hl, ys, yl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ctc_align(static, hl, ys, yl)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want_align)
    static.copy_(torch.from_numpy(other).cuda())
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.ctc_align(torch.from_numpy(other).cuda(), hl, ys, yl)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert not np.array_equal(out[0].cpu().numpy(), want_align)
    _check(tuple(o.cpu().numpy() for o in out), other, [40] * 3, targets)


# ------------------------------------------------------------------------------------------------ model level
def test_model_align_on_the_fixture_model():
    from helpers import asr_conf, golden
    from oracle.model import fill_parameters_, synth
    from tavsr.tasks.asr import ASRTask
    g = golden("asr_model_3L")
    model = ASRTask.build_model(argparse.Namespace(**asr_conf(num_blocks=3, dec_blocks=2)))
    fill_parameters_(model, seed=41)
    model = model.cuda().eval()
    speech = synth((int(g["B"]), int(g["Tin"]), 80), seed=42).cuda()
    slens, tlens, text = (torch.from_numpy(g[k]).cuda() for k in ("slens", "tlens", "text"))
    align, frame_lp, span, score, olens = model.align(speech.clone(), slens, text.clone(), tlens)
    with torch.no_grad():
        enc, olens2 = model.encode(speech.clone(), slens)
        logp = model.ctc.log_softmax(enc).cpu().numpy()
    assert torch.equal(olens, olens2) and align.shape == logp.shape[:2]
    targets = [text[b, : int(tlens[b])].tolist() for b in range(text.shape[0])]
    out = tuple(o.cpu().numpy() for o in (align, frame_lp, span, score))
    _check(out, logp, olens.tolist(), targets)
    assert np.isfinite(out[3]).all()
    # no dropout in forced_align, whatever the head's rate: twice the same
    model.ctc.dropout_rate = 0.5
    again = model.align(speech.clone(), slens, text.clone(), tlens)
    assert torch.equal(again[0], align) and torch.equal(again[3], score)


def test_speech2text_timestamps():
    from helpers import TOKENS_EN, asr_conf
    from oracle.model import fill_parameters_, synth
    from tavsr.inference.beam_search import Speech2Text
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=2, dec_blocks=2)
    conf["input_size"] = None
    conf["token_list"] = TOKENS_EN
    pm = ASRTask.build_model(argparse.Namespace(**conf)).eval()
    fill_parameters_(pm, seed=5)
    pm = pm.cuda()
    wav = 0.1 * synth((2, 24000), seed=21, kind="uniform")
    lens = torch.tensor([24000, 17600])
    wav[1, 17600:] = 0
    kw = dict(beam_size=5, ctc_weight=0.3, lm_weight=0.0, penalty=0.5, nbest=2)
    plain = Speech2Text(pm, None, **kw)(wav.cuda(), lens.cuda())
    timed = Speech2Text(pm, None, timestamps=True, **kw)(wav.cuda(), lens.cuda())
    with torch.no_grad():
        enc, olens = pm.encode(wav.cuda(), lens.cuda())
        logp = pm.ctc.log_softmax(enc).cpu().numpy()
    assert len(plain) == len(timed) == 2
    seen = 0
    for u in range(2):
        assert len(plain[u]) == len(timed[u]) >= 1
        end = int(olens[u]) * 0.04
        for p, t in zip(plain[u], timed[u]):
            assert len(p) == 4 and len(t) == 5 and t[:4] == p
            rec = t[4]
            if not R.feasible(int(olens[u]), t[2], len(TOKENS_EN)):
                assert rec is None
                continue
            seen += 1
            assert [x[0] for x in rec["tokens"]] == t[1]
            prev = 0.0
            for tok, b, e, conf_ in rec["tokens"]:
                assert prev <= b < e <= end + 1e-9 and 0.0 < conf_ <= 1.0
                prev = e
            assert [w[0] for w in rec["words"]] == [w for w in "".join(t[1]).split("<space>") if w]
            for w, b, e, conf_ in rec["words"]:
                assert 0.0 <= b < e <= end + 1e-9 and 0.0 < conf_ <= 1.0
            want = R.align_ref(logp[u], int(olens[u]), t[2])[3]
            _close([rec["score"]], [want], 1e-5)
    assert seen >= 2
