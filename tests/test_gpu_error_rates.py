"""GPU: the device route of the validation error rates (csrc/editdist.hip) - ``ops.edit_distance_rows`` against the numpy
restatement, ``ErrorCalculator`` on the device against its own host route, the refusal beyond ``tavsr_error_counts_ok``, graph
capture, and whole models with the switch on against off.  The results are integers (or one IEEE division of two of them):
every comparison is ``==``."""
import argparse
import random

import numpy as np
import pytest
import torch

import error_rates_ref as R
from helpers import AVSR_YAML, TOKENS_EN, asr_conf, avsr_conf

pytestmark = pytest.mark.gpu

LISTS = {"en": (TOKENS_EN, "<space>", "<blank>"), "bpe": (R.TOKENS_BPE,) + R.TOKENS_BPE_SYMS,
         "underbar": (R.TOKENS_BPE,) + R.TOKENS_UNDERBAR_SYMS}
STRIP = 256      # threads of a workgroup: the cells of one anti-diagonal are dealt out in strips of this length


def _distances(pairs, pad_h=5, pad_r=3, garbage=(7, 11)):
    """(device result, reference) for a list of (hyp, ref) symbol lists: rows of wider buffers whose leading dimensions exceed
    the row lengths, with symbols of the pairs' own alphabet behind every length (reading them would change a distance)"""
    from tavsr import ops
    B = len(pairs)
    n, m = max(len(h) for h, _ in pairs), max(len(r) for _, r in pairs)
    hyp = np.full((B, n + pad_h), garbage[0], dtype=np.int32)
    ref = np.full((B, m + pad_r), garbage[1], dtype=np.int32)
    for b, (h, r) in enumerate(pairs):
        hyp[b, :len(h)] = h
        hyp[b, len(h):] = (r + h + [garbage[0]])[0]
        ref[b, :len(r)] = r
        ref[b, len(r):] = (h + r + [garbage[1]])[0]
    hl = torch.tensor([len(h) for h, _ in pairs], dtype=torch.int32).cuda()
    rl = torch.tensor([len(r) for _, r in pairs], dtype=torch.int32).cuda()
    got = ops.edit_distance_rows(torch.from_numpy(hyp).cuda()[:, :n], hl, torch.from_numpy(ref).cuda()[:, :m], rl)
    assert got.dtype == torch.int32 and got.shape == (B,)
    return got.cpu().tolist(), [R.levenshtein(h, r) for h, r in pairs]


def _rand(rng, n, k):
    return [rng.randrange(k) for _ in range(n)]


LENGTHS = [0, 1, 2, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1]


@pytest.mark.parametrize("n", LENGTHS)
def test_edit_distance_rows_at_every_length_edge(n):
    """a pair of (n, m) for m through every edge length, in batches of two: (n, m) and (m, n)"""
    rng = random.Random(100 + n)
    for m in LENGTHS:
        a, b = _rand(rng, n, 5), _rand(rng, m, 5)
        got, want = _distances([(a, b), (b, a)])
        assert got == want, (n, m)


def test_edit_distance_rows_lopsided_long_and_degenerate_pairs():
    rng = random.Random(7)
    long_a, long_b = _rand(rng, 2 * STRIP + 1, 4), _rand(rng, 3, 4)
    got, want = _distances([(long_a, long_b), (long_b, long_a)])      # n >> m and m >> n, past two strips
    assert got == want
    same = _rand(rng, 70, 9)
    pairs = [([], []), ([], same), (same, []), (same, list(same)), (same, [x + 100 for x in same]), ([1], [1]), ([1], [2]),
             (same[:-1], same), (same, same[1:])]
    got, want = _distances(pairs)
    assert got == want and want[:5] == [0, 70, 70, 0, 70]


def test_edit_distance_rows_two_symbol_alphabet_and_full_code_point_range():
    rng = random.Random(8)
    pairs = [(_rand(rng, rng.randrange(0, 80), 2), _rand(rng, rng.randrange(0, 80), 2)) for _ in range(12)]      # many tied moves
    got, want = _distances(pairs, garbage=(0, 1))
    assert got == want
    wide = [0, 1, 0x20, 0xFFFF, 0x10000, 0x10FFFE, 0x10FFFF]
    pairs = [([rng.choice(wide) for _ in range(40)], [rng.choice(wide) for _ in range(37)]) for _ in range(4)]
    got, want = _distances(pairs, garbage=(0x10FFFF, 0x10FFFF))
    assert got == want


@pytest.mark.parametrize("B", [1, 70])
def test_edit_distance_rows_batches(B):
    rng = random.Random(9 + B)
    pairs = [(_rand(rng, rng.randrange(0, 81), 6), _rand(rng, rng.randrange(0, 81), 6)) for _ in range(B)]
    got, want = _distances(pairs, pad_h=17, pad_r=0)
    assert got == want


def test_edit_distance_rows_refuses_rows_beyond_its_lds_bound():
    from tavsr import ops
    from tavsr._lib import ENUMS, TavsrError, lib
    z = torch.zeros((1, 13653), dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    dist = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = lib().tavsr_edit_distance_rows(z.data_ptr(), 13653, one.data_ptr(), 13653, z.data_ptr(), 13653, one.data_ptr(), 13653,
                                        dist.data_ptr(), 1, ops.stream())
    torch.cuda.synchronize()
    assert rc == ENUMS["TAVSR_EUNSUPPORTED"] and int(dist) == -7
    with pytest.raises(TavsrError):
        ops.edit_distance_rows(z, one, z, one)
    assert ops.edit_distance_rows(z[:, :5], one, z[:, :13652], one).tolist() == [0]


# ---------------------------------------------------------------------------------------------- ErrorCalculator
def _batch(V, blank, space, unk, B, T, L, seed):
    """hypothesis rows with runs, blanks, spaces and <unk>; references padded with -1 at different lengths, one of them empty and
    one made of blank / space alone (empty for cer_ctc only); the attention hypothesis is a noisy copy of the reference"""
    g = torch.Generator().manual_seed(seed)
    ys_hat = torch.randint(0, V, (B, T), generator=g)
    ys_hat = ys_hat[:, torch.randint(0, T, (T,), generator=g).sort().values]      # repeated columns: runs
    for tok, p in ((blank, 0.3), (space, 0.1), (unk, 0.05)):
        ys_hat[torch.rand((B, T), generator=g) < p] = tok
    ys_pad = torch.randint(0, V, (B, L), generator=g)
    ys_pad[torch.rand((B, L), generator=g) < 0.2] = space
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1 % B] = L, 0
    ys_pad[torch.arange(L)[None, :] >= lens[:, None]] = -1
    if B > 2:
        ys_pad[2, :lens[2]] = torch.tensor([blank, space])[torch.arange(int(lens[2])) % 2]
    if B > 3:      # an id behind the first -1: it ends the hypothesis cut but still belongs to the reference
        ys_pad[3, L - 3:] = torch.tensor([-1, unk, -1])
    att = torch.cat([ys_pad, ys_pad[:, :1]], 1).clamp_min(0)
    noise = torch.randint(0, V, att.shape, generator=g)
    att = torch.where(torch.rand(att.shape, generator=g) < 0.3, noise, att)
    return ys_hat, att, ys_pad


@pytest.mark.parametrize("report_cer,report_wer", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_error_calculator_device_route_equals_host_route(name, report_cer, report_wer):
    """T = 301 frames: more positions than threads, not a multiple of them; L = 19"""
    from tavsr import ops
    from tavsr.models.espnet_model import ErrorCalculator
    tokens, space, blank = LISTS[name]
    calc = ErrorCalculator(tokens, space, blank, report_cer, report_wer)
    space_id = tokens.index(space) if space in tokens else tokens.index("<space>")
    ys_hat, att, ys_pad = _batch(len(tokens), tokens.index(blank), space_id, tokens.index("<unk>"), 7, 301, 19, seed=21)
    want_ctc, want_att = calc.cer_ctc(ys_hat, ys_pad), calc(att, ys_pad)
    assert isinstance(want_ctc, float)
    d_hat, d_att, d_pad = ys_hat.cuda(), att.cuda(), ys_pad.cuda()
    got_ctc, got_att = calc(d_hat, d_pad, is_ctc=True), calc(d_att, d_pad)
    assert got_ctc.is_cuda and got_ctc.dtype == torch.float64 and got_ctc.dim() == 0
    assert float(got_ctc) == want_ctc
    for got, want, on in zip(got_att, want_att, (report_cer, report_wer)):
        assert (got is None and want is None) if not on else (got.is_cuda and got.dtype == torch.float64 and float(got) == want)
    for mode, hat, d in (("ctc_chars", ys_hat, d_hat), ("att_chars", att, d_att), ("att_words", att, d_att)):
        errs, ref_n = calc.counts(d, d_pad, mode)
        assert errs.is_cuda and errs.dtype == ref_n.dtype == torch.int32
        host = calc.counts(hat, ys_pad, mode)
        assert (errs.tolist(), ref_n.tolist()) == (host[0].tolist(), host[1].tolist()), mode
        assert (errs.tolist(), ref_n.tolist()) == R.counts(tokens, space, blank, hat.tolist(), ys_pad.tolist(), mode), mode
    ops.DEVICE_ERROR_RATES = False      # the switch: CUDA tensors through the host route
    try:
        off = calc(d_hat, d_pad, is_ctc=True)
    finally:
        ops.DEVICE_ERROR_RATES = True
    assert isinstance(off, float) and off == want_ctc


def test_error_calculator_long_reference_rows_and_empty_references():
    """L = 260: more reference positions than threads; then a batch whose references are all empty: NaN where the host gives
    None (cer_ctc) or raises ZeroDivisionError (cer, wer)"""
    from tavsr.models.espnet_model import ErrorCalculator
    calc = ErrorCalculator(TOKENS_EN, "<space>", "<blank>", True, True)
    ys_hat, att, ys_pad = _batch(len(TOKENS_EN), 0, TOKENS_EN.index("<space>"), 1, 3, 37, 260, seed=22)
    want = (calc.cer_ctc(ys_hat, ys_pad),) + calc(att, ys_pad)
    got = (calc(ys_hat.cuda(), ys_pad.cuda(), is_ctc=True),) + calc(att.cuda(), ys_pad.cuda())
    assert tuple(float(x) for x in got) == want
    empty = torch.full((2, 5), -1)
    assert calc.cer_ctc(ys_hat[:2], empty) is None
    with pytest.raises(ZeroDivisionError):
        calc(att[:2], empty)
    got = (calc(ys_hat[:2].cuda(), empty.cuda(), is_ctc=True),) + calc(att[:2].cuda(), empty.cuda())
    assert all(x.is_cuda and bool(torch.isnan(x)) for x in got)


def test_error_counts_refuses_a_shape_past_its_bound_and_the_calculator_takes_the_host_route():
    from tavsr import ops
    from tavsr._lib import ENUMS, TavsrError, lib
    from tavsr.models.espnet_model import ErrorCalculator
    calc = ErrorCalculator(TOKENS_EN, "<space>", "<blank>", True, True)
    B, T, L = 2, 5000, 5000      # 5000 reference positions of up to 9 characters: 45000 symbols, past the 40960 words of LDS
    assert ops.error_counts_ok(1, 32, 499, 200, 9) and ops.error_counts_ok(6, 32, 201, 200, 9)
    assert not ops.error_counts_ok(1, B, T, L, 9)
    g = torch.Generator().manual_seed(23)
    ys_hat = torch.zeros((B, T), dtype=torch.int64)
    ys_hat[:, ::97] = torch.randint(1, 40, (B, len(range(0, T, 97))), generator=g)
    ys_pad = torch.full((B, L), -1)
    ys_pad[:, :40] = torch.randint(1, 40, (B, 40), generator=g)
    d_hat, d_pad = ys_hat.cuda(), ys_pad.cuda()
    small = calc(d_hat[:, :100], d_pad[:, :100], is_ctc=True)      # builds the device tables
    assert small.is_cuda
    tb = calc._device_tables[d_hat.device]
    errs = torch.full((1, B), -7, dtype=torch.int32, device="cuda")
    ref_n = torch.full((1, B), -7, dtype=torch.int32, device="cuda")
    rc = lib().tavsr_error_counts(d_hat.data_ptr(), T, T, d_pad.data_ptr(), L, L, tb.span.data_ptr(), tb.cps.data_ptr(),
                                  tb.cp_space.data_ptr(), tb.drop.data_ptr(), tb.V, tb.tok_max, 1, errs.data_ptr(), ref_n.data_ptr(), B,
                                  ops.stream())
    torch.cuda.synchronize()
    assert rc == ENUMS["TAVSR_EUNSUPPORTED"] and errs.tolist() == [[-7] * B] and ref_n.tolist() == [[-7] * B]
    with pytest.raises(TavsrError):
        ops.error_counts(d_hat, d_pad, tb, 1)
    got = calc(d_hat, d_pad, is_ctc=True)
    assert isinstance(got, float) and got == calc.cer_ctc(ys_hat, ys_pad)


def test_error_calculator_call_is_capturable_and_a_replay_follows_new_inputs():
    from tavsr.models.espnet_model import ErrorCalculator
    tokens, space, blank = LISTS["bpe"]
    calc = ErrorCalculator(tokens, space, blank, True, True)
    batches = [_batch(len(tokens), 0, 2, 1, 5, 90, 12, seed=s) for s in (31, 32)]
    s_hat, s_att, s_pad = (t.cuda() for t in batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # first call outside the capture: the device tables, the LDS opt-in
        calc(s_hat, s_pad, is_ctc=True), calc(s_att, s_pad)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = (calc(s_hat, s_pad, is_ctc=True),) + calc(s_att, s_pad)
    for ys_hat, att, ys_pad in (batches[1], batches[0]):
        s_hat.copy_(ys_hat), s_att.copy_(att), s_pad.copy_(ys_pad)
        graph.replay()
        torch.cuda.synchronize()
        assert tuple(float(x) for x in out) == (calc.cer_ctc(ys_hat, ys_pad),) + calc(att, ys_pad)


# ---------------------------------------------------------------------------------------------- models
def _stats_equal(on, off):
    assert on.keys() == off.keys()
    for k in on:
        a, b = on[k], off[k]
        if k.startswith("cer") or k == "wer":
            assert torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float64 and isinstance(b, float), k
            assert float(a) == b, k
        elif a is None or b is None:
            assert a is None and b is None, k
        elif torch.is_tensor(a):
            assert torch.equal(a, b), k
        else:
            assert float(a) == float(b), k


def _both_routes(fn):
    from tavsr import ops
    assert ops.DEVICE_ERROR_RATES
    on = fn()
    ops.DEVICE_ERROR_RATES = False
    try:
        off = fn()
    finally:
        ops.DEVICE_ERROR_RATES = True
    return on, off


def _asr_model():
    from oracle.model import fill_parameters_
    from tavsr.tasks.asr import ASRTask
    conf = asr_conf(num_blocks=2, dec_blocks=1, interctc_layer_idx=[1], interctc_use_conditioning=True)
    conf["model_conf"].update(interctc_weight=0.3, report_cer=True, report_wer=True)
    conf["token_list"] = TOKENS_EN
    model = ASRTask.build_model(argparse.Namespace(**conf))
    fill_parameters_(model, seed=51)
    return model.cuda().eval()


def _asr_batch(seed, B=3, Tin=120, L=9):
    from oracle.model import synth
    text = synth((B, L), seed=seed + 1, kind="int", lo=1, hi=40)
    tlens = torch.tensor([L, L - 3, 2][:B])
    text[torch.arange(L)[None, :] >= tlens[:, None]] = -1
    return dict(speech=synth((B, Tin, 80), seed=seed), speech_lengths=torch.tensor([Tin, Tin - 17, Tin - 40][:B]), text=text,
                text_lengths=tlens)


def test_asr_model_with_interctc_eval_forward_and_validation_switch_on_equals_off():
    from tavsr.train import validation
    model = _asr_model()
    batch = {k: v.cuda() for k, v in _asr_batch(60).items()}
    with torch.no_grad():
        (loss_on, on, _), (loss_off, off, _) = _both_routes(lambda: model(**{k: v.clone() for k, v in batch.items()}))
    assert {"cer_ctc", "cer_interctc_layer1", "cer", "wer"} <= on.keys() and torch.equal(loss_on, loss_off)
    _stats_equal(on, off)
    loader = [_asr_batch(70 + 10 * i) for i in range(3)]
    v_on, v_off = _both_routes(lambda: validation(model, loader, device="cuda"))
    assert v_on == v_off and all(isinstance(x, float) for x in v_on)


def test_avsr_model_eval_forward_switch_on_equals_off():
    from oracle.model import fill_parameters_, synth
    from tavsr.tasks.avsr import AVSRTask
    conf = avsr_conf(AVSR_YAML, num_blocks=2, dec_blocks=1)
    conf["model_conf"].update(report_cer=True, report_wer=True)
    conf["token_list"] = TOKENS_EN
    model = AVSRTask.build_model(argparse.Namespace(**conf))
    fill_parameters_(model, seed=52)
    model = model.cuda().eval()
    text = synth((2, 6), seed=83, kind="int", lo=1, hi=40)
    text[1, 4:] = -1
    batch = [synth((2, 64, 80), seed=81).cuda(), torch.tensor([64, 48]).cuda(), synth((2, 16, 88, 88), seed=82).cuda(),
             torch.tensor([16, 12]).cuda(), text.cuda(), torch.tensor([6, 4]).cuda()]
    with torch.no_grad():
        (loss_on, on, _), (loss_off, off, _) = _both_routes(lambda: model(*(t.clone() for t in batch)))
    assert {"cer_ctc", "cer", "wer"} <= on.keys() and torch.equal(loss_on, loss_off)
    _stats_equal(on, off)
