"""GPU: the device-side Mask-CTC mask draw - ``tavsr_mask_uniform`` against the CPU restatement ``tests/mask_draw_ref.py``
(bit-exact: integer outputs; the restatement's distribution is checked in test_mask_draw_host.py), the token contract of
``ops.mask_uniform``, and the training step with ``mask_draw = "device"``: eager against a step handed the regenerated pair,
reproducible under dropout, captured with new masks per replay, and length-normalised with the denominator on the device.

The models are the 3-block encoder / 2-block decoder audio-only one of test_gpu_maskctc.py's dropout tests (B = 8, 200 frames,
20 tokens) and the 2-block audio-visual one of its fixture test."""
import argparse
import copy
import functools

import numpy as np
import pytest
import torch

import mask_draw_ref as D
import maskctc_ref as R
from helpers import TOKENS_EN, avsr_conf, golden, rel_err
from oracle.model import fill_parameters_, synth

pytestmark = pytest.mark.gpu

MASK, EOS, IGN = 41, 40, -1


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _rows(lens, Lmax, seed=0, holes=()):
    """text [B, Lmax]: row b holds lens[b] tokens, trailing ignore_id; ``holes``: (row, column) pairs set to ignore_id afterwards"""
    rng = np.random.RandomState(seed)
    text = rng.randint(1, 40, size=(len(lens), Lmax)).astype(np.int64)
    for b, n in enumerate(lens):
        text[b, n:] = IGN
    for b, c in holes:
        text[b, c] = IGN
    return text


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device="cuda")


def _check_kernel(text, seed, offset):
    from tavsr import ops
    t = torch.from_numpy(text).cuda()
    ys_in, ys_out, n_target, tok = ops.mask_uniform(t, MASK, EOS, IGN, token=(offset, _seed_tensor(seed)))
    torch.cuda.synchronize()
    want = D.mask_uniform_dev_ref(text, MASK, EOS, IGN, seed, offset)
    assert ys_in.shape == ys_out.shape == t.shape and ys_in.dtype == ys_out.dtype == torch.int64 and n_target.dtype == torch.int32
    assert np.array_equal(ys_in.cpu().numpy(), want[0])
    assert np.array_equal(ys_out.cpu().numpy(), want[1])
    assert np.array_equal(n_target.cpu().numpy(), want[2])
    assert tok[0] == offset
    return want


CASES = {
    "one_token": (dict(lens=[1], Lmax=1), 0x5EED5EED, 0),
    "ragged_with_an_empty_row": (dict(lens=[20, 1, 7, 0, 13], Lmax=20), 0x5EED5EED, 0),
    "ignore_id_in_the_middle": (dict(lens=[9, 12, 12], Lmax=12, holes=((0, 0), (0, 4), (1, 5), (1, 6), (2, 11))), 77, 0),
    "past_one_block_width": (dict(lens=[300, 257], Lmax=300), 123456789, 0),
    "offset_not_zero": (dict(lens=[20, 1, 7, 0, 13], Lmax=20), 0x5EED5EED, 4 * 1234567),
    "offset_odd_and_beyond_32_bits": (dict(lens=[20, 1, 7, 0, 13], Lmax=20), -0x1234567890ABCDEF, (1 << 33) + 5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mask_uniform_kernel_equals_the_restatement(name):
    kw, seed, offset = CASES[name]
    text = _rows(**kw)
    ys_in, ys_out, n_target = _check_kernel(text, seed, offset)
    if name == "one_token":
        assert ys_in.tolist() == [[MASK]] and ys_out.tolist() == [[int(text[0, 0])]] and n_target.tolist() == [1]
    if name == "ragged_with_an_empty_row":
        assert n_target[3] == 0 and (ys_in[3] == EOS).all() and (ys_out[3] == IGN).all()


def test_mask_uniform_kernel_at_its_limit_and_one_beyond():
    from tavsr import _lib, ops
    lim = _lib.ENUMS["TAVSR_MASK_UNIFORM_MAX_L"]
    assert lim >= 2048
    _check_kernel(_rows([lim, lim // 2 + 1], lim, seed=3), 99, 8)
    text = torch.from_numpy(_rows([lim + 1], lim + 1)).cuda()
    with pytest.raises(_lib.TavsrError, match="limit"):
        ops.mask_uniform(text, MASK, EOS, IGN)
    # nothing is launched: the outputs keep what they held
    ys_in, ys_out = torch.full_like(text, 7), torch.full_like(text, 7)
    n_target = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().tavsr_mask_uniform(_lib.ptr(text), lim + 1, 1, lim + 1, MASK, EOS, IGN, _lib.ptr(_seed_tensor(1)), 0,
                                       _lib.ptr(ys_in), _lib.ptr(ys_out), lim + 1, _lib.ptr(n_target), _lib.stream())
    torch.cuda.synchronize()
    assert rc == _lib.ENUMS["TAVSR_EUNSUPPORTED"]
    assert (ys_in == 7).all() and (ys_out == 7).all() and (n_target == 7).all()


def test_token_regenerates_the_draw_and_a_new_pass_draws_anew():
    from tavsr import ops
    text = torch.from_numpy(_rows([20, 1, 7, 0, 13, 20, 20, 18], 20)).cuda()
    ops.manual_seed(5)
    ops.rng_step_begin()
    a = ops.mask_uniform(text, MASK, EOS, IGN)
    b = ops.mask_uniform(text, MASK, EOS, IGN)                    # the next site of the same pass: its own counter range
    assert a[3][0] == 0 and b[3][0] == 8 * D.counters_per_row(20) and b[3][1] is a[3][1]
    ops.rng_step_begin()
    c = ops.mask_uniform(text, MASK, EOS, IGN)
    again = ops.mask_uniform(text, MASK, EOS, IGN, token=a[3])
    for x, y in zip(a[:3], again[:3]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[0], c[0])
    seed = int(a[3][1].cpu()[0])
    want = D.mask_uniform_dev_ref(text.cpu().numpy(), MASK, EOS, IGN, seed, 0)
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[2].cpu().numpy(), want[2])


def test_count_recip():
    from tavsr import ops
    for n in ([0, 0, 0], [3], list(range(200)), [1, 0, 2, 4]):
        got = float(ops.count_recip(torch.tensor(n, dtype=torch.int32, device="cuda"))[0])
        assert got == float(np.float32(1.0) / np.float32(max(1, sum(n)))), n


# ------------------------------------------------------------------------------------------------ 2. the training step
def _build(conf, seed, task="asr"):
    from tavsr.tasks.asr import ASRTask
    from tavsr.tasks.avsr import AVSRTask
    conf = copy.deepcopy(conf)
    conf["token_list"] = list(TOKENS_EN)
    m = (AVSRTask if task == "avsr" else ASRTask).build_model(argparse.Namespace(**conf))
    fill_parameters_(m, seed=seed)
    return m.cuda().train()


@functools.lru_cache(maxsize=None)
def _asr(dropout):
    model = _build(R.asr_maskctc_conf(num_blocks=3, dec_blocks=2, dropout=dropout), 3)
    B = 8
    speech = synth((B, 200, 80), seed=6).cuda()
    slens = torch.tensor([200 - 8 * i for i in range(B)]).cuda()
    text = synth((B, 20), seed=7, kind="int", lo=1, hi=40)
    tlens = torch.tensor([20 - 2 * (i % 5) for i in range(B)])
    tlens[0] = 20
    for i, n in enumerate(tlens):
        text[i, int(n):] = -1
    return model, (speech, slens, text.cuda(), tlens.cuda())


def _set_dropout(d, p):
    for k, v in d.items():
        if isinstance(v, dict):
            _set_dropout(v, p)
        elif k.endswith("dropout_rate"):
            d[k] = p


@functools.lru_cache(maxsize=None)
def _avsr():
    g = golden("maskctc_avsr_2L")
    conf = avsr_conf(R.AVSR_MASKCTC_YAML, num_blocks=2, dec_blocks=1)
    _set_dropout(conf, 0.1)
    model = _build(conf, 101, task="avsr")
    B, Ta, Tv = int(g["B"]), int(g["Ta"]), int(g["Tv"])
    return model, (synth((B, Ta, 80), seed=102).cuda(), torch.from_numpy(g["alens"]).cuda(), synth((B, Tv, 88, 88), seed=103).cuda(),
                   torch.from_numpy(g["vlens"]).cuda(), torch.from_numpy(g["text"]).cuda(), torch.from_numpy(g["tlens"]).cuda())


def _step(model, batch, seed=11, **masks):
    from tavsr import ops
    for p in model.parameters():
        p.grad = None
    ops.manual_seed(seed)
    loss = model(*batch, **masks)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), [p.grad.clone() for p in model.parameters()]


def _assert_bit_equal(model, a, b):
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]), (a[0], b[0])
    for (n, _), x, y in zip(model.named_parameters(), a[1], b[1]):
        assert torch.equal(x, y), n


def _regenerated_pair(model, text):
    from tavsr import ops
    ys_in, ys_out, n_target, _ = ops.mask_uniform(text, model.mask_token, model.eos, model.ignore_id, token=model.last_mask_token)
    assert int(n_target.sum()) == int((ys_out != model.ignore_id).sum()) > 0
    return dict(ys_in_pad=ys_in, ys_out_pad=ys_out)


def test_device_draw_step_equals_the_step_handed_its_masks():
    model, batch = _asr(0.0)
    model.mask_draw, model.length_normalized_loss = "device", False
    got = _step(model, batch)
    pair = _regenerated_pair(model, batch[2])
    assert (pair["ys_in_pad"] == model.mask_token).any()
    model.mask_draw = "host"
    _assert_bit_equal(model, got, _step(model, batch, **pair))
    model.mask_draw = "device"                          # caller-supplied masks still win
    _assert_bit_equal(model, got, _step(model, batch, seed=12, **pair))
    other = _step(model, batch, seed=12)                # (no dropout: only the masks depend on the seed)
    assert not torch.equal(got[0], other[0])


def test_device_draw_step_with_dropout_is_bitwise_reproducible():
    model, batch = _asr(0.1)
    model.mask_draw, model.length_normalized_loss = "device", False
    a, b, c = _step(model, batch), _step(model, batch), _step(model, batch, seed=12)
    _assert_bit_equal(model, a, b)
    assert not torch.equal(a[0], c[0])


def test_device_draw_step_of_the_av_model_is_bitwise_reproducible():
    model, batch = _avsr()
    model.mask_draw = "device"
    a, b, c = _step(model, batch), _step(model, batch), _step(model, batch, seed=12)
    _assert_bit_equal(model, a, b)
    assert not torch.equal(a[0], c[0])
    assert model.last_mask_token is not None


def _capture(model, batch):
    from tavsr import ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(model, batch)
    torch.cuda.current_stream().wait_stream(side)
    for p in model.parameters():
        p.grad = None
    ops.manual_seed(11)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = model(*batch)[0]
        loss.backward()
    return graph, loss


def _replays_equal_eager(model, batch, ref):
    from tavsr import ops
    graph, loss = _capture(model, batch)
    for rep in range(2):
        ops.manual_seed(11)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), ref[0]), rep
        for (n, p), want in zip(model.named_parameters(), ref[1]):
            assert torch.equal(p.grad, want), (rep, n)
    graph.replay()                                      # no reseeding: the generator moved on, the masks are new
    torch.cuda.synchronize()
    second = loss.detach().clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(second).all() and not torch.equal(second, ref[0]) and not torch.equal(loss.detach(), second)


def test_captured_device_draw_step_equals_eager_and_draws_new_masks_per_replay():
    model, batch = _asr(0.1)
    model.mask_draw, model.length_normalized_loss = "device", False
    _replays_equal_eager(model, batch, _step(model, batch))


def test_length_normalised_loss_with_the_denominator_on_the_device():
    model, batch = _asr(0.0)
    try:
        model.mask_draw, model.length_normalized_loss = "device", True
        got = _step(model, batch)
        pair = _regenerated_pair(model, batch[2])
        model.mask_draw = "host"
        want = _step(model, batch, **pair)              # the host count of LabelSmoothingLossFn
        model.length_normalized_loss = False
        plain = _step(model, batch, **pair)
        assert not torch.equal(plain[0], want[0])       # (the normalisation does something)
        err = rel_err(got[0], want[0])
        print("loss", float(got[0]), float(want[0]), "rel", err)
        assert err < 1e-6
        worst = 0.0
        for (n, _), x, y in zip(model.named_parameters(), got[1], want[1]):
            if float(y.norm()) == 0.0:
                assert float(x.norm()) == 0.0, n
                continue
            worst = max(worst, rel_err(x, y))
            assert rel_err(x, y) < 1e-5, (n, rel_err(x, y))
        print("worst gradient rel-L2", worst)
        model.mask_draw, model.length_normalized_loss = "device", True
        _replays_equal_eager(model, batch, got)
    finally:
        model.length_normalized_loss = False
