"""GPU: language-model training on the HIP path - ``tavsr_lm_shift`` against the plain-Python rows, ``TransformerLMFn``
(forward, every parameter gradient) and ``ESPnetLanguageModel`` (``nll`` / ``batchify_nll`` / ``forward``) against the fp64
restatement ``tests/lm_ref.py``, the untouched scoring route, the captured step, ten optimizer steps and dropout.

Shapes: V = 41, four sentences of 1 / 31 / 32 / 70 tokens, so the input rows are 2 / 32 / 33 / 71 long - on both sides of the
attention kernels' 32-row query tile and of the 64-key boundary, 284 rows in all (a tail in every GEMM tile), one sentence of a
single token.  Three models: A (dk = 64: the fused attention core), B (dk = 16: the unfused one; ``LM_KW`` of the search tests)
and C (the recipe's widths D = 512, H = 8, K = 2048 at two layers).

Bars: 1e-4 relative L2 against fp64, the bar of tests/test_gpu_parity.py (the fp32 oracle on the CPU is within 1.2e-6 of the
fp64 one on every gradient here and within 1e-7 on the loss and the nll rows).  ``linear_k.bias`` has a gradient of exactly zero
(softmax does not see a per-query constant; 1e-18 in fp64), so its norm is held against the same layer's ``linear_q.bias``."""
import functools

import numpy as np
import pytest
import torch

import lm_ref as R
from helpers import rel_err
from oracle.beam_search import TransformerLMOracle
from oracle.model import fill_parameters_, synth

pytestmark = pytest.mark.gpu

V, SOS = 41, 40
LENS = (1, 31, 32, 70)
MODELS = {
    "A": dict(pos_enc=None, embed_unit=32, att_unit=128, head=2, unit=256, layer=2, dropout_rate=0.0),
    "B": dict(pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0),
    "C": dict(pos_enc=None, embed_unit=128, att_unit=512, head=8, unit=2048, layer=2, dropout_rate=0.0),
}
BAR = 1e-4


def _text(width, pad, lens=LENS, seed=31):
    """ids 1 .. V - 2 (no <blank>, no <sos/eos>); the same ids whatever the width and the pad value"""
    ids = synth((len(lens), max(80, width)), seed=seed, kind="int", lo=1, hi=V - 1)[:, :width].contiguous()
    for b, l in enumerate(lens):
        ids[b, l:] = pad
    return ids, torch.tensor(lens, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 oracle of model ``name`` on the fixed batch: (fp32 state dict, nll, x_lengths, loss, weight, gradients)"""
    ref = R.LMRef(TransformerLMOracle(V, **MODELS[name]), V).train()
    fill_parameters_(ref, seed=40 + ord(name))
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.double()
    text, lens = _text(70, -1)
    loss, _, weight = ref(text, lens)
    loss.backward()
    with torch.no_grad():
        nll, xl = ref.nll(text, lens)
    return state, nll, xl, loss.detach(), int(weight), {k: p.grad.clone() for k, p in ref.named_parameters()}


def _product(name, dropout=None):
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.lm import ESPnetLanguageModel
    kw = dict(MODELS[name])
    if dropout is not None:
        kw["dropout_rate"] = dropout
    m = ESPnetLanguageModel(TransformerLM(V, **kw), V, ignore_id=-1)
    m.load_state_dict(_reference(name)[0])
    return m.cuda().train()


def _step(m, text, lens):
    for p in m.parameters():
        p.grad = None
    loss, stats, weight = m(text.cuda(), lens.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), weight, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------ 1. the rows
@pytest.mark.parametrize("width", [70, 80])
def test_lm_shift_kernel_equals_the_python_rows_whatever_the_pad_value(width):
    from tavsr import ops
    want = R.lm_shift(*[t.tolist() for t in _text(width, -1)], SOS)
    assert want[0].shape == (4, width + 1)
    for pad in (-1, 0, 7):
        text, lens = _text(width, pad)
        got = ops.lm_shift(text.cuda(), lens.cuda(), SOS)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (pad, width)
    wide = R.lm_shift(*[t.tolist() for t in _text(width, -1)], SOS, width=width + 6)       # nll(max_length = width + 5)
    got = ops.lm_shift(*[t.cuda() for t in _text(width, 7)], SOS, width=width + 6)
    for g, w in zip(got, wide):
        assert torch.equal(g.cpu(), w)


def test_lm_shift_kernel_single_sentence_and_empty_sentence():
    from tavsr import ops
    for lens in ((70,), (0,), (3,)):
        text, l = _text(70, -1, lens=lens)
        want = R.lm_shift(text.tolist(), l.tolist(), SOS)
        got = ops.lm_shift(text.cuda(), l.cuda(), SOS)
        for g, w in zip(got, want):
            assert torch.equal(g.cpu(), w), lens
    text, l = _text(70, -1)                                             # a strided view of a wider batch: ld_text > W
    got = ops.lm_shift(text.cuda()[:, :40], torch.tensor([1, 31, 32, 40]).cuda(), SOS)
    want = R.lm_shift(text[:, :40].tolist(), [1, 31, 32, 40], SOS)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)


def test_row_sums_kernel_is_the_per_sentence_sum():
    from tavsr import ops
    x = synth((7, 71), seed=3).cuda()
    got = ops.row_sums(x)
    assert rel_err(got.cpu(), x.double().sum(1).cpu()) < 1e-6 and torch.equal(got, ops.row_sums(x))
    assert rel_err(ops.row_sums(x[:, :33]).cpu(), x[:, :33].double().sum(1).cpu()) < 1e-6


# ------------------------------------------------------------------------------------------------ 2. loss, nll, gradients
def _check_against_reference(name, got, where):
    _, _, _, loss_w, weight_w, grads_w = _reference(name)
    loss, weight, grads = got
    print(f"{name} {where}: loss {float(loss):.7f} (fp64 {float(loss_w):.7f})")
    assert abs(float(loss) - float(loss_w)) / abs(float(loss_w)) < BAR, where
    assert int(weight) == weight_w == sum(LENS) + len(LENS), where
    assert set(grads) == set(grads_w)
    worst = ("", 0.0)
    for k, g in grads.items():
        assert torch.isfinite(g).all(), (where, k)
        if k.endswith("linear_k.bias"):
            q = grads[k.replace("linear_k", "linear_q")]
            print(f"{name} {where}: |d {k}| = {float(g.norm()):.3e}, |d linear_q.bias| = {float(q.norm()):.3e}")
            assert float(g.norm()) <= BAR * float(q.norm()), (where, k)
            continue
        e = rel_err(g.cpu(), grads_w[k])
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < BAR, (where, k, e)
    print(f"{name} {where}: worst gradient {worst[0]} rel {worst[1]:.3e}")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_training_step_matches_the_fp64_reference(name):
    """loss, weight, nll rows, x_lengths and every parameter gradient at ``BAR`` for text padded with -1 and with 0 at width 70
    and at width 80 (ten all-padding columns); bit-equal between the two pad values."""
    from tavsr import ops
    _, nll_w, xl_w, _, _, _ = _reference(name)
    m = _product(name)
    out = {}
    for width in (70, 80):
        for pad in (-1, 0):
            text, lens = _text(width, pad)
            out[width, pad] = step = _step(m, text, lens)
            _check_against_reference(name, step, f"width {width} pad {pad}")
            nll, xl = m.nll(text.cuda(), lens.cuda())
            assert nll.shape == (4, width + 1) and torch.equal(xl.cpu(), xl_w)
            e = rel_err(nll[:, :71].cpu(), nll_w)
            print(f"{name} width {width} pad {pad}: nll rel {e:.3e}")
            assert e < BAR and float(nll[:, 71:].abs().sum()) == 0.0
            for b, l in enumerate(LENS):
                assert float(nll[b, l + 1:].abs().sum()) == 0.0 and bool((nll[b, : l + 1] > 0).all())
            out[width, pad] += (nll.clone(),)
        a, b = out[width, -1], out[width, 0]
        assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), (width, k)
    sums = ops.row_sums(out[70, -1][3])
    assert rel_err(sums.cpu(), nll_w.sum(1)) < BAR


def test_nll_max_length_pads_and_cuts_the_rows():
    m = _product("B")
    text, lens = _text(70, -1)
    base, _ = m.nll(text.cuda(), lens.cuda())
    wide, xl = m.nll(text.cuda(), lens.cuda(), max_length=75)
    assert wide.shape == (4, 76) and torch.equal(xl.cpu(), lens + 1) and float(wide[:, 71:].abs().sum()) == 0.0
    assert rel_err(wide[:, :71].cpu(), base.cpu()) < 1e-6
    cut, xl = m.nll(text.cuda()[:3], lens.cuda()[:3], max_length=32)
    assert cut.shape == (3, 33) and torch.equal(xl.cpu(), lens[:3] + 1) and rel_err(cut.cpu(), base[:3, :33].cpu()) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. the scoring route
def test_eval_route_is_the_former_forward_bit_for_bit():
    m = _product("B").lm.eval()
    x = synth((3, 33), seed=5, kind="int", lo=1, hi=V).cuda()
    with torch.no_grad():
        a, b = m(x)[0], m._score_forward(x)[0]
    assert torch.equal(a, b) and not a.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    c = m(x)[0]                                    # nothing to differentiate: the scoring pass, autograd on or off
    assert torch.equal(a, c) and not c.requires_grad
    for p in m.parameters():
        p.requires_grad_(True)
    d = m(x)[0]                                    # autograd records: the training function, same values within rounding
    assert d.requires_grad and rel_err(d.detach().cpu(), a.cpu()) < 1e-5


# ------------------------------------------------------------------------------------------------ 4. batchify_nll
def test_batchify_nll_in_slices_equals_one_call():
    m = _product("B")
    lens7 = (1, 31, 32, 70, 5, 64, 33)
    text, lens = _text(70, -1, lens=lens7, seed=37)
    one, xl1 = m.nll(text.cuda(), lens.cuda())
    got, xl = m.batchify_nll(text.cuda(), lens.cuda(), batch_size=3)
    assert got.shape == one.shape == (7, 71) and torch.equal(xl, xl1) and xl.cpu().tolist() == [l + 1 for l in lens7]
    e = rel_err(got.cpu(), one.cpu())
    print(f"batchify_nll vs one call: rel {e:.3e}")
    assert e < BAR
    ref = R.LMRef(TransformerLMOracle(V, **MODELS["B"]), V)
    ref.load_state_dict(_reference("B")[0])
    with torch.no_grad():
        want, xlw = ref.double().eval().batchify_nll(text, lens, batch_size=3)
    assert torch.equal(xl.cpu(), xlw) and rel_err(got.cpu(), want) < BAR
    whole, _ = m.batchify_nll(text.cuda(), lens.cuda(), batch_size=100)
    assert torch.equal(whole, one)


# ------------------------------------------------------------------------------------------------ 5. the captured step
def test_training_step_captured_replays_other_batches_bit_equal_to_eager():
    m = _product("B")
    text_a, lens_a = _text(70, -1)
    text_b, lens_b = _text(70, 0, lens=(70, 2, 33, 17), seed=77)
    want_b, want_a = _step(m, text_b, lens_b), _step(m, text_a, lens_a)
    text_s, lens_s = text_a.cuda(), lens_a.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(m, text_a, lens_a)
    torch.cuda.current_stream().wait_stream(side)
    for p in m.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = m(text_s, lens_s)[0]
        loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}       # the graph's own gradient tensors: every replay rewrites them
    for rep, (text, lens, ref) in enumerate(((text_b, lens_b, want_b), (text_a, lens_a, want_a), (text_b, lens_b, want_b))):
        text_s.copy_(text.cuda())
        lens_s.copy_(lens.cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), ref[0]), rep
        for k in grads:
            assert torch.equal(grads[k], ref[2][k]), (rep, k)


# ------------------------------------------------------------------------------------------------ 6. ten optimizer steps
def test_ten_fused_adam_steps_follow_adam_on_the_fp64_reference():
    from tavsr.train import FusedAdam
    ref = R.LMRef(TransformerLMOracle(V, **MODELS["B"]), V).train()
    ref.load_state_dict(_reference("B")[0])
    ref = ref.double()
    m = _product("B")
    text, lens = _text(70, -1)
    kw = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    opt_r, opt = torch.optim.Adam(ref.parameters(), **kw), FusedAdam(m.parameters(), **kw)
    losses = []
    for it in range(10):
        opt_r.zero_grad()
        lr_ = ref(text, lens)[0]
        lr_.backward()
        opt_r.step()
        opt.zero_grad()
        lg = m(text.cuda(), lens.cuda())[0]
        lg.backward()
        opt.step()
        losses.append((float(lg.detach()), float(lr_.detach())))
        print(f"step {it}: loss {losses[-1][0]:.6f} (fp64 {losses[-1][1]:.6f})")
        assert abs(losses[-1][0] - losses[-1][1]) / abs(losses[-1][1]) < BAR, it
    assert losses[-1][0] < losses[0][0]


# ------------------------------------------------------------------------------------------------ 7. dropout
def test_dropout_step_runs_is_reproducible_and_its_backward_matches_central_differences():
    """espnet's constructor default, dropout 0.5: the method of test_gpu_dropout.py (d loss / d theta along the gradient by
    central differences under masks frozen by re-seeding, 3 %), the same seed gives the same bits, and the masks do something."""
    from tavsr import ops
    m = _product("B", dropout=0.5)
    text, lens = (t.cuda() for t in _text(70, -1))

    def loss_at():
        ops.manual_seed(2024)
        return m(text, lens)[0]

    def step():
        for p in m.parameters():
            p.grad = None
        loss = loss_at()
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    l0 = _step(_product("B"), text, lens)[0]
    assert np.isfinite(float(l1)) and abs(float(l1) - float(l0)) > 1e-3 * abs(float(l0))
    ops.manual_seed(2025)
    assert float(m(text, lens)[0].detach()) != float(l1)                     # another seed, other masks
    params = list(m.parameters())
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1)))
    assert np.isfinite(gnorm) and gnorm > 0
    eps = 2e-3 / gnorm * float(torch.sqrt(sum((p.double() ** 2).sum() for p in params)))   # ~0.2 % relative step
    with torch.no_grad():
        for p, g in zip(params, g1):
            p.add_(g, alpha=eps / gnorm)
        lp = float(loss_at())
        for p, g in zip(params, g1):
            p.add_(g, alpha=-2 * eps / gnorm)
        lm_ = float(loss_at())
    fd = (lp - lm_) / (2 * eps)
    print(f"dropout 0.5: loss {float(l1):.6f} (no dropout {float(l0):.6f}), directional derivative {fd:.6f} vs |g| {gnorm:.6f}")
    assert abs(fd - gnorm) / gnorm < 3e-2, (fd, gnorm)
