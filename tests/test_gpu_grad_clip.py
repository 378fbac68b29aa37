"""GPU: gradient clipping on the HIP path - the norm kernels against float64, non-finite values, torch's coefficient bit for
bit, the fused clipped Adam update against "scale, then the plain update", and ``FusedAdam.set_grad_clip`` end to end (espnet's
skip rule, the one-step-late settlement and its roll-back, live runs only, the schedulers, the two training loops).

Bounds.  The 2-norm is accumulated in double from exact squares: n adds of non-negative terms carry a relative error below
n * 2^-53 (< 2^-30 at the largest n here), the double square root and the rounding to fp32 add less than 2^-24 + 2^-52, so
2^-22 (two fp32 ulps of the reference) is met with room; the largest magnitude is a selection and must be exact.  Everything
that compares two runs of the same arithmetic is bit for bit."""
import math

import pytest
import torch

import grad_clip_ref as GR
from helpers import rel_err
from oracle.model import synth

pytestmark = pytest.mark.gpu

INF = math.inf
NORM_TYPES = [2.0, INF]


def _L():
    from tavsr import _lib
    return _lib


def _geometry():
    lib = _L().lib()
    return int(lib.tavsr_grad_norm_tile()), int(lib.tavsr_grad_norm_span())


def _norm(g, norm_type, max_norm=1.0, part0=1, counters=None):
    """the two launches on a flat fp32 tensor: (out = [norm, coef, non-finite], counters, partials); the slots in front of and
    behind the partials must come back untouched"""
    L = _L()
    lib, code, n = L.lib(), (2 if norm_type == 2.0 else 0), g.numel()
    k = lib.tavsr_grad_norm_nparts(n)
    parts = torch.full((part0 + k + 1,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((3,), -1.0, device="cuda")
    counters = torch.zeros(3, dtype=torch.int32, device="cuda") if counters is None else counters
    L.check(lib.tavsr_grad_norm_parts(g.data_ptr(), n, code, parts.data_ptr(), part0, L.stream()), "tavsr_grad_norm_parts")
    L.check(lib.tavsr_grad_clip_coef(parts.data_ptr() + 8 * part0, k, code, max_norm, out.data_ptr(), counters.data_ptr(),
                                     L.stream()), "tavsr_grad_clip_coef")
    torch.cuda.synchronize()
    assert float(parts[-1]) == -7.0 and all(float(x) == -7.0 for x in parts[:part0])
    return out, counters, parts[part0: part0 + k]


def _fp32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _adam(p, g, m, v, clip=None, wd=0.0, step=3, lr=1e-3):
    L = _L()
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, 0.9, 0.98, 1e-9, wd, step, 1.0)
    if clip is None:
        L.check(L.lib().tavsr_adamw_step(*args, L.stream()), "tavsr_adamw_step")
    else:
        L.check(L.lib().tavsr_adamw_step_clip(*args, clip.data_ptr(), L.stream()), "tavsr_adamw_step_clip")
    torch.cuda.synchronize()


def _state(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, device="cuda", generator=gen)
    m = torch.randn(n, device="cuda", generator=gen) * 0.1
    v = torch.rand(n, device="cuda", generator=gen) * 0.01
    return p, m, v


# ------------------------------------------------------------------------------------------------ 1. the norm
def _sizes():
    W, G = _geometry()
    return [1, 3, 4, 5, W - 1, W, W + 1, G - 1, G, G + 1, 2 * G + 3]


def test_partial_counts_follow_from_the_length_alone():
    lib = _L().lib()
    W, G = _geometry()
    assert W % 4 == 0 and G % W == 0 and G > W
    assert [lib.tavsr_grad_norm_nparts(n) for n in (0, 1, W, W + 3, W + 4, G, G + 4, 2 * G + 3, 40 * G)] == \
        [0, 1, 1, 1, 2, G // W, G // W, G // W, G // W]


@pytest.mark.parametrize("kind", ["randn", "huge", "zeros"])
@pytest.mark.parametrize("idx", range(11))
def test_norm_kernels_against_float64(idx, kind):
    n = _sizes()[idx]
    gen = torch.Generator(device="cuda").manual_seed(100 + idx)
    g = torch.zeros(n, device="cuda") if kind == "zeros" else torch.randn(n, device="cuda", generator=gen)
    if kind == "huge":                                              # squares overflow fp32, the norm does not
        g.mul_(1e-20).add_(1e20)
    v = g.double().cpu()
    ref = {2.0: math.sqrt(float((v * v).sum())), INF: float(v.abs().max())}
    for norm_type in NORM_TYPES:
        out, counters, parts = _norm(g, norm_type, max_norm=1.0)
        got = float(out[0])
        print(f"n={n} {kind} norm_type={norm_type}: got {got!r} ref {ref[norm_type]!r} rel {abs(got - ref[norm_type]) / max(ref[norm_type], 1e-300):.3e}")
        if norm_type == 2.0:
            assert abs(got - ref[2.0]) <= 2.0 ** -22 * ref[2.0]
        else:
            assert got == ref[INF]
        assert float(out[2]) == 0.0 and counters.tolist()[:2] == [1, 0]
        again, _, parts2 = _norm(g, norm_type, max_norm=1.0, part0=0)
        assert torch.equal(out, again) and torch.equal(parts, parts2)


@pytest.mark.parametrize("idx", [1, 3, 4, 6, 7, 10])
def test_norm_is_bit_equal_at_another_256_byte_offset(idx):
    n = _sizes()[idx]
    gen = torch.Generator(device="cuda").manual_seed(200 + idx)
    data = torch.randn(n, device="cuda", generator=gen)
    a = torch.empty(n + 64, device="cuda")[64:].copy_(data)
    b = torch.empty(n + 192, device="cuda")[192:].copy_(data)
    assert (a.data_ptr() - b.data_ptr()) % 256 == 0 and a.data_ptr() != b.data_ptr()
    for norm_type in NORM_TYPES:
        oa, _, pa = _norm(a, norm_type)
        ob, _, pb = _norm(b, norm_type)
        assert torch.equal(oa, ob) and torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------------ 2. non-finite values
@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("where", ["first", "tail", "boundary_lo", "boundary_hi"])
@pytest.mark.parametrize("bad", [math.nan, INF, -INF])
def test_one_non_finite_value_skips_the_update(bad, where, norm_type):
    W, _ = _geometry()
    n = 3 * W + 7                                                   # four workgroups, three floats in the scalar tail
    at = dict(first=0, tail=n - 1, boundary_lo=W - 1, boundary_hi=W)[where]
    assert _L().lib().tavsr_grad_norm_nparts(n) == 4 and n % 4 == 3
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    g[at] = bad
    out, counters, parts = _norm(g, norm_type, max_norm=1.0)
    norm, coef, flag = out.tolist()
    assert (math.isnan(norm) if math.isnan(bad) else norm == INF) and coef == 0.0 and flag == 1.0
    assert counters.tolist() == [1, 1, 0]
    p, m, v = _state(n, 8)
    before = [t.clone() for t in (p, m, v)]
    _adam(p, g, m, v, clip=out)
    for now, was in zip((p, m, v), before):
        assert torch.equal(now, was)
    assert bool(torch.isfinite(p).all())


# ------------------------------------------------------------------------------------------------ 3. the coefficient
def _torch_coef(norm32, max_norm):
    """clip_grad_norm_'s two lines on the returned fp32 norm (a CPU tensor: IEEE arithmetic)"""
    total_norm = torch.tensor([norm32], dtype=torch.float32)
    clip_coef = max_norm / (total_norm + 1e-6)
    return float(torch.clamp(clip_coef, max=1.0))


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_coefficient_is_torchs_bit_for_bit(norm_type):
    n = 1027
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    norm = float(_norm(g, norm_type)[0][0])
    counters = torch.zeros(3, dtype=torch.int32, device="cuda")
    below, above = _fp32(norm * 0.999), _fp32(norm * 1.001)
    bounds = (below, above, 0.5, 1.0, 5.0, _fp32(1e-3), 100.0, _fp32(norm / 3), _fp32(norm / 7))
    for max_norm in bounds:
        out, _, _ = _norm(g, norm_type, max_norm=max_norm, counters=counters)
        got_norm, coef, flag = out.tolist()
        assert got_norm == norm and flag == 0.0
        assert coef == _torch_coef(norm, max_norm), (max_norm, coef)
        assert (coef < 1.0) == (max_norm < norm)
    assert counters.tolist() == [len(bounds), 0, sum(b < norm for b in bounds)]
    # the norm just below max_norm: coef is exactly 1 and the clipped update IS the plain one
    out, _, _ = _norm(g, norm_type, max_norm=above)
    assert float(out[1]) == 1.0
    a, b = _state(n, 12), _state(n, 12)
    _adam(*a[:1], g, *a[1:], clip=out, wd=0.01)
    _adam(*b[:1], g, *b[1:], wd=0.01)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # no gradient at all: coef 1, nothing clipped
    out, c0, _ = _norm(torch.zeros(n, device="cuda"), norm_type, max_norm=_fp32(1e-3))
    assert out.tolist() == [0.0, 1.0, 0.0] and c0.tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ 4. the fused update
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [3, 4, 1027])
def test_clipped_update_equals_scaling_the_gradient_then_the_plain_update(n, wd):
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(20 + n)) * 3
    for norm_type in NORM_TYPES:
        out, _, _ = _norm(g, norm_type, max_norm=0.5)
        coef = out[1]
        assert 0.0 < float(coef) < 1.0
        a, b = _state(n, 21), _state(n, 21)
        for step in (1, 2, 7):
            _adam(a[0], g, a[1], a[2], clip=out, wd=wd, step=step)
            _adam(b[0], g * coef, b[1], b[2], wd=wd, step=step)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (norm_type, step)
        assert not torch.equal(a[0], _state(n, 21)[0])


# ------------------------------------------------------------------------------------------------ 5. FusedAdam end to end
SIZES = [5, 64, 65, 300]
SCALES = [0.01, 1.0, 0.01, 0.01, 1.0, 0.01]         # max_norm 1.0 binds at steps 2 and 5 (counting from 1), for both norm types
NAN_STEP = 2                                        # step 3 carries a NaN
KW = dict(betas=(0.9, 0.98), eps=1e-9)


def _grad_sets():
    sets = [[synth((s,), seed=800 + 10 * k + i) * sc for i, s in enumerate(SIZES)] for k, sc in enumerate(SCALES)]
    sets[NAN_STEP][2][17] = math.nan
    return sets


def _start():
    return [synth((s,), seed=750 + i) for i, s in enumerate(SIZES)]


def _noam_rate(count):
    return 1.6 * 256 ** (-0.5) * min(count ** (-0.5), count * 5 ** (-1.5))


def _make(noam, lr=3e-3):
    from tavsr.train import FusedAdam, NoamScheduler
    params = [torch.nn.Parameter(x.cuda()) for x in _start()]
    opt = NoamScheduler(256, 1.6, 5, FusedAdam(params, lr=0, **KW)) if noam else FusedAdam(params, lr=lr, **KW)
    return params, opt, (opt.optimizer if noam else opt)


def _drive(params, opt, sets):
    for gs in sets:
        for p, g in zip(params, gs):
            p.grad = None if g is None else g.cuda()
        opt.step()


@pytest.mark.parametrize("noam", [False, True], ids=["plain", "noam"])
@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_fused_adam_clips_skips_and_rolls_back_like_the_reference(norm_type, noam):
    sets = _grad_sets()
    lr = _noam_rate if noam else 3e-3
    want, log = GR.adam_clip_steps(_start(), sets, 1.0, norm_type, lr=lr, **KW)
    # the schedule of events, on the reference alone
    assert [e["clipped"] for e in log] == [False, True, False, False, True, False]
    assert [e["skipped"] for e in log] == [k == NAN_STEP for k in range(6)]
    assert log[5]["count"] == 5 and log[3]["count"] == 3 and (not noam or log[3]["lr"] == _noam_rate(3))
    params, opt, fused = _make(noam)
    opt.set_grad_clip(1.0, norm_type)
    rates = []
    for gs in sets:
        _drive(params, opt, [gs])
        rates.append(opt._rate if noam else None)
    stats = opt.clip_stats()
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (6, 1, 2)
    assert abs(stats["last_norm"] - log[5]["norm"]) <= 2.0 ** -22 * log[5]["norm"]
    assert fused._step == 5 and fused._steps == [5] * 4
    if noam:
        assert opt._step == 5 and rates[3] == _noam_rate(3) and rates == [e["lr"] for e in log]
    for i, (p, w) in enumerate(zip(params, want)):
        print(f"param {i}: rel_err {rel_err(p.detach().cpu(), w):.3e}")
        assert rel_err(p.detach().cpu(), w) < 2e-6, i
    # the sharpest test of the roll-back: an optimizer that never saw the NaN step ends on the same bits
    params2, opt2, fused2 = _make(noam)
    opt2.set_grad_clip(1.0, norm_type)
    _drive(params2, opt2, [gs for k, gs in enumerate(sets) if k != NAN_STEP])
    assert opt2.clip_stats()["skipped"] == 0
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(fused, name), getattr(fused2, name)), name
    assert fused2._step == 5 and (not noam or opt2._step == 5)


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_only_live_gradients_enter_the_norm(norm_type):
    params, opt, _ = _make(False)
    opt.set_grad_clip(1.0, norm_type)
    first = [synth((s,), seed=820 + i) * 0.01 for i, s in enumerate(SIZES)]
    first[1] = torch.full((SIZES[1],), 1e6)
    second = [synth((s,), seed=830 + i) * 0.01 for i, s in enumerate(SIZES)]
    second[1] = None
    _drive(params, opt, [first])
    assert opt.clip_stats()["last_norm"] >= 1e6
    lo, hi = opt.offsets[1], opt.offsets[2]
    before = [t[lo:hi].clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
    assert float(opt.grad[lo:hi].abs().max()) == 1e6              # the stale slot the norm must not read
    _drive(params, opt, [second])
    stats = opt.clip_stats()
    ref = GR.total_norm(second, norm_type)
    assert abs(stats["last_norm"] - ref) <= 2.0 ** -22 * ref and stats["clipped"] == 1 and stats["skipped"] == 0
    for now, was in zip((opt.flat, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(now[lo:hi], was)
    assert opt._steps == [2, 1, 2, 2]
    want, _ = GR.adam_clip_steps(_start(), [first, second], 1.0, norm_type, lr=3e-3, **KW)
    for i, (p, w) in enumerate(zip(params, want)):
        assert rel_err(p.detach().cpu(), w) < 2e-6, i


@pytest.mark.parametrize("noam", [False, True], ids=["plain", "noam"])
def test_a_skipped_last_step_is_settled_by_state_dict(noam):
    sets = _grad_sets()
    params, opt, fused = _make(noam)
    opt.set_grad_clip(1.0)
    _drive(params, opt, [sets[0], sets[1], sets[NAN_STEP]])
    assert fused._clip_pending is not None                          # nobody has asked yet
    sd = opt.state_dict()
    inner = sd["optimizer"] if noam else sd
    assert inner["step"] == 2 and inner["steps"] == [2] * 4 and (not noam or sd["_step"] == 2)
    assert fused._clip_pending is None and bool(torch.isfinite(fused.flat).all())
    opt.set_grad_clip(-1.0)                                         # and off again: the unclipped path, no stale verdict
    _drive(params, opt, [sets[3]])
    assert fused._step == 3 and fused.clip_stats()["steps"] == 3


class _Lin(torch.nn.Module):
    """loss = sum(w_i * x_i): the gradient is the batch, whatever the parameters are"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(x) for x in _start()])

    def forward(self, **x):
        return sum((w * x[f"x{i}"]).sum() for i, w in enumerate(self.w)), {}, torch.tensor(1)


def _batch(k, nan=False):
    gs = [synth((s,), seed=800 + 10 * k + i) * SCALES[k] for i, s in enumerate(SIZES)]
    if nan:
        gs[3][0] = math.nan
    return {f"x{i}": g for i, g in enumerate(gs)}


@pytest.mark.parametrize("nan_at", [1, 3])
def test_training_does_not_spend_a_one_cycle_position_on_a_nan_batch(nan_at):
    """the trainer moves scheduler.step() of step k behind the settlement of step k (tavsr.train._Stepper); nan_at 3: the
    skipped step is the last of the epoch"""
    from tavsr.train import FusedAdam, OneCycleLR, training
    runs = []
    for with_nan in (True, False):
        model = _Lin().cuda()
        opt = FusedAdam(model.parameters(), 5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        sch = OneCycleLR(opt, max_lr=5e-3, total_steps=10, anneal_strategy="linear")
        loader = [_batch(0), _batch(1), _batch(3)]
        if with_nan:
            loader.insert(nan_at, _batch(2, nan=True))
        training(model, loader, opt, sch, 1, grad_clip=1.0)
        assert opt._clip_pending is None
        runs.append((opt, sch))
    (oa, sa), (ob, sb) = runs
    assert sa.last_epoch == sb.last_epoch == 3 and oa.state_dict()["step"] == ob.state_dict()["step"] == 3
    assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"] and oa.param_groups[0]["betas"] == ob.param_groups[0]["betas"]
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name
    assert oa.clip_stats()["skipped"] == 1 and ob.clip_stats()["skipped"] == 0 and oa.clip_stats()["clipped"] == 1
    assert sa.get_last_lr() == sb.get_last_lr()


# ------------------------------------------------------------------------------------------------ 6. off is off
def test_without_clipping_the_steps_are_the_former_launches_bit_for_bit():
    from tavsr.train import FusedAdam
    sets = [[synth((s,), seed=800 + 10 * k + i) for i, s in enumerate(SIZES)] for k in range(6)]
    opts = []
    for mode in ("never", "minus_one", "on_then_off"):
        params = [torch.nn.Parameter(x.cuda()) for x in _start()]
        opt = FusedAdam(params, lr=3e-3, weight_decay=1e-2, **KW)
        if mode == "minus_one":
            opt.set_grad_clip(-1)
        elif mode == "on_then_off":
            opt.set_grad_clip(1.0, INF)
            opt.set_grad_clip(0.0)
        _drive(params, opt, sets)
        opts.append(opt)
    # the former driver: one tavsr_adamw_step over the whole flat buffer per step
    ref = FusedAdam([torch.nn.Parameter(x.cuda()) for x in _start()], lr=3e-3, weight_decay=1e-2, **KW)
    L = _L()
    for k, gs in enumerate(sets):
        for off, g in zip(ref.offsets, gs):
            ref.grad[off: off + g.numel()].copy_(g)
        L.check(L.lib().tavsr_adamw_step(ref.flat.data_ptr(), ref.grad.data_ptr(), ref.exp_avg.data_ptr(), ref.exp_avg_sq.data_ptr(),
                                         ref.flat.numel(), 3e-3, 0.9, 0.98, 1e-9, 1e-2, k + 1, 1.0, L.stream()), "tavsr_adamw_step")
    torch.cuda.synchronize()
    for opt in opts:
        for name in ("flat", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(opt, name), getattr(ref, name)), name
        assert opt.clip_stats()["steps"] == 0 and opt.clip_stats()["last_norm"] is None and opt._step == 6


# ------------------------------------------------------------------------------------------------ 7. the driver's loop
def test_lm_training_epoch_with_grad_clip_on_a_tiny_lm():
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.lm import ESPnetLanguageModel
    from tavsr.train import FusedAdam, lm_training
    V = 41
    torch.manual_seed(0)
    lm = ESPnetLanguageModel(TransformerLM(V, pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0),
                             V, ignore_id=-1).cuda()
    opt = FusedAdam(lm.parameters(), lr=1e-3, **KW)
    lens = (1, 31, 32, 70)
    loader = []
    for b in range(3):
        ids = synth((4, 80), seed=31 + b, kind="int", lo=1, hi=V - 1)[:, :70].contiguous()
        for r, l in enumerate(lens):
            ids[r, l:] = -1
        loader.append((ids, torch.tensor(lens, dtype=torch.int64), ["x"] * 4))
    before = opt.flat.clone()
    loss = lm_training(lm, loader, opt, None, 1, grad_clip=0.05)
    stats = opt.clip_stats()
    print(f"loss {loss:.4f} stats {stats}")
    assert math.isfinite(loss) and stats["steps"] == 3 and stats["clipped"] > 0 and stats["skipped"] == 0
    assert stats["last_norm"] > 0.05 and bool(torch.isfinite(opt.flat).all()) and not torch.equal(opt.flat, before)
