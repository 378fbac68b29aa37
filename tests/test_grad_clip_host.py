"""Host side of ``grad_clip``: the float64 restatement (tests/grad_clip_ref.py) against torch's own clip_grad_norm_ + Adam, the two
training loops of ``tavsr.train`` with a torch optimizer (the fallback every non-fused optimizer takes), the LM driver's keys,
the refusals and the C ABI's declarations.  No GPU."""
import math
import os
import re
import warnings

import pytest
import torch
import yaml

import grad_clip_ref as GR
from helpers import ROOT
from oracle.model import synth

INF = math.inf
SHAPES = [(7, 5), (33,), (2, 3, 4)]
# per-step gradient scale: the 2-norm of a synth() gradient set of SHAPES is ~10 and its largest magnitude 2 - 3.4 at scale 1, so
# with max_norm 1.0 the steps at scale 1 (2 and 5, counting from 1) clip and those at 0.01 do not, for both norm types
SCALES = [0.01, 1.0, 0.01, 0.01, 1.0, 0.01]
CLIPS = [False, True, False, False, True, False]


def _grads(step, scale, shapes=SHAPES):
    return [synth(s, seed=700 + 10 * step + i) * scale for i, s in enumerate(shapes)]


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_restatement_equals_torch_clip_grad_norm_and_adam_in_float64(norm_type):
    start = [synth(s, seed=650 + i).double() for i, s in enumerate(SHAPES)]
    steps = [_grads(k, sc) for k, sc in enumerate(SCALES)]
    kw = dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-9)
    got, log = GR.adam_clip_steps(start, steps, 1.0, norm_type, **kw)
    assert [e["clipped"] for e in log] == CLIPS and not any(e["skipped"] for e in log)      # the schedule, on the reference alone
    assert [e["count"] for e in log] == [1, 2, 3, 4, 5, 6]
    params = [torch.nn.Parameter(x.clone()) for x in start]
    opt = torch.optim.Adam(params, **kw)
    for k, gs in enumerate(steps):
        for p, g in zip(params, gs):
            p.grad = g.double().clone()
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0, norm_type=norm_type)
        assert float(norm) == pytest.approx(log[k]["norm"], rel=1e-13)
        assert float(norm) == pytest.approx(GR.total_norm(gs, norm_type), rel=1e-13)
        opt.step()
    for a, b in zip(got, params):
        assert torch.allclose(a, b.detach(), rtol=1e-12, atol=1e-14)


def test_restatement_skips_non_finite_steps_and_counts_taken_steps_only():
    start = [synth(s, seed=650 + i) for i, s in enumerate(SHAPES)]
    steps = [_grads(k, 0.01) for k in range(4)]
    steps[1][2][0, 1, 2] = math.nan
    steps[2][0][3, 3] = -INF
    rates = []
    got, log = GR.adam_clip_steps(start, steps, 1.0, 2.0, lr=lambda count: rates.append(count) or 1e-3 * count)
    assert [e["skipped"] for e in log] == [False, True, True, False] and [e["count"] for e in log] == [1, 1, 1, 2]
    assert math.isnan(log[1]["norm"]) and log[2]["norm"] == INF and rates == [1, 2, 2, 2]
    want, _ = GR.adam_clip_steps(start, [steps[0], steps[3]], 1.0, 2.0, lr=lambda count: 1e-3 * count)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert GR.clip_coef(0.0, 5.0) == 1.0 and GR.clip_coef(10.0, 5.0) == 5.0 / (10.0 + 1e-6)
    assert math.isnan(GR.total_norm([torch.tensor([1.0, math.nan])], INF)) and GR.total_norm([None, torch.tensor([-3.0, 2.0])], INF) == 3.0


# ------------------------------------------------------------------------------------------------ the loops
class _Lin(torch.nn.Module):
    """forward(**batch) -> (loss, stats, weight) with loss = sum(w_i * x_i): the gradient is the batch itself, whatever the
    parameters are, so the float64 loop can be fed the same gradients"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(synth(s, seed=650 + i)) for i, s in enumerate(SHAPES)])

    def forward(self, **x):
        loss = sum((w * x[f"x{i}"]).sum() for i, w in enumerate(self.w))
        return loss, {}, torch.tensor(1)


class _LinLM(_Lin):
    """the same as a language model: forward(xs, ilens); xs[b, 0] picks the step's gradient set, a negative one gives NaN"""

    def forward(self, xs, ilens):
        k = int(xs[0, 0])
        if k < 0:
            return super().forward(**_batch(0, math.nan))
        return super().forward(**_batch(k, SCALES[k]))


def _batch(k, scale):
    return {f"x{i}": g for i, g in enumerate(_grads(k, scale))}


def _one_cycle(opt, total):
    return torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-3, total_steps=total, anneal_strategy="linear", cycle_momentum=False)


def _schedule(total):
    """the learning rate torch's OneCycleLR sets for the count-th optimizer step (count from 1)"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=5e-3)
    sch = _one_cycle(opt, total)
    rates = []
    for _ in range(total):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return lambda count: rates[count - 1]


ADAM = dict(betas=(0.9, 0.98), eps=1e-9)


def _state(model, opt, sch):
    st = opt.state_dict()["state"]
    return ([p.detach().clone() for p in model.parameters()],
            {k: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in s.items()} for k, s in st.items()}, sch.last_epoch,
            opt.param_groups[0]["lr"])


def _same_state(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[2] == b[2] and a[3] == b[3] and a[1].keys() == b[1].keys()
    for k in a[1]:
        for n, t in a[1][k].items():
            assert torch.equal(t, b[1][k][n]) if torch.is_tensor(t) else t == b[1][k][n], (k, n)


def test_training_with_a_torch_optimizer_clips_and_skips_like_the_reference_loop():
    from tavsr.train import training
    nan_at = 3
    loader = [_batch(k, sc) for k, sc in enumerate(SCALES)]
    loader.insert(nan_at, _batch(0, math.nan))
    steps = [list(b.values()) for b in loader]
    want, log = GR.adam_clip_steps(_Lin().w, steps, 1.0, 2.0, lr=_schedule(10), **ADAM)
    assert [e["skipped"] for e in log] == [k == nan_at for k in range(7)]
    assert [e["clipped"] for e in log] == CLIPS[:nan_at] + [False] + CLIPS[nan_at:]
    model = _Lin()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3, **ADAM)
    sch = _one_cycle(opt, 10)
    with pytest.warns(UserWarning, match="1 of 7 optimizer steps"):
        loss = training(model, loader, opt, sch, 1, device="cpu", grad_clip=1.0)
    assert math.isnan(loss)                             # the NaN batch is part of the epoch's loss, as in espnet
    for a, b in zip(model.parameters(), want):
        assert torch.allclose(a.detach().double(), b, rtol=1e-6, atol=1e-7)
    assert sch.last_epoch == 6 and opt.param_groups[0]["lr"] == _schedule(10)(7)
    # the NaN batch alone: parameters, moments, step counts and the schedule's position stay as they are
    before = _state(model, opt, sch)
    with pytest.warns(UserWarning, match="1 of 1 optimizer steps"):
        training(model, [_batch(0, math.nan)], opt, sch, 1, device="cpu", grad_clip=1.0, grad_clip_type=INF)
    _same_state(before, _state(model, opt, sch))
    # gradient accumulation: the clip sees the window's accumulated gradient
    model2 = _Lin()
    opt2 = torch.optim.Adam(model2.parameters(), lr=5e-3, **ADAM)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        training(model2, loader[:3], opt2, None, 2, device="cpu", grad_clip=1.0, grad_clip_type=INF)
    acc = [[(a + b) / 2 for a, b in zip(steps[0], steps[1])], [g / 2 for g in steps[2]]]
    want2, log2 = GR.adam_clip_steps(_Lin().w, acc, 1.0, INF, lr=5e-3, **ADAM)
    assert [e["clipped"] for e in log2] == [True, False]
    for a, b in zip(model2.parameters(), want2):
        assert torch.allclose(a.detach().double(), b, rtol=1e-6, atol=1e-7)


def test_lm_training_with_a_torch_optimizer_clips_and_skips_like_the_reference_loop():
    from tavsr.train import lm_training
    order = [0, 1, -1, 2, 3, 4, 5]
    loader = [(torch.full((1, 2), k, dtype=torch.int64), torch.tensor([2]), ["x"]) for k in order]
    steps = [_grads(0, math.nan) if k < 0 else _grads(k, SCALES[k]) for k in order]
    want, log = GR.adam_clip_steps(_Lin().w, steps, 1.0, INF, lr=_schedule(10), **ADAM)
    assert [e["skipped"] for e in log] == [k < 0 for k in order] and sum(e["clipped"] for e in log) == 2
    model = _LinLM()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3, **ADAM)
    sch = _one_cycle(opt, 10)
    with pytest.warns(UserWarning, match="1 of 7 optimizer steps"):
        lm_training(model, loader, opt, sch, 1, device="cpu", grad_clip=1.0, grad_clip_type=INF)
    for a, b in zip(model.parameters(), want):
        assert torch.allclose(a.detach().double(), b, rtol=1e-6, atol=1e-7)
    assert sch.last_epoch == 6
    before = _state(model, opt, sch)
    with pytest.warns(UserWarning):
        lm_training(model, loader[2:3], opt, sch, 1, device="cpu", grad_clip=1.0)
    _same_state(before, _state(model, opt, sch))


@pytest.mark.parametrize("loop", ["training", "lm_training"])
def test_grad_clip_off_is_bit_equal_to_not_passing_it(loop):
    from tavsr import train as T
    out = []
    for kw in ({}, dict(grad_clip=-1.0), dict(grad_clip=0.0, grad_clip_type=INF)):
        model = _Lin() if loop == "training" else _LinLM()
        opt = torch.optim.Adam(model.parameters(), lr=5e-3, **ADAM)
        sch = _one_cycle(opt, 10)
        if loop == "training":
            loss = T.training(model, [_batch(k, sc) for k, sc in enumerate(SCALES)], opt, sch, 2, device="cpu", **kw)
        else:
            loader = [(torch.full((1, 2), k, dtype=torch.int64), torch.tensor([2]), ["x"]) for k in range(6)]
            loss = T.lm_training(model, loader, opt, sch, 2, device="cpu", **kw)
        out.append((loss, _state(model, opt, sch)))
    for loss, st in out[1:]:
        assert loss == out[0][0]
        _same_state(out[0][1], st)
    assert out[0][1][2] == 3                            # three optimizer steps moved the schedule three times


def test_noam_wrapper_over_a_torch_optimizer_keeps_its_count_on_a_skipped_step():
    from tavsr.train import NoamScheduler, training
    model = _Lin()
    opt = NoamScheduler(256, 1.6, 4, torch.optim.Adam(model.parameters(), lr=0, **ADAM))
    loader = [_batch(0, 0.01), _batch(0, math.nan), _batch(1, 1.0)]
    with pytest.warns(UserWarning, match="1 of 3 optimizer steps"):
        training(model, loader, opt, None, 1, device="cpu", grad_clip=1.0)
    assert opt._step == 2
    want, _ = GR.adam_clip_steps(_Lin().w, [list(b.values()) for b in loader], 1.0, 2.0, lr=opt.rate, **ADAM)
    for a, b in zip(model.parameters(), want):
        assert torch.allclose(a.detach().double(), b, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------ driver, refusals, C ABI
@pytest.mark.parametrize("keys,want", [(dict(grad_clip=5.0, grad_clip_type=INF), (5.0, INF)), (dict(grad_clip=-1.0), (-1.0, 2.0)),
                                       ({}, (-1.0, 2.0))])
def test_lm_main_passes_the_recipe_keys_to_lm_training(tmp_path, monkeypatch, keys, want):
    from tavsr import lm_main
    conf = dict(lm="transformer", lm_conf=dict(att_unit=8, dropout_rate=0.0, embed_unit=8, head=2, layer=1, pos_enc=None, unit=8),
                model_conf=dict(ignore_id=-1), token_list="char/english", token_type="char", bpemodel=None, init=None,
                training_settings=dict(batch_size=2, num_workers=0, optimizer="adam", scheduler="noam", learning_rate=0.01, **keys),
                epochs=2, accum_grad=1, average_epochs=1, device="cpu", dtype="float32")
    recipe, text = tmp_path / "lm.yaml", tmp_path / "text.txt"
    recipe.write_text(yaml.safe_dump(conf))
    text.write_text("hello\nworld\nagain")
    seen = []

    class Opt:
        def clip_stats(self):
            return dict(steps=3, skipped=1, clipped=2, last_norm=0.5)

    def fake_training(lm, loader, optimizer, scheduler, accum_grad, device, **kw):
        seen.append((accum_grad, device, kw))
        return 1.0

    monkeypatch.setattr(lm_main.LMTask, "build_model", staticmethod(lambda conf: torch.nn.Linear(2, 2)))
    monkeypatch.setattr(lm_main, "set_optimizer", lambda conf, lm, loader: (Opt(), None))
    monkeypatch.setattr(lm_main, "lm_training", fake_training)
    monkeypatch.setattr(lm_main, "lm_validation", lambda lm, loader, device: 2.0)
    monkeypatch.setattr(lm_main, "save_model", lambda out, lm, tag: f"{out}/{tag}")
    monkeypatch.setattr(lm_main, "save_val_stats", lambda out, stats: None)
    monkeypatch.setattr(lm_main, "average_model", lambda lm, paths: None)
    data = ["--training-dataset", str(text), "--validation-dataset", str(text), "--test-dataset", str(text)]
    lm_main.main(["--lm-config-file", str(recipe), "--mode", "training", "--output-dir", str(tmp_path / "out")] + data)
    assert len(seen) == 2
    for accum, device, kw in seen:
        assert accum == 1 and device == "cpu" and kw == dict(grad_clip=want[0], grad_clip_type=want[1])


def test_lm_main_prints_the_clip_statistics_after_each_epoch(tmp_path, monkeypatch, capsys):
    test_lm_main_passes_the_recipe_keys_to_lm_training(tmp_path, monkeypatch, dict(grad_clip=5.0), (5.0, 2.0))
    lines = [l for l in capsys.readouterr().out.splitlines() if "GRAD CLIP=" in l]
    assert len(lines) == 2 and all("STEPS=3" in l and "SKIPPED=1" in l and "CLIPPED=2" in l and "LAST NORM=0.5" in l for l in lines)


def test_only_the_two_norm_and_the_infinity_norm_are_taken():
    from tavsr.train import FusedAdam, training
    model = _Lin()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for bad in (1.0, 0.0, 3.0):
        with pytest.raises(ValueError, match="2.0 or float\\('inf'\\)"):
            training(model, [_batch(0, 1.0)], opt, None, 1, device="cpu", grad_clip=1.0, grad_clip_type=bad)
    # the optimizer's own check comes before it touches the device
    bare = FusedAdam.__new__(FusedAdam)
    with pytest.raises(ValueError, match="2.0 or float\\('inf'\\)"):
        bare.set_grad_clip(1.0, norm_type=1.0)


def test_the_clip_symbols_are_declared_and_bound():
    from tavsr import _lib
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    declared = set(re.findall(r"\b(tavsr_[a-z0-9_]+)\s*\(", hdr))
    want = {"tavsr_grad_norm_parts", "tavsr_grad_norm_nparts", "tavsr_grad_norm_tile", "tavsr_grad_norm_span", "tavsr_grad_clip_coef",
            "tavsr_adamw_step_clip"}
    assert want <= declared
    for n in sorted(want):
        assert n in _lib.PROTOTYPES, n
    import ctypes as C
    assert _lib.PROTOTYPES["tavsr_grad_norm_nparts"] == (C.c_int32, [C.c_int64])
    step, clip = _lib.PROTOTYPES["tavsr_adamw_step"], _lib.PROTOTYPES["tavsr_adamw_step_clip"]
    assert clip[0] is step[0] and clip[1] == step[1][:-1] + [C.c_void_p, C.c_void_p]      # one more pointer, in front of the stream
    if os.path.exists(_lib.LIB_PATH):                   # (a tree that has been built: exported as well)
        raw = C.CDLL(_lib.LIB_PATH)
        for n in sorted(want):
            assert hasattr(raw, n), n
