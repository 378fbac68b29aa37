"""GPU: the encoders' feed-forward activations beyond the recipes' relu / swish - tanh, hardtanh, selu (espnet get_activation,
src/encoder/branchformer/encoder.py:206, src/encoder/audiovisual/tailored/encoder.py:99) - kernel by kernel against fp64
(the GEMM's epilogue for them, the streaming FFN kernels csrc/ffn2.hip forward and data gradient), the layer against the
reference's own vectors (tests/golden/bf_layer_ffn_*.npz), a training step against the oracle, every route selector of the
feed-forward block, and the C-side layer sequencer bit-equal to the Python sequencing."""
import argparse
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import asr_conf, golden, grad_ok, max_rel, rel_err

pytestmark = pytest.mark.gpu

NEW_ACTS = ("tanh", "hardtanh", "selu")
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772


def _act64(name, z):
    z = z.double()
    return {"tanh": torch.tanh, "hardtanh": F.hardtanh, "selu": torch.selu}[name](z)


def _dact64(name, z):
    z = z.double()
    if name == "tanh":
        return 1 - torch.tanh(z) ** 2
    if name == "hardtanh":
        return ((z > -1) & (z < 1)).double()
    return torch.where(z <= 0, SELU_SCALE * SELU_ALPHA * torch.exp(z), torch.full_like(z, SELU_SCALE))


def _special_z():
    """kinks, both sides of them, the Taylor / closed-form seams (|z| = 1/4), |z| < 1e-3, saturation and a spread of ordinary values"""
    base = [0.0, 1.0, -1.0, 0.25, -0.25, 1e-3, -1e-3, 3e-4, -7e-5, 1e-6, -1e-8, 20.0, -20.0, 9.0, -9.0, 88.0, -88.0, 0.5, -0.5]
    eps = [1 + 2 ** -23, 1 - 2 ** -24]
    vals = base + [s * e for s in (1.0, -1.0, 0.25, -0.25) for e in eps]
    g = torch.Generator().manual_seed(3)
    vals += (torch.randn(4096 - len(vals), generator=g) * 3).tolist()
    return torch.tensor(vals, dtype=torch.float32)


def _per_element_ok(got, want, tol=1e-6):
    got, want = got.double().cpu(), want.double().cpu()
    bad = (got - want).abs() > tol * want.abs().clamp_min(1.0)
    assert not bool(bad.any()), (int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


@pytest.mark.parametrize("act", NEW_ACTS)
def test_gemm_epilogue_activation_and_derivative_vs_fp64(act):
    from tavsr import ops
    z = _special_z().cuda()
    M, N, K = 64, z.numel(), 32
    # forward: A = 0, so C[m][n] = act(bias[n]) and Z = bias exactly
    y, zz = ops.linear(torch.zeros(M, K, device="cuda"), torch.randn(N, K, device="cuda"), z, act=act, save_z=True)
    assert torch.equal(zz, z.expand(M, N))
    _per_element_ok(y, _act64(act, z).expand(M, N))
    small = (z.abs() < 1e-3) & (z != 0)                    # relative accuracy kept near 0 (no 1 - 2 / (e^2z + 1) cancellation)
    assert float((y[0][small].double() / _act64(act, z[small]).cuda() - 1).abs().max()) < 1e-6
    # backward: dy = 1, w = 1/32, so dy w = 1 exactly and the result is act'(DZ)
    dx = ops.linear_dx(torch.ones(M, K, device="cuda"), torch.full((K, N), 1.0 / K, device="cuda"), DZ=z.expand(M, N).contiguous(),
                       dact=act)
    _per_element_ok(dx, _dact64(act, z).expand(M, N))


@pytest.mark.parametrize("act", NEW_ACTS)
def test_gemm_epilogue_with_dropout_regenerates_the_mask(act):
    from tavsr import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    M, K, N = 300, 256, 2048
    x, w, b = (torch.randn(M, K, device="cuda", generator=g), torch.randn(N, K, device="cuda", generator=g) / 16,
               torch.randn(N, device="cuda", generator=g) * 0.1)
    ops.manual_seed(77)
    h, z, tok = ops.linear_drop(x, w, b, 0.1, act=act, save_z=True)
    keep = ops.dropout(torch.ones(M, N, device="cuda"), tok[0], token=tok)[0].double()       # mask / (1 - p) of the same token
    assert 0.85 < float((keep > 0).double().mean()) < 0.95
    zr = x.double() @ w.double().t() + b.double()
    assert max_rel(z, zr) < 2e-6
    assert max_rel(h, keep * _act64(act, zr)) < 2e-6
    dy = torch.randn(M, K, device="cuda", generator=g)
    dh = ops.linear_dx_drop(dy, w.t().contiguous(), tok, alpha=0.5, DZ=z, dact=act)
    assert max_rel(dh, 0.5 * (dy.double() @ w.double().t()) * keep * _dact64(act, z)) < 2e-6


def _ffn_params(D, N1, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return (1 + 0.1 * r(D), 0.1 * r(D), r(N1, D) / D ** 0.5, 0.1 * r(N1), r(D, N1) / N1 ** 0.5, 0.1 * r(D))


@pytest.mark.parametrize("M", [3168, 300])
@pytest.mark.parametrize("act", NEW_ACTS)
def test_ffn2_forward_and_data_gradient_vs_fp64(act, M):
    from tavsr import ops
    D, N1 = 256, 2048
    ln_w, ln_b, w1, b1, w2, b2 = _ffn_params(D, N1, seed=M)
    x = torch.randn(M, D, device="cuda")
    assert ops.ffn2_usable(x, w1, act)
    y, (n, mean, rstd, z, h, t_in, t_out), _, _ = ops.ffn2_fwd(x, ln_w, ln_b, 1e-12, w1, b1, w2, b2, act, 0.5, save=True)
    xd = x.double()
    nr = F.layer_norm(xd, (D,), ln_w.double(), ln_b.double(), 1e-12)
    zr = nr @ w1.double().t() + b1.double()
    hr = _act64(act, zr)
    assert max_rel(z, zr) < 5e-6
    assert max_rel(h, hr) < 5e-6
    assert max_rel(h, _act64(act, z)) < 1e-6              # the activation itself, on the kernel's own pre-activations
    assert max_rel(y, xd + 0.5 * (hr @ w2.double().t() + b2.double())) < 5e-6
    dyd = torch.randn(M, D, device="cuda")
    dz, dn = ops.ffn2_bwd_dx(dyd, 0.5, w1, w2, z, act, None)
    dzr = 0.5 * (dyd.double() @ w2.double()) * _dact64(act, z)
    assert max_rel(dz, dzr) < 5e-6
    assert max_rel(dn, dzr @ w1.double()) < 5e-6


def _fill(module, seed):
    from oracle.model import fill_parameters_
    fill_parameters_(module, seed=seed)
    return module.cuda()


@pytest.mark.parametrize("act", NEW_ACTS)
def test_layer_vs_reference_golden(act):
    from oracle.model import compact, synth
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.layers import RelPositionalEncoding
    g = golden(f"bf_layer_ffn_{act}")
    B, T, D = int(g["B"]), int(g["T"]), int(g["D"])
    enc = MyBranchformerEncoder(input_size=D, num_blocks=1, input_layer=None, dropout_rate=0.0, positional_dropout_rate=0.0,
                                attention_dropout_rate=0.0, ffn_activation_type=act, merge_method="learned_ave")
    layer = enc.encoders[0]
    assert sorted(layer.state_dict().keys()) == list(g["keys"])
    layer = _fill(layer, 21).train()
    lens = torch.from_numpy(g["lens"]).cuda()
    mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    x = synth((B, T, D), seed=22).cuda()
    xs, pos = RelPositionalEncoding(D, 0.0)(x)
    xs = xs.detach().requires_grad_(True)
    (y, _), _ = layer((xs, pos), mask)
    (y * synth((B, T, D), seed=23).cuda()).sum().backward()
    assert max_rel(y.cpu(), g["y"]) < 1e-4
    assert rel_err(xs.grad.cpu() * 16.0, g["grad_x"]) < 1e-3          # golden grad is w.r.t. the unscaled input
    for n, p in layer.named_parameters():
        if "g_" + n in g.files:
            assert grad_ok(compact(p.grad.cpu()), g["g_" + n], 1e-3), n
    assert rel_err(layer.weight_global.cpu(), g["weight_global"]) < 1e-4


@pytest.mark.parametrize("act", ["tanh", "selu"])
def test_asr_training_step_vs_oracle(act):
    from oracle.model import build_asr_oracle, compact, fill_parameters_, synth
    from tavsr.tasks.asr import ASRTask
    from tavsr.utils.tokens import CHAR_ENGLISH
    conf = asr_conf(num_blocks=2, dec_blocks=1, ffn_activation_type=act)
    oracle = build_asr_oracle(copy.deepcopy(conf), CHAR_ENGLISH).train()
    fill_parameters_(oracle, seed=7)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf)))
    model.load_state_dict(oracle.state_dict())
    model = model.cuda().train()
    speech, slens = synth((4, 400, 80), seed=8), torch.tensor([400, 372, 333, 251])
    text, tlens = synth((4, 30), seed=9, kind="int", lo=1, hi=40), torch.tensor([30, 25, 20, 12])
    for b in range(4):
        text[b, int(tlens[b]):] = -1
    lo = oracle(speech, slens, text, tlens)[0]
    lo.backward()
    lg = model(speech.cuda(), slens.cuda(), text.cuda(), tlens.cuda())[0]
    lg.backward()
    assert abs(float(lg) - float(lo)) < 1e-4 * abs(float(lo))
    go, gg = dict(oracle.named_parameters()), dict(model.named_parameters())
    for n in go:
        if ".feed_forward" in n or "linear_pos" in n or n.startswith("encoder.embed"):
            assert grad_ok(compact(gg[n].grad.cpu()), compact(go[n].grad), 1e-3), n


FFN_SWITCHES = [("tavsr.ops", "FFN2", False), ("tavsr.ops", "FFN2_BWD", False), ("tavsr.ops", "FFN2_BWD_LN", False),
                ("tavsr.ops", "LN_BWD_DROP", False), ("tavsr.ops", "LAYER_C", False), ("tavsr.ops", "WGRAD_BESIDE", False),
                ("tavsr._lib", "SINGLE_STREAM", True)]


def _asr_model(act, dropout):
    from oracle.model import synth
    from tavsr.tasks.asr import ASRTask
    torch.manual_seed(0)
    model = ASRTask.build_model(argparse.Namespace(**asr_conf(num_blocks=2, dec_blocks=1, dropout=dropout,
                                                              ffn_activation_type=act)))
    text = synth((4, 30), seed=2, kind="int", lo=1, hi=40)
    batch = [synth((4, 400, 80), seed=1).cuda(), torch.tensor([400, 372, 333, 251]).cuda(), text.cuda(),
             torch.full((4,), 30).cuda()]
    model = model.cuda().train()
    return model, batch, [p for p in model.parameters() if p.requires_grad]


def _step(model, batch, params):
    from tavsr import ops
    ops.manual_seed(4242)
    torch.manual_seed(3)
    for p in params:
        p.grad = None
    loss = model(*batch)[0]
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), [p.grad.detach().clone() for p in params]


@pytest.mark.parametrize("act,dropout", [("tanh", 0.0), ("hardtanh", 0.1), ("selu", 0.1)])
def test_every_feed_forward_route_agrees(act, dropout):
    """each route selector of the block flipped alone (the GEMM-epilogue route, the two-GEMM data gradient, the C-side
    sequencer off, the weight gradients in line, one queue): loss and every gradient as the default route's"""
    model, batch, params = _asr_model(act, dropout)
    ref = _step(model, batch, params)
    names = [n for n, _ in model.named_parameters()]
    for mod, name, value in FFN_SWITCHES:
        m = importlib.import_module(mod)
        keep = getattr(m, name)
        assert keep != value, (mod, name)
        setattr(m, name, value)
        try:
            got = _step(model, batch, params)
        finally:
            setattr(m, name, keep)
        assert abs(got[0] - ref[0]) < 1e-4 * abs(ref[0]), (name, got[0], ref[0])
        bad = [n for n, a, b in zip(names, got[1], ref[1]) if not grad_ok(a, b, 2e-3)]
        assert not bad, (name, bad[:6])


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("act", NEW_ACTS)
def test_layer_sequencer_in_c_equals_python_sequencing(act, train):
    from tavsr import ops
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.layers import RelPositionalEncoding
    B, T, D = 3, 99, 256
    lens = torch.tensor([99, 66, 49], device="cuda")

    def run(layer_c):
        keep = ops.LAYER_C
        ops.LAYER_C = layer_c
        try:
            torch.manual_seed(0)
            p = 0.1 if train else 0.0
            enc = MyBranchformerEncoder(input_size=D, num_blocks=2, input_layer=None, dropout_rate=p, positional_dropout_rate=0.0,
                                        attention_dropout_rate=p, ffn_activation_type=act, merge_method="learned_ave").cuda()
            enc.train(train)
            g = torch.Generator(device="cuda").manual_seed(5)
            xs, pos = RelPositionalEncoding(D, 0.0)(torch.randn(B, T, D, device="cuda", generator=g))
            xs = xs.detach().requires_grad_(train)
            mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
            ops.manual_seed(123)
            h = (xs, pos)
            with torch.set_grad_enabled(train):
                for layer in enc.encoders:
                    h, mask = layer(h, mask)
            grads = []
            if train:
                (h[0] * torch.randn(B, T, D, device="cuda", generator=g)).sum().backward()
                grads = [xs.grad] + [q.grad for _, q in sorted(enc.named_parameters()) if q.grad is not None]
            return h[0].detach(), grads
        finally:
            ops.LAYER_C = keep

    y_c, g_c = run(True)
    y_p, g_p = run(False)
    assert torch.equal(y_c, y_p)
    assert len(g_c) == len(g_p)
    for a, b in zip(g_c, g_p):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_the_c_abi_refuses_what_the_runtime_switch_kernels_do_not_hold():
    from tavsr import ops
    from tavsr._lib import TavsrError
    x = torch.randn(64, device="cuda")
    with pytest.raises(TavsrError):
        ops.act_bwd_(x.clone(), x, "tanh")
