"""E-Branchformer on the HIP path: forward + backward of 12 encoder layers at B = 32, T = 99, D = 256 (cgMLP and feed-forward
units 1024, the recipe's dropout rates), at merge_conv_kernel 3 and 31, against the Branchformer encoder with
``merge_method: concat`` at the same sizes on the same build - and the merge convolution's kernels alone
(tavsr_dwconv_add_fwd / _bwd, csrc/dwconv_time.hip): their time, their share of the step, and the bytes they must move over
that time, at the layer's size (cache resident) and at a size whose working set (not one tensor alone) exceeds the Infinity Cache.

Times are device events around replays of a captured graph (scripts/ffn2_bench.timed).  Writes profiles/ebf_bench.txt."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tailored-avsr_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ffn2_bench import timed  # noqa: E402
from tavsr import ops  # noqa: E402
from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder  # noqa: E402
from tavsr.encoder.e_branchformer import EBranchformerEncoder  # noqa: E402
from tavsr.layers import RelPositionalEncoding  # noqa: E402

COPY_RATE = 6.29e12      # bytes/s of a float4 copy kernel on this chip (8.0e12 by the data sheet)


def step_time(enc, B, T, D):
    enc = enc.cuda().train()
    params = list(enc.parameters())
    xs, pos = RelPositionalEncoding(D, 0.0)(torch.randn(B, T, D, device="cuda"))
    lens = torch.full((B,), T, device="cuda", dtype=torch.int64)
    lens[1::2] -= torch.arange(B // 2, device="cuda") % 20
    mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]
    dy = torch.randn(B, T, D, device="cuda")
    xs.requires_grad_()

    def step():
        for p in params:
            p.grad = None
        xs.grad = None
        h, m = (xs, pos), mask
        for layer in enc.encoders:
            h, m = layer(h, m, lens=lens)
        torch.autograd.backward(h[0], dy)
    return timed(step, iters=40)


def kernel_times(B, T, Cn, K):
    x, du = torch.randn(B * T, Cn, device="cuda"), torch.randn(B * T, Cn, device="cuda")
    w, bias = torch.randn(Cn, K, device="cuda") / K ** 0.5, torch.randn(Cn, device="cuda")
    u, dx = torch.empty_like(x), torch.empty_like(x)
    return (timed(lambda: ops.dwconv_add_fwd(x, w, bias, B, T, out=u)), timed(lambda: ops.dwconv_add_bwd(du, x, w, B, T, dx=dx)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ebf_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ebf_bench.py measures on the GPU: no device found")
    B, T, D, NB = 32, 99, 256, 12
    lines = [f"scripts/ebf_bench.py: forward + backward of {NB} encoder layers, B = {B}, T = {T}, D = {D}, units 1024 / 1024, dropout 0.1,",
             "captured graph, device events; us per step.  Comparator: MyBranchformerEncoder(merge_method='concat'), same sizes, same build."]
    torch.manual_seed(0)
    common = dict(input_size=D, output_size=D, attention_heads=4, num_blocks=NB, input_layer=None, dropout_rate=0.1,
                  positional_dropout_rate=0.0, attention_dropout_rate=0.1, cgmlp_linear_units=1024, linear_units=1024,
                  ffn_activation_type="swish")
    base = step_time(MyBranchformerEncoder(merge_method="concat", **common), B, T, D)
    lines.append(f"  branchformer, merge concat                 {base:9.1f} us")
    M, Cn = B * T, 2 * D
    for K in (3, 31):
        t = step_time(EBranchformerEncoder(use_ffn=True, macaron_ffn=True, merge_conv_kernel=K, **common), B, T, D)
        kf, kb = kernel_times(B, T, Cn, K)
        share = NB * (kf + kb) / t
        lines.append(f"  e_branchformer, merge_conv_kernel {K:2d}       {t:9.1f} us   ({t / base - 1:+.1%} against concat)")
        lines.append(f"      tavsr_dwconv_add_fwd {kf:6.1f} us, tavsr_dwconv_add_bwd (3 launches) {kb:6.1f} us per layer: "
                     f"{NB} x ({kf:.1f} + {kb:.1f}) = {NB * (kf + kb):.0f} us = {share:.1%} of the step")
    lines.append("")
    lines.append("The kernels alone: bytes that must move (fwd: x in, u out; bwd: du and x in, dx out; taps and partial slabs not counted) over")
    lines.append(f"kernel time, against the {COPY_RATE / 1e12:.2f} TB/s of a float4 copy kernel on this chip (8.0 TB/s data sheet).  [B*T, C] fp32:")
    for (b, t_, why) in ((B, T, "the layer's size: 6.5 MB per tensor, cache resident"), (32, 3000, "197 MB per tensor; the 2 (fwd) / 3 (bwd) tensors of a launch, 393 / 590 MB, exceed the 256 MB Infinity Cache")):
        for K in (3, 31):
            kf, kb = kernel_times(b, t_, Cn, K)
            nb = 4.0 * b * t_ * Cn
            lines.append(f"  B {b} T {t_:4d} C {Cn} K {K:2d} ({why})")
            lines.append(f"      fwd {kf:8.1f} us  {2 * nb / kf / 1e6:6.2f} TB/s = {2 * nb / kf * 1e6 / COPY_RATE:5.1%} of the copy rate;   "
                         f"bwd {kb:8.1f} us  {3 * nb / kb / 1e6:6.2f} TB/s = {3 * nb / kb * 1e6 / COPY_RATE:5.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
