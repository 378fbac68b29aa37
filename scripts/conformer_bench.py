"""Conformer on the HIP path: forward + backward of 12 encoder layers at B = 32, T = 99, D = 256 (macaron_style, use_cnn_module,
cnn_module_kernel 31, feed-forward units 2048, dropout 0.1) against the E-Branchformer encoder (use_ffn, macaron_ffn,
merge_conv_kernel 31, the same feed-forward units, cgMLP units 1024) on the same build in the same run - and the convolution
module's kernels alone (tavsr_glu_dwconv_fwd / _bwd, csrc/dwconv_time.hip) at B = 32, C = 256, K in {3, 31}, T in {99, 3000}:
their time and the bytes they must move (fwd: h in, z out; bwd: dz and h in, dh out) against a float4 copy of as many bytes,
against tavsr_dwconv_add_* at the same C, K, T, and against torch's own F.glu + F.conv1d(groups=C) chain on the device with its
transposes, all taken in the same run.

Times are device events around replays of a captured graph (scripts/ffn2_bench.timed).  Writes profiles/conformer_bench.txt."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tailored-avsr_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ebf_bench import step_time  # noqa: E402
from ffn2_bench import timed  # noqa: E402
from tavsr import ops  # noqa: E402
from tavsr.encoder.conformer import ConformerEncoder  # noqa: E402
from tavsr.encoder.e_branchformer import EBranchformerEncoder  # noqa: E402


def copy_time(nbytes, iters=60):
    """us of a float4 copy kernel (tavsr_multi_copy) that reads nbytes / 2 and writes nbytes / 2"""
    n = int(nbytes) // 8
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    return timed(lambda: ops.multi_copy_([dst], [src]), iters=iters)


def kernel_times(B, T, C, K, iters=60):
    """(glu_dwconv fwd, bwd, dwconv_add fwd, bwd, torch chain fwd) in us; ``iters``: launches in the timed window"""
    M = B * T
    h, dz = torch.randn(M, 2 * C, device="cuda"), torch.randn(M, C, device="cuda")
    w, bias = torch.randn(C, K, device="cuda") / K ** 0.5, torch.randn(C, device="cuda")
    z, dh, dx = torch.empty(M, C, device="cuda"), torch.empty(M, 2 * C, device="cuda"), torch.empty(M, C, device="cuda")
    gf = timed(lambda: ops.glu_dwconv_fwd(h, w, bias, B, T, out=z), iters=iters)
    gb = timed(lambda: ops.glu_dwconv_bwd(dz, h, w, B, T, dh=dh), iters=iters)
    x = h[:, :C].contiguous()
    af = timed(lambda: ops.dwconv_add_fwd(x, w, bias, B, T, out=z), iters=iters)
    ab = timed(lambda: ops.dwconv_add_bwd(dz, x, w, B, T, dx=dx), iters=iters)
    w3, h3 = w.view(C, 1, K), h.view(B, T, 2 * C)

    def chain():      # what a user runs without the kernel: [B, T, 2C] rows in, [B, T, C] rows out
        return F.conv1d(F.glu(h3.transpose(1, 2), dim=1), w3, bias, padding=(K - 1) // 2, groups=C).transpose(1, 2).contiguous()
    with torch.no_grad():
        tf = timed(chain, iters=iters)
    return gf, gb, af, ab, tf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformer_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conformer_bench.py measures on the GPU: no device found")
    B, T, D, NB, K = 32, 99, 256, 12, 31
    lines = [f"scripts/conformer_bench.py: forward + backward of {NB} encoder layers, B = {B}, T = {T}, D = {D}, feed-forward units 2048, dropout 0.1,",
             "captured graph, device events; us per step.  Comparator: EBranchformerEncoder(use_ffn, macaron_ffn, merge_conv_kernel=31, cgMLP units 1024),",
             "same sizes, same build, same run."]
    torch.manual_seed(0)
    common = dict(input_size=D, output_size=D, attention_heads=4, num_blocks=NB, input_layer=None, dropout_rate=0.1,
                  positional_dropout_rate=0.0, attention_dropout_rate=0.1, linear_units=2048)
    base = step_time(EBranchformerEncoder(use_ffn=True, macaron_ffn=True, merge_conv_kernel=K, cgmlp_linear_units=1024,
                                          ffn_activation_type="swish", **common), B, T, D)
    lines.append(f"  e_branchformer, merge_conv_kernel {K}                    {base:9.1f} us")
    t = step_time(ConformerEncoder(macaron_style=True, use_cnn_module=True, cnn_module_kernel=K, rel_pos_type="latest",
                                   activation_type="swish", **common), B, T, D)
    gf, gb, _, _, _ = kernel_times(B, T, D, K, iters=400)
    lines.append(f"  conformer, macaron_style, cnn_module_kernel {K}          {t:9.1f} us   ({t / base - 1:+.1%} against e_branchformer)")
    lines.append(f"      tavsr_glu_dwconv_fwd {gf:6.1f} us, tavsr_glu_dwconv_bwd (3 launches) {gb:6.1f} us per layer: "
                 f"{NB} x ({gf:.1f} + {gb:.1f}) = {NB * (gf + gb):.0f} us = {NB * (gf + gb) / t:.1%} of the step")
    lines.append("")
    lines.append("The kernels alone, C = 256, fp32.  Bytes that must move: fwd h [B*T, 2C] in + z [B*T, C] out = 3 N, bwd dz + h in + dh out = 5 N,")
    lines.append("N = 4 B T C bytes (taps and partial slabs not counted), over kernel time, against a float4 copy kernel moving as many bytes in")
    lines.append("the same run; tavsr_dwconv_add_* at the same C, K, T (it moves 2 N / 3 N); torch's F.glu + F.conv1d(groups=C) chain on [B, T, 2C] rows")
    lines.append("with its transposes (forward only, no_grad).")
    slower = []
    for (b, t_, why) in ((B, T, "the layer's size: h 6.5 MB, cache resident"),
                         (32, 3000, "h 197 MB + z 98 MB, dh 197 MB: the backward's 492 MB exceed the 256 MB Infinity Cache")):
        for k in (3, 31):
            it = 400 if t_ < 1000 else 60      # small launches: a longer window
            gf, gb, af, ab, tf = kernel_times(b, t_, D, k, iters=it)
            n = 4.0 * b * t_ * D
            cf, cb = copy_time(3 * n, it), copy_time(5 * n, it)
            lines.append(f"  B {b} T {t_:4d} C {D} K {k:2d} ({why})")
            lines.append(f"      fwd {gf:8.1f} us  {3 * n / gf / 1e6:6.2f} TB/s; copy of 3 N {cf:8.1f} us ({cf / gf:5.1%} of the kernel's time);  "
                         f"dwconv_add_fwd {af:8.1f} us;  torch chain {tf:8.1f} us ({tf / gf:4.1f} x)")
            lines.append(f"      bwd {gb:8.1f} us  {5 * n / gb / 1e6:6.2f} TB/s; copy of 5 N {cb:8.1f} us ({cb / gb:5.1%} of the kernel's time);  "
                         f"dwconv_add_bwd {ab:8.1f} us")
            if gf > tf:
                slower.append(f"B {b} T {t_} K {k}")
    lines.append("")
    lines.append("tavsr_glu_dwconv_fwd slower than torch's chain: " + ("at " + ", ".join(slower) if slower else "at none of the shapes measured."))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
