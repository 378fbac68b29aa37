"""The cgMLP gate at the kernel sizes the recipes do not use: ops.dwconv_gate_fwd and ops.dwconv_gate_bwd (three launches: the
backward kernel, the slab sum, the split) at K in {3, 15, 45, 63}, C = 1024, r and dr the left halves of [B*T, 2C] buffers as the
layer holds them, at the layer's size (B 32, T 99: 13 MB per tensor, cache resident) and at B 8, T 3000 (98 MB per tensor).  K = 31
has kernels of its own (csrc/cgmlp.hip) and benches of its own (scripts/csgu_bench.py, scripts/act_bwd_bench.py).

Times are device events around replays of a captured graph (scripts/ffn2_bench.timed); a case's figure is the median of
``--windows`` such windows.  One run prints one table; to compare two builds, run each several times, alternating (TAVSR_LIB
selects the library), and take the spread of a build's own medians as the margin: profiles/gate_bench.txt."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tailored-avsr_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ffn2_bench import timed  # noqa: E402
from tavsr import ops  # noqa: E402

SHAPES = ((32, 99), (8, 3000))
KERNEL_SIZES = (3, 15, 45, 63)
C = 1024


def case_times(B, T, K, windows):
    M = B * T
    g = torch.Generator(device="cuda").manual_seed(1000 * K + T)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    gn, du, wide, dwide = rn(M, C), rn(M, C), rn(M, 2 * C), torch.empty(M, 2 * C, device="cuda")
    w, bias = rn(C, K) / K ** 0.5, rn(C)
    r, dr = wide[:, :C], dwide[:, :C]
    _, conv = ops.dwconv_gate_fwd(gn, r, w, bias, B, T)
    fwd = [timed(lambda: ops.dwconv_gate_fwd(gn, r, w, bias, B, T)) for _ in range(windows)]
    bwd = [timed(lambda: ops.dwconv_gate_bwd(du, gn, r, conv, w, dr, B, T)) for _ in range(windows)]
    return statistics.median(fwd), statistics.median(bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gate_bench.py measures on the GPU: no device found")
    lines = [f"scripts/gate_bench.py: C = {C}, captured graph, device events; us per call, median of {args.windows} windows of 60 calls"]
    for B, T in SHAPES:
        for K in KERNEL_SIZES:
            f, b = case_times(B, T, K, args.windows)
            lines.append(f"  B {B:2d} T {T:4d} K {K:2d}   fwd {f:9.2f}   bwd {b:9.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
