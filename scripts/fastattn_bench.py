"""The attention branch of a Branchformer layer, rel_selfattn against fast_selfattn: forward and forward + backward of the branch
alone (behind the layer's LayerNorm: the projections, the attention core, the output projection / ``transform``, every parameter
gradient and the gradient of the normalised rows) at B = 32, D = 256, H = 4, T = 99 and T = 499 (and 199, 299 between them, to place
the crossover), dropout off, ragged lengths.

Times are device events around replays of a captured graph of ten calls (scripts/ffn2_bench.timed); the two forms are measured
alternately, three rounds each, and the table gives the median and the spread.  Writes profiles/fastattn_bench.txt."""
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
from tavsr.layer_blocks import AttnBranch, FastAttnBranch  # noqa: E402
from tavsr.layers import FastSelfAttention, RelPositionalEncoding, RelPositionMultiHeadedAttention  # noqa: E402


def branch_fns(kind, B, T, D, H):
    """(forward, forward + backward) of one attention branch on fixed inputs"""
    torch.manual_seed(0)
    mod = (FastSelfAttention(D, H, 0.0) if kind == "fast_selfattn" else RelPositionMultiHeadedAttention(H, D, 0.0)).cuda()
    p = {"attn." + n: v for n, v in mod.named_parameters()}
    n = torch.randn(B * T, D, device="cuda")
    d_out = torch.randn(B * T, D, device="cuda")
    lens = torch.full((B,), T, device="cuda", dtype=torch.int64)
    lens[1::2] -= torch.arange(B // 2, device="cuda") % 20
    pos = RelPositionalEncoding(D, 0.0).pos_emb(T, n.device)

    def fwd():
        if kind == "fast_selfattn":
            return FastAttnBranch.fwd(n, p, lens, B, T, H, 0.0)
        cx, s = AttnBranch.fwd(n, p, pos, lens, B, T, H, 0.0)
        return ops.linear(cx, p["attn.linear_out.weight"], p["attn.linear_out.bias"]), s

    def fwd_bwd():
        out, s = fwd()
        G, grp = {}, ops.WgradGroup()
        if kind == "fast_selfattn":
            dn = FastAttnBranch.bwd(d_out, s, p, lens, B, T, H, grp, G)
        else:
            dn, _ = AttnBranch.bwd(d_out, s, p, pos, lens, B, T, H, grp, G)
        grp.flush()
        return out, dn, G
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastattn_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fastattn_bench.py measures on the GPU: no device found")
    B, D, H = 32, 256, 4
    TS = (99, 199, 299, 499)
    lines = [f"scripts/fastattn_bench.py: the attention branch of one Branchformer layer alone, B = {B}, D = {D}, H = {H}, dropout off, ragged",
             "lengths; captured graph of ten calls, device events; us per call, median of three alternating rounds (min .. max).",
             "", f"{'T':>5}  {'form':<14} {'forward':>26}  {'forward + backward':>26}"]
    med = {}
    for T in TS:
        fns = {k: branch_fns(k, B, T, D, H) for k in ("rel_selfattn", "fast_selfattn")}
        ts = {(k, j): [] for k in fns for j in (0, 1)}
        for _ in range(3):
            for k in fns:
                for j in (0, 1):
                    ts[(k, j)].append(timed(fns[k][j], iters=60))
        for k in fns:
            cells = []
            for j in (0, 1):
                v = ts[(k, j)]
                med[(T, k, j)] = statistics.median(v)
                cells.append(f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})")
            lines.append(f"{T:>5}  {k:<14} {cells[0]:>26}  {cells[1]:>26}")
    lines.append("")
    for T in TS:
        for j, what in ((0, "forward"), (1, "forward + backward")):
            r = med[(T, "rel_selfattn", j)] / med[(T, "fast_selfattn", j)]
            lines.append(f"T = {T:3d} {what:<19}: rel_selfattn / fast_selfattn = {r:.2f}")
    for j, what in ((0, "forward"), (1, "forward + backward")):
        wins = [T for T in TS if med[(T, "fast_selfattn", j)] < med[(T, "rel_selfattn", j)]]
        if not wins:
            lines.append(f"{what}: the linear form wins at none of the measured lengths: no crossover up to T = {TS[-1]}")
        elif wins[0] == TS[0]:
            lines.append(f"{what}: the linear form wins at every measured length (a crossover, if any, lies below T = {TS[0]})")
        else:
            lines.append(f"{what}: the linear form wins from T = {wins[0]} on (it loses at T = {TS[TS.index(wins[0]) - 1]}: the crossover lies between them)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
