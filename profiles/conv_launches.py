"""The trunk's stride-1 3x3 convolution launches of layers 4 and 3 (3200 frames) alone, for counter runs: forward with
conv_posmajor 0 / 3 (position-major, contiguous tile range per XCD) / 1 (sorted tile order), weight gradient with 0 / 3 / 1
and 5 (bit 2: the equal K slices of before round 8; 1 and 3 take slices of two lengths where the planner gives them: layer 3),
each launched twice; the second launch is the one summarised.
usage: rocprofv3 --kernel-trace --pmc <counters> -d DIR -o p --output-format csv -- python3 profiles/conv_launches.py
       python profiles/conv_launches.py --summarise DIR/p_counter_collection.csv      (per launch: every counter, and hit rates)"""
import csv
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tailored-avsr_amd")]
N_IMG = 3200
LAYERS = (("layer 4", 3, 3, 512), ("layer 3", 6, 6, 256))
FLAGS = (0, 3, 1)
DW_FLAGS = (0, 3, 1, 5)


def labels():
    out = []
    for name, H, W, Cc in LAYERS:
        out += [f"{name} forward NT {N_IMG * H * W}x{Cc}x{9 * Cc} posmajor={f}" for f in FLAGS]
        out += [f"{name} wgrad TN {Cc}x{9 * Cc}x{N_IMG * H * W} posmajor={f}" for f in DW_FLAGS]
    return out


def run():
    import torch
    from tavsr import ops
    for name, H, W, Cc in LAYERS:
        M, K = N_IMG * H * W, 9 * Cc
        x = torch.randn(M, Cc, device="cuda")
        w = torch.randn(Cc, K, device="cuda") / K ** 0.5
        dz = torch.randn(M, Cc, device="cuda")
        z = torch.empty(M, Cc, device="cuda")
        dw = torch.empty(Cc, K, device="cuda")
        for f in FLAGS:
            for _ in range(2):
                ops.gemm(M, Cc, K, x, Cc, w, K, z, Cc, conv=(1, H, W, Cc, 1, 9, f))
        for f in DW_FLAGS:
            for _ in range(2):
                ops.gemm(Cc, K, M, dz, Cc, x, Cc, dw, K, a_kmajor=True, b_kmajor=True, conv=(2, H, W, Cc, 1, 9, f))
        torch.cuda.synchronize()


def summarise(path):
    rows = defaultdict(dict)            # dispatch id -> {counter: value}, kernel name
    names = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            if "gemm_glds_kernel" not in r["Kernel_Name"]:
                continue                # (the weight gradients' split-K epilogue and torch's fills are not the launches compared)
            d = int(r["Dispatch_Id"])
            rows[d][r["Counter_Name"]] = rows[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            names[d] = r["Kernel_Name"]
    ids = sorted(rows)
    lab = labels()
    assert len(ids) == 2 * len(lab), (len(ids), len(lab))
    counters = sorted({c for v in rows.values() for c in v})
    print(f"{'launch':58s} " + " ".join(f"{c:>24s}" for c in counters) + ("   L2 hit rate" if "TCC_HIT_sum" in counters else ""))
    for i, name in enumerate(lab):
        v = rows[ids[2 * i + 1]]
        extra = f"   {v['TCC_HIT_sum'] / max(1.0, v['TCC_HIT_sum'] + v['TCC_MISS_sum']):.3f}" if "TCC_HIT_sum" in v else ""
        if "SQ_VALU_MFMA_BUSY_CYCLES" in v and "SQ_BUSY_CU_CYCLES" in v:
            extra += f"   MFMA busy / CU busy {v['SQ_VALU_MFMA_BUSY_CYCLES'] / max(1.0, v['SQ_BUSY_CU_CYCLES']):.3f}"
        if "SQ_WAIT_ANY" in v and "SQ_WAVE_CYCLES" in v:
            extra += f"   wait / wave cycles {v['SQ_WAIT_ANY'] / max(1.0, v['SQ_WAVE_CYCLES']):.3f}"
        print(f"{name:58s} " + " ".join(f"{v.get(c, float('nan')):24.0f}" for c in counters) + extra)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        run()
