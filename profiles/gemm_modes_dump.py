"""One small problem per operand source and layout of the LDS-DMA GEMM (csrc/gemm_glds.h, gemm.hip, gemm_conv.hip), fixed seeds,
every output written as .npy - run once under each of two builds of the library (TAVSR_LIB) and compare the directories with
profiles/dump_outputs_cmp.py: a refactor of the kernels must leave every file bit-identical.
usage: [TAVSR_LIB=.../libtavsr_hip.so] python profiles/gemm_modes_dump.py OUT_DIR"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tailored-avsr_amd"))
from tavsr import ops  # noqa: E402

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(1234)


def rnd(*shape):
    return torch.randn(*shape, device="cuda", generator=gen)


def save(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        np.save(os.path.join(out_dir, name + (f".{i}" if len(tensors) > 1 else "") + ".npy"), t.detach().cpu().numpy())


# ---- plain source: the four layouts on every LDS-DMA tile configuration (cfg 7: two wave sets), K split 1 and 3
M, N, K = 300, 200, 416
a, b = rnd(M, K), rnd(K, N)
for mode in ("NT", "NN", "TN", "TT"):
    A = a.t().contiguous() if mode[0] == "T" else a
    B = b if mode[1] == "N" else b.t().contiguous()
    for cfg in range(9):
        for ns in (1, 3):
            out = torch.zeros(M, N, device="cuda")
            ops.gemm(M, N, K, A, A.stride(0), B, B.stride(0), out, N, a_kmajor=mode[0] == "T", b_kmajor=mode[1] == "N", force=(cfg, ns))
            save(f"plain_{mode}_cfg{cfg}_ns{ns}", out)

# ---- K tail: K % 4 == 0 and != 0, without and with the planner's split (few tiles, K >= 512)
for (M, N, K) in ((100, 64, 100), (99, 64, 197), (128, 256, 2052), (256, 256, 3170)):
    a, b = rnd(M, K), rnd(K, N)
    k4, m4, n4 = (K + 3) // 4 * 4, (M + 3) // 4 * 4, (N + 3) // 4 * 4
    for mode in ("NT", "NN", "TN", "TT"):
        a_km, b_km = mode[0] == "T", mode[1] == "N"
        if (a_km and M % 4) or (b_km and N % 4):
            continue
        A = torch.full((K, m4) if a_km else (M, k4), float("nan"), device="cuda")
        B = torch.full((K, n4) if b_km else (N, k4), float("nan"), device="cuda")
        if a_km:
            A[:, :M] = a.t()
        else:
            A[:, :K] = a
        if b_km:
            B[:, :N] = b
        else:
            B[:, :K] = b.t()
        out = torch.empty(M, N, device="cuda")
        ops.gemm(M, N, K, A, A.stride(0), B, B.stride(0), out, N, a_kmajor=a_km, b_kmajor=b_km)
        save(f"tail_{mode}_{M}x{N}x{K}", out)

# ---- grouped launch of three problems
x = rnd(197, 256)
wbs = [(rnd(n, 256), rnd(n), off) for n, off in ((256, 0), (64, 256), (128, 320))]
out = torch.zeros(197, 448, device="cuda")
ops.linear_group(x, wbs, out)
save("grouped3", out)

# ---- fused bias gradient (row sums of op(A)), without and with split
for (M, N, K) in ((256, 64, 96), (256, 256, 3168)):
    dy, xx = rnd(K, M), rnd(K, N)
    gw, gb = torch.empty(M, N, device="cuda"), torch.empty(M, device="cuda")
    ops.gemm(M, N, K, dy, M, xx, N, gw, N, a_kmajor=True, b_kmajor=True, alpha=0.5, a_rowsum=gb)
    save(f"rowsum_{M}x{N}x{K}", gw, gb)

# ---- tavsr_gemm_ln (split and unsplit plans)
for (M, N, K) in ((77, 256, 2048), (640, 256, 256)):
    x, w, bb, rs, gam, bet = rnd(M, K), rnd(N, K) / K ** 0.5, rnd(N), rnd(M, N), rnd(N).abs() + 0.5, rnd(N)
    y, n = ops.linear(x, w, bb, act="relu", res=rs, ln=(gam, bet, 1e-12))
    save(f"ln_{M}x{N}x{K}", y, n)


# ---- CONV 1: image rows (forward / data gradient)
def conv1(name, imgs, H, W, cin, cout, stride=1, taps=9, pad0=False, pm=0, b_kmajor=False, res=False, dz=False):
    x = rnd(imgs * H * W, cin)
    if pad0:
        Ho, Wo = (H - 3) // stride + 1, (W - 3) // stride + 1
    else:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Mo, Kc = imgs * Ho * Wo, taps * cin
    w = rnd(Kc, cout) if b_kmajor else rnd(cout, Kc)
    z = torch.empty(Mo, cout, device="cuda")
    R = rnd(Mo, cout) if res else None
    DZ = rnd(Mo, cout) if dz else None
    ops.gemm(Mo, cout, Kc, x, cin, w, w.stride(0), z, cout, b_kmajor=b_kmajor, conv=(1, H, W, cin, stride, 90 if pad0 else taps, pm),
             bias=rnd(cout), act="relu" if not dz else None, R=R, ldr=cout if res else 0, DZ=DZ, dact="relu" if dz else None)
    save("conv1_" + name, z)


conv1("s1_c64", 4, 6, 6, 64, 64)
conv1("s1_c128", 4, 6, 6, 64, 128)
conv1("s1_c64_bk_res_dz", 4, 6, 6, 64, 64, b_kmajor=True, res=True, dz=True)
conv1("s1_c128_res", 4, 6, 6, 64, 128, res=True)
conv1("s2", 4, 6, 6, 64, 64, stride=2)
conv1("1x1_s2", 4, 6, 6, 64, 64, stride=2, taps=1)
conv1("pad0_s2", 2, 9, 9, 32, 64, stride=2, pad0=True)
for pm in (1, 3):
    for cout in (64, 128):
        conv1(f"pm{pm}_3x3_n64_c{cout}", 64, 3, 3, 64, cout, pm=pm)          # every tile on one position
        conv1(f"pm{pm}_6x6_n5_c{cout}", 5, 6, 6, 64, cout, pm=pm)            # tiles straddle positions
    conv1(f"pm{pm}_3x3_n64_bk_res", 64, 3, 3, 64, 64, pm=pm, b_kmajor=True, res=True)
conv1("pm9_6to3", 8, 6, 6, 64, 64, stride=2, pm=9)
conv1("pm9_6to3_c128", 8, 6, 6, 64, 128, stride=2, pm=9)


# ---- CONV 2: image patches as the k-major B operand (weight gradient)
def conv2(name, imgs, H, W, cin, cout, pm=0, force=None, rowsum=False):
    dz, x = rnd(imgs * H * W, cout), rnd(imgs * H * W, cin)
    dw = torch.empty(cout, 9 * cin, device="cuda")
    gb = torch.empty(cout, device="cuda") if rowsum else None
    ops.gemm(cout, 9 * cin, imgs * H * W, dz, cout, x, cin, dw, 9 * cin, a_kmajor=True, b_kmajor=True, conv=(2, H, W, cin, 1, 9, pm),
             a_rowsum=gb, force=force)
    save("conv2_" + name, *([dw, gb] if rowsum else [dw]))


for cout in (64, 128):
    for pm in (0, 1, 5):
        conv2(f"c{cout}_pm{pm}_3x3", 64, 3, 3, 64, cout, pm=pm)
        conv2(f"c{cout}_pm{pm}_6x6", 24, 6, 6, 64, cout, pm=pm)
    conv2(f"c{cout}_pm1_3x3_two_lengths", 352, 3, 3, 64, cout, pm=1, force=(-1, 8))      # K = 3168: 11 units of 288 over 8 slices
    conv2(f"c{cout}_pm1_6x6_two_lengths", 88, 6, 6, 64, cout, pm=1, force=(-1, 8))
    conv2(f"c{cout}_pm1_3x3_rowsum", 64, 3, 3, 64, cout, pm=1, rowsum=True)
    conv2(f"c{cout}_pm0_6x6_rowsum", 24, 6, 6, 64, cout, pm=0, rowsum=True)

# ---- Conv3d stem, modes 4 / 5 (4-byte gathers) and 6 / 7 (padded clips): one clip of 2 frames of 16x16
clip = rnd(1, 2, 16, 16)
w0 = torch.zeros(64, 256, device="cuda")
w0[:, :245] = rnd(64, 245)
z4, Ho, Wo = ops.stem_conv_fwd(clip, w0)
save("stem4", z4)
dzs = rnd(z4.shape[0], 64)
save("stem5", ops.stem_conv_dw(dzs, clip))
xp = ops.stem_pad(clip)
w288 = ops.stem_weight_288(w0[:, :245].reshape(64, 1, 5, 7, 7))
z6, _, _ = ops.stem_conv_fwd_pad16(xp, w288, 1, 2, 16, 16)
save("stem6", z6)
save("stem7", ops.stem_conv_dw_pad16(dzs, xp, 2, 16, 16))
print(f"wrote {len(os.listdir(out_dir))} files to {out_dir}")
