"""Per-workgroup phase timeline of the LDS-DMA GEMM kernel (debug build with -DTAVSR_GEMM_TRACE, see
scripts/gpu_trace.sh).  For each shape: one traced launch; prints the launch span and, over the workgroups,
start offset / prologue (entry -> first tile landed) / K loop / epilogue in microseconds (wall_clock64, 100 MHz).
usage: TAVSR_LIB=.../lib_trace/libtavsr_hip.so python profiles/gemm_trace.py
       ... gemm_trace.py --conv     the trunk's 3x3 implicit convolutions of layers 4 and 3 (3200 frames): forward with
                                    conv_posmajor 0 / 3 (position-major, one contiguous tile range per XCD) / 1 (sorted tile
                                    order), weight gradient with 0 / 3 / 1 (taps heaviest first); per tile class (K-steps executed) and per XCD"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tailored-avsr_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tavsr import _lib, ops  # noqa: E402

SHAPES = [("NT", 3168, 2048, 256, (4, 1)), ("NT", 3168, 2048, 256, (8, 1)), ("NT", 3168, 256, 2048, (4, 1)),
          ("NT", 3168, 256, 2048, (8, 4)), ("NT", 3168, 256, 2048, (8, 5)), ("NT", 3168, 256, 256, (4, 1)),
          ("NN", 3168, 256, 2048, (4, 1)), ("TN", 2048, 256, 3168, (4, 4))]


def pct(x):
    return " ".join(f"{np.percentile(x, q):7.2f}" for q in (0, 10, 50, 90, 100))


def read_trace(L, buf):
    n = L.tavsr_gemm_trace_read(buf.ctypes.data_as(C.c_void_p), buf.shape[0])
    t = buf[:n, :4].astype(np.int64)
    us = (t - t[:, 0].min()) / 100.0
    xcc = ((buf[:n, 4] >> np.uint64(32)) & np.uint64(0xF)).astype(np.int64)
    cyc = (buf[:n, 5] & np.uint64((1 << 40) - 1)).astype(np.float64)
    nk = (buf[:n, 5] >> np.uint64(40)).astype(np.int64)
    return n, us, xcc, cyc, nk


def conv_main():
    """per traced tile: K-steps executed, K-loop cycles, prologue / epilogue, XCD, start time"""
    L = _lib.lib()
    L.tavsr_gemm_trace_read.restype = C.c_int
    buf = np.zeros((1 << 15, 6), dtype=np.uint64)
    n_img = 3200
    for name, H, W, Cc in (("layer 4", 3, 3, 512), ("layer 3", 6, 6, 256)):
        M, K = n_img * H * W, 9 * Cc
        x = torch.randn(M, Cc, device="cuda")
        w = torch.randn(Cc, K, device="cuda") / K ** 0.5
        dz = torch.randn(M, Cc, device="cuda")
        z = torch.empty(M, Cc, device="cuda")
        dw = torch.empty(Cc, K, device="cuda")
        launches = [(f"{name} forward NT {M}x{Cc}x{K} conv_posmajor={f}", f,
                     lambda f=f: ops.gemm(M, Cc, K, x, Cc, w, K, z, Cc, conv=(1, H, W, Cc, 1, 9, f))) for f in (0, 3, 1)]
        launches += [(f"{name} weight gradient TN {Cc}x{K}x{M} conv_posmajor={f}", f,
                      lambda f=f: ops.gemm(Cc, K, M, dz, Cc, x, Cc, dw, K, a_kmajor=True, b_kmajor=True, conv=(2, H, W, Cc, 1, 9, f)))
                     for f in (0, 3, 1)]
        for title, f, run in launches:
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            L.tavsr_gemm_trace_read(buf.ctypes.data_as(C.c_void_p), buf.shape[0])     # reset
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            n, us, xcc, cyc, nk = read_trace(L, buf)
            life = np.maximum(us[:, 3] - us[:, 0], 1e-3)
            outside = 1.0 - (us[:, 2] - us[:, 1]) / life
            print(f"== {title}: {n} workgroups, span {us[:, 3].max():.1f} us (events {e0.elapsed_time(e1) * 1e3:.1f} us, traced kernels "
                  f"only), outside the K loop: {100 * outside.mean():.1f} % of a tile's life (prologue {np.mean(us[:, 1] - us[:, 0]):.2f} us, "
                  f"epilogue {np.mean(us[:, 3] - us[:, 2]):.2f} us of {life.mean():.1f} us)")
            print("   per XCD: tiles, K-steps, first start, last end (us)")
            for xc in np.unique(xcc):
                s = xcc == xc
                print(f"     xcd {xc}: {s.sum():5d} {nk[s].sum():8d} {us[s, 0].min():8.1f} {us[s, 3].max():8.1f}")
            print("   per tile class (K-steps executed): tiles, cycles per K-step p10 / p50 / p90, K loop us p50, by quartile of start time p50")
            cps = cyc / np.maximum(nk - 1, 1)           # the cycle counter starts behind the first step's barrier
            for k in np.unique(nk)[::-1]:
                s = nk == k
                order = np.argsort(us[s, 0])
                q = [np.median(cps[s][part]) for part in np.array_split(order, 4) if len(part)]
                print(f"     {k:4d}: {s.sum():5d}  {np.percentile(cps[s], 10):7.0f} {np.median(cps[s]):7.0f} {np.percentile(cps[s], 90):7.0f}  "
                      f"{np.median(us[s, 2] - us[s, 1]):7.1f}   " + " ".join(f"{v:7.0f}" for v in q), flush=True)


def main():
    if "--conv" in sys.argv[1:]:
        return conv_main()
    L = _lib.lib()
    L.tavsr_gemm_trace_read.restype = C.c_int
    buf = np.zeros((1 << 15, 6), dtype=np.uint64)
    for mode, M, N, K, force in SHAPES:
        a = torch.randn(M, K, device="cuda")
        b = torch.randn(K, N, device="cuda")
        A = a.t().contiguous() if mode == "TN" else a
        B = b if mode != "NT" else b.t().contiguous()
        Cout = torch.empty(M, N, device="cuda")
        kw = dict(a_kmajor=mode == "TN", b_kmajor=mode != "NT")
        for _ in range(3):
            ops.gemm(M, N, K, A, A.stride(0), B, B.stride(0), Cout, N, force=force, **kw)
        torch.cuda.synchronize()
        L.tavsr_gemm_trace_read(buf.ctypes.data_as(C.c_void_p), buf.shape[0])     # reset
        ops.gemm(M, N, K, A, A.stride(0), B, B.stride(0), Cout, N, force=force, **kw)
        n = L.tavsr_gemm_trace_read(buf.ctypes.data_as(C.c_void_p), buf.shape[0])
        t = buf[:n, :4].astype(np.int64)
        t0 = t[:, 0].min()
        us = (t - t0) / 100.0
        hw = buf[:n, 4]
        xcc = (hw >> np.uint64(32)) & np.uint64(0xF)
        hwid = hw & np.uint64(0xFFFFFFFF)
        cu = (hwid >> np.uint64(8)) & np.uint64(0xF)
        sh = (hwid >> np.uint64(12)) & np.uint64(0x1)
        se = (hwid >> np.uint64(13)) & np.uint64(0x7)
        cuid = (xcc * np.uint64(8) + se) * np.uint64(32) + sh * np.uint64(16) + cu
        ncu = len(np.unique(cuid))
        per_cu = np.bincount(np.unique(cuid, return_inverse=True)[1])
        print(f"== {mode} M={M} N={N} K={K} cfg/split={force}: {n} workgroups on {ncu} CUs "
              f"(per CU min/med/max {per_cu.min()}/{int(np.median(per_cu))}/{per_cu.max()}), span {us[:, 3].max():.2f} us")
        print(f"   percentiles            {'p0':>7} {'p10':>7} {'p50':>7} {'p90':>7} {'p100':>7}")
        print(f"   start offset           {pct(us[:, 0])}")
        print(f"   prologue (first tile)  {pct(us[:, 1] - us[:, 0])}")
        print(f"   K loop                 {pct(us[:, 2] - us[:, 1])}")
        print(f"   epilogue               {pct(us[:, 3] - us[:, 2])}")
        print(f"   lifetime               {pct(us[:, 3] - us[:, 0])}")
        print(f"   end                    {pct(us[:, 3])}")
        cyc = (buf[:n, 5] & np.uint64((1 << 40) - 1)).astype(np.float64)      # (the K-steps executed sit above bit 40)
        loop_us = np.maximum(us[:, 2] - us[:, 1], 1e-3)
        nk = max(1, (K // force[1]) // 32 - 1)
        print(f"   K-loop cycles/K-step   {pct(cyc / nk)}   shader clock GHz {pct(cyc / loop_us / 1e3)}", flush=True)


if __name__ == "__main__":
    main()
