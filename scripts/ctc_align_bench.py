"""CTC forced alignment: time per batch of tavsr_ctc_align (ops.ctc_align, both routes) beside the two ways to get an alignment
without it - the same recursion written with torch device ops (one chain of T dependent steps of a dozen launches each, then T
back-trace steps; what a user would write today) and the float64 host reference of tests/ctc_align_ref.py (logits copied to
the host, one Python loop per utterance).  Two shapes: the bench config's batch (N = 32, T = 100, L = 40, V = 41) and long
utterances with a large vocabulary (N = 8, T = 499, L = 200, V = 5000).  Every utterance has all T frames and all L tokens,
N(0,1) logits, about 30 % repeated tokens.  Device times: HIP events around the call (allocations included), p50 over the
timed repetitions after two warm-up calls; host reference: wall clock around the copy and the loop.

    python scripts/ctc_align_bench.py [--out profiles/ctc_align_bench.txt] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tailored-avsr_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(32, 100, 40, 41), (8, 499, 200, 5000)]


def torch_align(logits, targets, blank=0):
    """the recursion of tavsr_ctc_align with torch device ops, for full-length utterances: -> (align [N, T], score [N])"""
    N, T, V = logits.shape
    L = targets.shape[1]
    S = 2 * L + 1
    dev = logits.device
    ninf = float("-inf")
    lp = logits.log_softmax(-1)
    lab = torch.full((N, S), blank, dtype=torch.int64, device=dev)
    lab[:, 1::2] = targets
    em = lp.gather(2, lab[:, None, :].expand(N, T, S))
    skip = torch.zeros((N, S), dtype=torch.bool, device=dev)
    skip[:, 3::2] = lab[:, 3::2] != lab[:, 1:-2:2]
    d = torch.full((N, S), ninf, dtype=lp.dtype, device=dev)
    d[:, :2] = em[:, 0, :2]
    moves = torch.zeros((T, N, S), dtype=torch.int64, device=dev)
    pad1, pad2 = torch.full((N, 1), ninf, dtype=lp.dtype, device=dev), torch.full((N, 2), ninf, dtype=lp.dtype, device=dev)
    for t in range(1, T):
        d1 = torch.cat([pad1, d[:, :-1]], 1)
        d2 = torch.where(skip, torch.cat([pad2, d[:, :-2]], 1), pad1)
        m1 = d1 > d
        best = torch.where(m1, d1, d)
        m2 = d2 > best
        best = torch.where(m2, d2, best)
        moves[t] = m1.to(torch.int64).masked_fill(m2, 2)
        d = best + em[:, t]
    s = torch.where(d[:, S - 2] > d[:, S - 1], S - 2, S - 1).view(N, 1)
    score = d.gather(1, s).view(N)
    path = torch.empty((N, T), dtype=torch.int64, device=dev)
    for t in range(T - 1, 0, -1):
        path[:, t] = s.view(N)
        s = s - moves[t].gather(1, s)
    path[:, 0] = s.view(N)
    return lab.gather(1, path), score


def device_ms(fn, reps):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.percentile(ms, 50)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench.py measures on the MI355X: no GPU here, nothing measured")
    import ctc_align_ref as R
    from tavsr import ops
    dev = torch.device("cuda", 0)
    lines = ["CTC forced alignment, time per batch (ms): tavsr_ctc_align against the same recursion in torch device ops and the float64 host "
             "reference", "device rows: HIP events around the call, p50 (p10 - p90); host row: wall clock, logits copied to the host first"]
    rec = {"metric": "ctc_align", "unit": "ms per batch (p50)"}
    for N, T, L, V in SHAPES:
        rng = np.random.default_rng(N + T)
        tg = rng.integers(1, V, size=(N, L))
        rep = rng.random((N, L)) < 0.3
        for l in range(1, L):
            tg[:, l] = np.where(rep[:, l], tg[:, l - 1], tg[:, l])
        logits = torch.from_numpy(rng.standard_normal((N, T, V)).astype(np.float32)).to(dev)
        targets = torch.from_numpy(tg).to(dev)
        hlens = torch.full((N,), T, dtype=torch.int64, device=dev)
        tlens = torch.full((N,), L, dtype=torch.int64, device=dev)
        lds = ops.ctc_align_lds_ok(T, L)
        rows = []
        if lds:
            rows.append(("tavsr_ctc_align, moves in LDS", device_ms(lambda: ops.ctc_align(logits, hlens, targets, tlens, route="lds"), args.reps)))
        rows.append(("tavsr_ctc_align, moves in HBM", device_ms(lambda: ops.ctc_align(logits, hlens, targets, tlens, route="ws"), args.reps)))
        rows.append(("torch device ops", device_ms(lambda: torch_align(logits, targets), max(3, args.reps // 5))))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = logits.cpu().numpy()
        want = [R.align_ref(R.log_softmax(host[n]), T, tg[n].tolist()) for n in range(N)]
        host_ms = 1e3 * (time.perf_counter() - t0)
        # the three agree: scores to fp32 accuracy, and the kernel's paths reach the float64 optimum
        al, _, _, sc = ops.ctc_align(logits, hlens, targets, tlens)
        al_t, sc_t = torch_align(logits, targets)
        ref = np.array([w[3] for w in want])
        got = np.array([R.path_score(R.log_softmax(host[n]), al[n].cpu().numpy(), T) for n in range(N)])
        err = max(np.abs(sc.cpu().numpy() - ref).max(), np.abs(sc_t.cpu().numpy() - ref).max(), np.abs(got - ref).max()) / np.abs(ref).max()
        same = int((al.cpu() == al_t.cpu()).all(1).sum())
        lines.append(f"N = {N}, T = {T}, L = {L}, V = {V} (move table {T * ((2 * L + 16) // 16) * 4 / 1024:.1f} KB per problem, "
                     f"{'fits LDS' if lds else 'workspace route only'}); scores agree to {err:.1e}, {same} of {N} paths equal torch's")
        r = rec[f"N{N}_T{T}_L{L}_V{V}"] = {}
        for name, (p50, p10, p90) in rows:
            lines.append(f"  {name:<32} {p50:10.3f}  ({p10:.3f} - {p90:.3f})")
            r[name] = round(p50, 3)
        lines.append(f"  {'float64 host reference':<32} {host_ms:10.3f}")
        r["float64 host reference"] = round(host_ms, 3)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
