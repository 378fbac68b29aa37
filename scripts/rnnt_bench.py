"""Transducer: step time and peak memory of joint + RNN-T loss, forward + backward (functional_rnnt.RNNTLossFn: the lattice rows go
through in bounded chunks) beside the same computation with the joint tensor [B, T, U+1, V] materialised by torch device ops
(tanh of the broadcast sum, the output Linear, log_softmax, the lattice as T steps of logcumsumexp, autograd backward) - what a
user would write without the kernels, and what warp-transducer's interface requires.  B = 32, T = 100, U = 40, J = 256, encoder
256 and decoder 320 wide, at V = 41 and V = 5000; every utterance has all T frames and all U labels.  Also: one LSTM layer
forward + backward at B = 32, L = 41, I = H = 320 (ops.lstm_fwd + ops.lstm_bwd) beside torch.nn.LSTM on the device, and the greedy
search's time per encoder frame (inference/transducer.py, a replayed graph per frame) at B = 1 and B = 32, T = 100, V = 41.
Times: HIP events around the call (allocations included), p50 (p10 - p90) over the timed repetitions after two warm-up calls;
peak memory: torch.cuda.max_memory_allocated over one call, above what was allocated before it.  Records, not thresholds.

    python scripts/rnnt_bench.py [--out profiles/rnnt_bench.txt] [--reps 10]
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

B, T, U, J, DE, DD = 32, 100, 40, 256, 256, 320


def torch_joint_loss(enc, dec, target, P, blank=0):
    """the materialised form, full-length utterances: -> sum_b nll[b] / B"""
    w_enc, b_enc, w_dec, w_out, b_out = P
    F = torch.nn.functional
    z = torch.tanh(F.linear(enc, w_enc, b_enc)[:, :, None, :] + F.linear(dec, w_dec)[:, None, :, :])
    lp = F.linear(z, w_out, b_out).log_softmax(-1)                       # [B, T, U+1, V]
    lpb = lp[..., blank]
    lpl = lp[:, :, :-1].gather(3, target.long()[:, None, :, None].expand(-1, lp.shape[1], -1, 1))[..., 0]      # [B, T, U]
    zero = lpb.new_zeros(lpb.shape[0], 1)
    c = torch.cat([zero[:, None].expand(-1, lpb.shape[1], -1), lpl.cumsum(2)], 2)      # c[t][u] = sum_{j < u} lpl[t][j]
    alpha = c[:, 0]
    for t in range(1, lpb.shape[1]):
        alpha = c[:, t] + torch.logcumsumexp(alpha + lpb[:, t - 1] - c[:, t], 1)
    return -(alpha[:, -1] + lpb[:, -1, -1]).sum() / lpb.shape[0]


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_bench.py measures on the MI355X: no GPU here, nothing measured")
    from tavsr import ops
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    from tavsr.functional_rnnt import RNNTLossFn
    from tavsr.inference.transducer import BeamSearchTransducer
    dev = torch.device("cuda", 0)
    lines = [f"Transducer, B = {B}, T = {T}, U = {U}, J = {J} (encoder {DE}, decoder {DD} wide), fp32; ms per call: p50 (p10 - p90), HIP events",
             "joint + RNN-T loss, forward + backward: RNNTLossFn (lattice rows in chunks) | the joint tensor materialised by torch device ops"]
    rec = {"metric": "rnnt", "unit": "ms per call (p50) / MB peak"}
    t_len = torch.full((B,), T, dtype=torch.int64, device=dev)
    u_len = torch.full((B,), U, dtype=torch.int64, device=dev)
    for V in (41, 5000):
        torch.manual_seed(V)
        leaves = [torch.randn(B, T, DE, device=dev), torch.randn(B, U + 1, DD, device=dev), torch.randn(J, DE, device=dev) / 16,
                  torch.randn(J, device=dev) / 4, torch.randn(J, DD, device=dev) / 18, torch.randn(V, J, device=dev) / 8, torch.randn(V, device=dev) / 2]
        for t in leaves:
            t.requires_grad_(True)
        target = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
        out = {}

        def ours():
            for t in leaves:
                t.grad = None
            loss = RNNTLossFn.apply(leaves[0], leaves[1], t_len, u_len, target, dict(blank=0), *leaves[2:])
            loss.backward()
            out["ours"] = (loss.detach(), leaves[0].grad)

        def mat():
            for t in leaves:
                t.grad = None
            loss = torch_joint_loss(leaves[0], leaves[1], target, leaves[2:])
            loss.backward()
            out["torch"] = (loss.detach(), leaves[0].grad)

        rows = B * T * (U + 1)
        chunk = ops.rnnt_chunk(V, rows)
        r = rec[f"V{V}"] = {}
        for name, fn, reps in (("RNNTLossFn", ours, args.reps), ("torch, materialised", mat, max(3, args.reps // 2))):
            p50, p10, p90 = device_ms(fn, reps)
            mb = peak_mb(fn)
            r[name] = {"ms": round(p50, 3), "peak_mb": round(mb, 1)}
            lines.append(f"  V = {V:<5} {name:<22} {p50:10.3f}  ({p10:.3f} - {p90:.3f})   peak {mb:9.1f} MB")
        lo, lt = float(out["ours"][0]), float(out["torch"][0])
        ge = float((out["ours"][1] - out["torch"][1]).norm() / out["torch"][1].norm())
        lines.append(f"            {rows} lattice rows in chunks of {chunk} ({-(-rows // chunk)} chunks); joint tensor {rows * V * 4 / 2**20:.0f} MB; "
                     f"loss {lo:.4f} | {lt:.4f}, d loss / d enc differs by {ge:.1e} (relative L2)")
    # ---- LSTM layer
    Ln, H = U + 1, DD
    torch.manual_seed(1)
    x = torch.randn(B, Ln, H, device=dev)
    dy = torch.randn(B, Ln, H, device=dev)
    m = torch.nn.LSTM(H, H, 1, batch_first=True)
    P = [p.detach().to(dev).contiguous() for p in (m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0)]

    def lstm_ours():
        y, _, _, sv = ops.lstm_fwd(x, *P)
        ops.lstm_bwd(dy, sv, P[0], P[1])

    p50, p10, p90 = device_ms(lstm_ours, args.reps)
    lines.append(f"one LSTM layer, forward + backward, B = {B}, L = {Ln}, I = H = {H} ({ops.lstm_rows_per_wg()} rows per workgroup: "
                 f"{-(-B // ops.lstm_rows_per_wg())} workgroups)")
    lines.append(f"  {'ops.lstm_fwd + ops.lstm_bwd':<30} {p50:10.3f}  ({p10:.3f} - {p90:.3f})")
    rec["lstm"] = {"ops": round(p50, 3)}
    try:
        md = m.to(dev)
        xr = x.clone().requires_grad_(True)

        def lstm_torch():
            for p in md.parameters():
                p.grad = None
            xr.grad = None
            md(xr)[0].backward(dy)

        p50, p10, p90 = device_ms(lstm_torch, args.reps)
        lines.append(f"  {'torch.nn.LSTM on the device':<30} {p50:10.3f}  ({p10:.3f} - {p90:.3f})")
        rec["lstm"]["torch"] = round(p50, 3)
    except Exception as e:      # the vendor library's RNN may be missing on a box: a record, not a requirement
        lines.append(f"  torch.nn.LSTM on the device: not measured ({type(e).__name__})")
    # ---- greedy search
    torch.manual_seed(2)
    dec, jn = TransducerDecoder(41, hidden_size=DD).to(dev).eval(), JointNetwork(41, DE, DD, joint_space_size=J).to(dev).eval()
    search = BeamSearchTransducer(dec, jn, beam_size=1)
    lines.append(f"greedy search (a replayed graph per encoder frame), T = {T}, V = 41: wall clock per decode call / {T} frames, best of 5 "
                 "(capture included)")
    for nb in (1, 32):
        enc = torch.randn(nb, T, DE, device=dev)
        lens = torch.full((nb,), T, dtype=torch.int64, device=dev)
        best = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hyps = search.decode(enc, lens)
            dt = 1e3 * (time.perf_counter() - t0)
            best = dt if best is None else min(best, dt)
        n_tok = sum(len(h[0][0]) - 1 for h in hyps)
        lines.append(f"  B = {nb:<3} {best:9.3f} ms per utterance batch, {1e3 * best / T:8.1f} us per frame ({n_tok} tokens emitted)")
        rec[f"greedy_B{nb}"] = {"ms": round(best, 3), "us_per_frame": round(1e3 * best / T, 1)}
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
