"""Transducer beam searches: time per step and per utterance of ALSD (a step = one value of i) and TSD (a step = one frame with its
max_sym_exp = 2 expansions) beside the greedy search on the same inputs (inference/transducer.py), at B = 1 and B = 32, T = 100,
V = 41 and V = 5000, beam 10, every utterance with all T frames.  Decoder 320 wide (one layer), encoder 256, joint space 256 - the
transducer recipe's sizes; random weights with lin_out scaled by 2 and 4.5 added to the blank bias (an untrained joint makes ALSD
emit a label at every step: tests/test_gpu_rnnt_search.py).  Both routes are timed: the step replayed as a graph (the first call
of a shape captures it and is not timed) and the same launches issued eagerly.  Wall clock around ``decode`` ending in the host
read of the results, best and median of the repetitions.  Records, not thresholds.

    python scripts/rnnt_search_bench.py [--out profiles/rnnt_search_bench.txt] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tailored-avsr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

T, K, DE, DD, J, U_MAX, M = 100, 10, 256, 320, 256, 50, 2


def timed(fn, reps):
    fn()                                                    # warm-up (and, on the graph route, the capture)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_search_bench.py measures on the MI355X: no GPU here, nothing measured")
    from tavsr.decoder.joint_network import JointNetwork
    from tavsr.decoder.transducer_decoder import TransducerDecoder
    from tavsr.inference.transducer import BeamSearchTransducer
    dev = torch.device("cuda", 0)
    lines = [f"Transducer searches on {torch.cuda.get_device_name(0)}, T = {T}, beam {K}, u_max {U_MAX}, max_sym_exp {M}, decoder {DD} x 1 layer, "
             f"encoder {DE}, joint {J}, fp32",
             "wall clock per decode call (host read of the results included): best / median ms; us per step = best / steps; "
             "ms per utterance = best / B",
             f"steps: greedy {T} frames, ALSD {T + min(U_MAX, T - 1)} values of i, TSD {T} frames of {M} expansions"]
    rec = {"metric": "rnnt_search", "unit": "us per step (best)"}
    for V in (41, 5000):
        torch.manual_seed(V)
        dec, jn = TransducerDecoder(V, hidden_size=DD).to(dev).eval(), JointNetwork(V, DE, DD, joint_space_size=J).to(dev).eval()
        with torch.no_grad():
            jn.lin_out.weight *= 2.0
            jn.lin_out.bias[0] += 4.5
        for nb in (1, 32):
            enc = torch.randn(nb, T, DE, device=dev) * 3.0
            lens = torch.full((nb,), T, dtype=torch.int64, device=dev)
            lines.append(f"V = {V}, B = {nb}")
            for name, kw, steps in (("greedy", dict(beam_size=1), T), ("alsd", dict(beam_size=K, search_type="alsd", u_max=U_MAX), T + min(U_MAX, T - 1)),
                                    ("tsd", dict(beam_size=K, search_type="tsd", max_sym_exp=M), T)):
                for route in ("graph", "eager"):
                    search = BeamSearchTransducer(dec, jn, use_graph=route == "graph", **kw)
                    best, med, out = timed(lambda: search.decode(enc, lens), args.reps)
                    labels = sum(len(h[0][0]) - 1 for h in out)
                    lines.append(f"  {name:<7} {route:<6} {best:9.3f} / {med:9.3f} ms   {1e3 * best / steps:8.1f} us per step   "
                                 f"{best / nb:8.3f} ms per utterance   ({labels} labels in the best hypotheses)")
                    rec[f"V{V}_B{nb}_{name}_{route}"] = round(1e3 * best / steps, 1)
    lines.append("(the greedy search captures its graph in every call; ALSD and TSD keep theirs across calls of a shape)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
