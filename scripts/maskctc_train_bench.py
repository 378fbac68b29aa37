"""Mask-CTC training step, host-drawn against device-drawn masks: the 12-layer audio-only Mask-CTC recipe
(configs/asr_branchformer_maskctc_english.yaml: Branchformer 12L + Conv2dSubsampling + CTC + 6L MLM decoder, recipe dropout,
random-init weights) at bench.py's audio-only batch (32 x 400 mel frames x 80, 40 tokens), forward + backward, in one process.

Legs, run interleaved block by block so that clock drift and neighbours on the machine hit all of them alike:
  eager / host draw       ``mask_draw = "host"``: numpy draw, one ``text.tolist()`` per step (a device synchronisation behind the
                          enqueued encoder)
  eager / device draw     ``mask_draw = "device"``: ``ops.mask_uniform``, no host read in the step
  captured / device draw  the same step as one replayed graph (new masks at every replay)
A block is ``--steps`` steps enqueued back to back with one synchronisation at its end: the host is free to run ahead across
step boundaries where the step lets it, which is what the removed read is about - a clock around every single step would hide it.
Reported per leg: p50 and the p10 - p90 band of the time per step over ``--blocks`` blocks (host clock).

    python scripts/maskctc_train_bench.py [--out profiles/maskctc_train_bench.txt] [--blocks 20] [--steps 8]
"""
import argparse
import copy
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
import yaml  # noqa: E402

B, T_IN, N_MEL, L_TXT = 32, 400, 80, 40      # bench.py's audio-only batch


def build(dev):
    from tavsr.tasks.asr import ASRTask
    from tavsr.utils.tokens import CHAR_ENGLISH
    conf = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_maskctc_english.yaml")))
    conf.update(input_size=N_MEL, specaug=None, token_list=list(CHAR_ENGLISH))
    torch.manual_seed(0)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).to(dev).train()
    g = torch.Generator().manual_seed(1234)
    speech = torch.randn(B, T_IN, N_MEL, generator=g)
    text = torch.randint(1, 40, (B, L_TXT), generator=g)
    batch = [t.to(dev) for t in (speech, torch.full((B,), T_IN, dtype=torch.int64), text, torch.full((B,), L_TXT, dtype=torch.int64))]
    return model, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskctc_train_bench.py measures on the MI355X: no GPU here, nothing measured")
    from tavsr import ops
    dev = torch.device("cuda", 0)
    model, batch = build(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    np.random.seed(0)
    ops.manual_seed(0)

    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(*batch)[0]
        loss.backward()
        return loss

    def eager(draw):
        def step():
            model.mask_draw = draw
            fwd_bwd()
        return step

    for draw in ("host", "device"):
        for _ in range(3):
            eager(draw)()
    model.mask_draw = "device"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = fwd_bwd()
    legs = [("eager / host draw", eager("host")), ("eager / device draw", eager("device")), ("captured / device draw", graph.replay)]

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    for _, fn in legs:
        block(fn)
    T = {name: [] for name, _ in legs}
    seen = set()
    for _ in range(args.blocks):
        for name, fn in legs:
            T[name].append(block(fn))
        seen.add(float(static_loss))
    assert len(seen) > 1 and all(np.isfinite(x) for x in seen), "the captured step does not draw new masks per replay"
    lines = [f"Mask-CTC training step (fwd + bwd), audio-only Branchformer 12L + 6L MLM decoder, batch {B} x {T_IN} mel frames x {N_MEL}, "
             f"{L_TXT} tokens, f32, recipe dropout, random-init weights",
             f"{args.blocks} blocks per leg, interleaved; a block = {args.steps} steps back to back, one synchronisation at its end; host clock",
             f"  {'ms per step':<26} {'p50':>9} {'p10':>9} {'p90':>9} {'utt/s (p50)':>13}"]
    rec = {"metric": "maskctc_train_step", "unit": "ms per step", "blocks": args.blocks, "steps_per_block": args.steps}
    for name, _ in legs:
        x = 1e3 * np.array(T[name])
        p50, p10, p90 = (float(np.percentile(x, q)) for q in (50, 10, 90))
        lines.append(f"  {name:<26} {p50:9.3f} {p10:9.3f} {p90:9.3f} {1e3 * B / p50:13.1f}")
        rec[name] = {"p50": round(p50, 3), "p10": round(p10, 3), "p90": round(p90, 3)}
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
