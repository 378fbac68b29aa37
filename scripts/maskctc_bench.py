"""Mask-CTC decoding on the BASELINE config-5 model shape (tailored AV-Branchformer 12L, 4 s utterances: 400 mel frames + 100
lip frames 88 x 88, random-init weights) with an MLM decoder of the attention decoder's depth (6 layers), K = 10.

Per batch size (1 and 64): time per utterance (p50 / p10 / p90 over the timed batches, host clock around a device synchronise) of
  (a) encode            - the captured encoder (``CapturedEncode``, as ``Speech2TextMaskCTC`` runs it)
  (b) init              - CTC head + ``maskctc_init`` + the one host read (lengths, largest num_iter)
  (c) the loop          - eager / captured, each with and without the hoisted source-attention projections
                          (``prepare_memory`` is inside the timed region of the hoisted variants)
and, in the same process after the Mask-CTC measurements, the existing beam-10 search WITHOUT a language model on the same encoder
output (an attention model's CTC head and decoder, random-init) for scale: the two decode different model families.
The threshold is set as in the decoding fixtures: the middle of the widest gap between neighbouring token probabilities around
their median over the warm-up batch, so about half the positions start masked.
Protocol of bench_decode.py: inputs resident in HBM before the clock starts, a warm-up at the timed batch size, captured graphs
exist when the clock starts (one per (B, L, passes); their capture cost is reported separately).  Also reported: the device time of
one ``maskctc_step`` launch (200 launches captured into one graph, device events around a replay) as a share of one pass of the loop.

    python scripts/maskctc_bench.py [--out profiles/maskctc_bench.txt] [--reps1 32] [--reps64 8]
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

from bench_decode import DUR_S, make_conf, make_utts  # noqa: E402

K = 10


def build(dev):
    from tavsr.inference.beam_search import BatchBeamSearch, CapturedEncode
    from tavsr.models.maskctc_model import MaskCTCInference
    from tavsr.tasks.avsr import AVSRTask
    from tavsr.utils.tokens import CHAR_ENGLISH
    conf = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "avsr_tailored_maskctc_english.yaml")))
    conf.update(acoustic_input_size=80, visual_input_size=None, specaug=None, token_list=list(CHAR_ENGLISH))
    torch.manual_seed(1)
    model = AVSRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).eval().to(dev)
    torch.manual_seed(1)
    att = AVSRTask.build_model(argparse.Namespace(**copy.deepcopy(make_conf()))).eval().to(dev)      # for the beam search beside it
    search = BatchBeamSearch(att, None, beam_size=10, ctc_weight=0.1, lm_weight=0.0, penalty=0.5)
    return model, MaskCTCInference(model, K, 0.99), CapturedEncode(model), search


def median_gap_threshold(inf, enc, olens):
    inf.threshold_probability = 0.0
    _, _, prob, y_len, _ = inf.start(enc, olens)
    p = np.sort(np.concatenate([prob[b, : int(y_len[b])].cpu().numpy() for b in range(enc.shape[0])]).astype(np.float64))
    band = p[int(0.4 * len(p)): max(int(0.6 * len(p)), int(0.4 * len(p)) + 2)]
    i = int(np.argmax(np.diff(band)))
    return float((band[i] + band[i + 1]) / 2)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class Loop:
    """the four variants of the loop on one start state (y0, y_len, plan, passes)"""

    def __init__(self, inf):
        self.inf, self.graphs, self.capture_s = inf, {}, []

    def start(self, enc, olens):
        y_in, _, _, y_len, plan = self.inf.start(enc, olens)
        B = enc.shape[0]
        host = torch.cat([y_len, plan[:, 1].to(torch.int64), plan[:, 0].to(torch.int64)]).tolist()      # the one host read
        L, passes = max(max(host[:B]), 1), max(host[B: 2 * B])
        return y_in[:, :L].contiguous(), y_len, plan, passes, sum(host[:B]), sum(host[2 * B:])

    def eager(self, enc, olens, y0, y_len, plan, passes, hoist):
        kv = self.inf.mlm.prepare_memory(enc, olens) if hoist else None
        return self.inf.passes(enc, olens, y0.clone(), y_len.clamp(min=1), y_len, plan, passes, memory_kv=kv)

    def captured(self, enc, olens, y0, y_len, plan, passes, hoist):
        key = (tuple(enc.shape), y0.shape[1], passes, hoist)
        g = self.graphs.get(key)
        if g is None:
            t0 = time.perf_counter()
            st = dict(enc=enc.clone(), olens=olens.clone(), y=y0.clone(), y_len=y_len.clone(), plan=plan.clone())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.eager(st["enc"], st["olens"], st["y"], st["y_len"], st["plan"], passes, hoist)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                dec_lens = st["y_len"].clamp(min=1)
                kv = self.inf.mlm.prepare_memory(st["enc"], st["olens"]) if hoist else None
                self.inf.passes(st["enc"], st["olens"], st["y"], dec_lens, st["y_len"], st["plan"], passes, memory_kv=kv)
            torch.cuda.synchronize()
            self.capture_s.append(time.perf_counter() - t0)
            g = self.graphs[key] = (graph, st)
        graph, st = g
        for k, v in (("enc", enc), ("olens", olens), ("y", y0), ("y_len", y_len), ("plan", plan)):
            st[k].copy_(v)
        graph.replay()
        return st["y"]


def step_kernel_us(inf, enc, olens, y0, y_len, plan, n=200):
    """device time of one ``maskctc_step`` launch: n launches captured into one graph (no host enqueue between them), device events
    around a replay.  Pass 0 on the same start state every time (the selection runs, ``y`` is restored by the replay's first node)."""
    from tavsr import ops
    logits, _ = inf.mlm(enc, olens, y0, y_len.clamp(min=1))
    y = y0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.maskctc_step(logits, y, y_len, plan, 0, inf.mask_token)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            y.copy_(y0)
            ops.maskctc_step(logits, y, y_len, plan, 0, inf.mask_token)
    copies = torch.cuda.CUDAGraph()
    with torch.cuda.graph(copies):
        for _ in range(n):
            y.copy_(y0)
    out = []
    for g in (graph, copies):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            ts.append(1e3 * a.elapsed_time(b) / n)
        out.append(float(np.median(ts)))
    return max(out[0] - out[1], 0.0)        # (the restoring copy's own node subtracted)


def pct(xs, B):
    x = 1e3 * np.array(xs) / B
    return "%9.3f %9.3f %9.3f" % tuple(np.percentile(x, q) for q in (50, 10, 90))


def measure(dev, model, inf, encode, search, B, reps, lines, rec):
    loop = Loop(inf)
    with torch.no_grad():
        warm = make_utts(B, 7, dev)
        for _ in range(max(1, 8 // B)):
            enc, olens = encode(*warm)
        enc, olens = enc.clone(), olens.clone()
        if rec.get("threshold") is None:
            rec["threshold"] = median_gap_threshold(inf, enc, olens)
        inf.threshold_probability = rec["threshold"]
        data = [make_utts(B, 1234 + i, dev) for i in range(reps)]
        variants = [("eager", False), ("eager", True), ("captured", False), ("captured", True)]
        T = {k: [] for k in ["encode", "init"] + [f"{m}{'+hoist' if h else ''}" for m, h in variants] + ["beam10"]}
        tokens = masked = passes_total = 0
        encs, per_pass_us = [], []
        for rnd in ("warm", "timed"):
            for batch in ([warm] if rnd == "warm" else []) + data:      # (the warm round also captures the graphs the timed round replays)
                t_enc, (e, ol) = clock(lambda: encode(*batch))
                e, ol = e.clone(), ol.clone().to(torch.int64)
                t_init, (y0, y_len, plan, passes, ntok, nmask) = clock(lambda: loop.start(e, ol))
                outs = []
                for mode, hoist in variants:
                    fn = loop.eager if mode == "eager" else loop.captured
                    t, y = clock(lambda: fn(e, ol, y0, y_len, plan, passes, hoist))
                    outs.append(y.clone())
                    if rnd == "timed":
                        T[f"{mode}{'+hoist' if hoist else ''}"].append(t)
                        if mode == "captured" and hoist and passes:
                            per_pass_us.append(1e6 * t / passes)
                assert all(torch.equal(outs[0], o) for o in outs[1:]), "the four variants of the loop disagree"
                if rnd == "timed":
                    T["encode"].append(t_enc)
                    T["init"].append(t_init)
                    tokens, masked, passes_total = tokens + ntok, masked + nmask, passes_total + passes
                    encs.append((e, ol))
        step_us = step_kernel_us(inf, e, ol, y0, y_len, plan)
        pass_us = float(np.median(per_pass_us))
        for e, ol in [encs[0]] + encs:                      # the beam search last, on the same encoder outputs (first one: warm-up)
            t, _ = clock(lambda: search.decode(e, ol, nbest=1))
            T["beam10"].append(t)
        T["beam10"] = T["beam10"][1:]
    n = reps * B
    lines.append(f"batch {B}: {reps} timed batches, {tokens / n:.1f} tokens / utterance, {masked / n:.1f} masked, "
                 f"{passes_total / reps:.1f} passes / batch, threshold {rec['threshold']:.6f}")
    lines.append(f"  {'ms per utterance':<22} {'p50':>9} {'p10':>9} {'p90':>9}")
    for k, v in T.items():
        lines.append(f"  {k:<22} {pct(v, B)}")
    cap = loop.capture_s
    lines.append(f"  graphs captured: {len(cap)} (one per (B, L, passes, hoist)), {1e3 * float(np.mean(cap)):.1f} ms each incl. warm-up run")
    lines.append(f"  maskctc_step: {step_us:.1f} us per launch inside a replayed graph = {100 * step_us / pass_us:.1f} % of a captured+hoist pass "
                 f"({pass_us:.0f} us)")
    rec[f"batch{B}"] = {k: round(1e3 * float(np.median(v)) / B, 4) for k, v in T.items()}
    rec[f"batch{B}"].update(step_us=round(step_us, 2), pass_us=round(pass_us, 1), tokens_per_utt=round(tokens / n, 1),
                            masked_per_utt=round(masked / n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps1", type=int, default=32)
    ap.add_argument("--reps64", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskctc_bench.py measures on the MI355X: no GPU here, nothing measured")
    dev = torch.device("cuda", 0)
    model, inf, encode, search = build(dev)
    lines = ["Mask-CTC decode, tailored AV-Branchformer 12L + 6L MLM decoder, 4 s utterances (T = 99 encoder frames), K = 10, f32, "
             "random-init weights; beam10 = the attention model's beam-10 search without LM on the same encoder output",
             f"utterance length {DUR_S} s; all times host clock around a device synchronise"]
    rec = {"metric": "maskctc_decode", "unit": "ms per utterance (p50)", "threshold": None}
    for B, reps in ((1, args.reps1), (64, args.reps64)):
        measure(dev, model, inf, encode, search, B, reps, lines, rec)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
