"""What the time-synchronous search (Speech2Text(time_sync=True), tavsr/inference/timesync.py) costs, beside the label-synchronous
search on the same model and the same encoder outputs, and beside the CPU restatement of espnet's BeamSearchTimeSync.

Model of BASELINE config 5 (tailored AV-Branchformer 12L + 6L decoder + 16 x 512 Transformer LM, random-init weights), 4 s utterances
(~100 encoder frames), V = 41, beam 10, ctc_weight 0.1, lm_weight 0.6, length bonus 0.5.  Time-synchronous: without scorers (the
one-launch route; ctc_weight 1.0), with the decoder, with decoder and LM.  Label-synchronous: decoder, decoder + LM.  Batch 1 and 64.
The searches alternate inside one process, round by round, on the same encoder outputs (resident in HBM); one warm-up round at the
timed batch size (captures every graph); host clock around a device synchronise per decode() call; median and p10 .. p90.
A time-synchronous search does one step per FRAME, a label-synchronous one one step per TOKEN: both are given per utterance
and per step.  Then, eagerly and outside the timing, how many slots are new per frame - what a scorer pass that skipped frames
without a new node could save.  The CPU restatement (tests/timesync_ref.py, fp64 Python, one utterance, CTC term alone) is timed on
the same posteriors; with scorers it would call a Python decoder per new prefix and is not timed.

    python scripts/timesync_bench.py [--out profiles/timesync_bench.txt] [--reps1 12] [--reps64 5]
"""
import argparse
import copy
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

from bench_decode import DUR_S, LM_CONF, SEARCH, make_conf, make_utts  # noqa: E402


def build(dev):
    from tavsr.inference.beam_search import BatchBeamSearch, CapturedEncode
    from tavsr.inference.timesync import BeamSearchTimeSync
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.avsr import AVSRTask
    conf = make_conf()
    torch.manual_seed(1)
    model = AVSRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).eval().to(dev)
    lm = TransformerLM(len(conf["token_list"]), **LM_CONF).eval().to(dev)
    K, w, wl, pen = SEARCH["beam_size"], SEARCH["ctc_weight"], SEARCH["lm_weight"], SEARCH["penalty"]

    def routes():
        return [("time-sync, CTC alone (one launch)", BeamSearchTimeSync(model, None, K, 1.0, 0.0, pen)),
                ("time-sync, decoder", BeamSearchTimeSync(model, None, K, w, 0.0, pen)),
                ("time-sync, decoder + LM", BeamSearchTimeSync(model, lm, K, w, wl, pen)),
                ("label-sync, decoder", BatchBeamSearch(model, None, K, w, 0.0, pen)),
                ("label-sync, decoder + LM", BatchBeamSearch(model, lm, K, w, wl, pen))]
    return model, CapturedEncode(model), routes


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def steps_of(search, enc_lens):
    n = getattr(search, "n_steps", None)
    return max(n) if n else int(enc_lens.max())      # label-synchronous: tokens searched; time-synchronous: frames


def measure(encode, routes, B, reps, dev, lines, rec):
    with torch.no_grad():
        encs = []
        for i in range(reps + 1):                                  # batch 0: warm-up round
            e, ol = encode(*make_utts(B, 1234 + i, dev))
            e = e[0] if isinstance(e, tuple) else e
            encs.append((e.clone(), ol.clone().to(torch.int64)))
        T = {name: [] for name, _ in routes}
        steps = {name: [] for name, _ in routes}
        for rnd, (e, ol) in enumerate(encs):
            for name, search in routes:
                t, _ = clock(lambda: search.decode(e, ol, nbest=1))
                if rnd > 0:
                    T[name].append(t)
                    steps[name].append(steps_of(search, ol))
    lines.append(f"batch {B}: {reps} timed rounds, {encs[0][0].shape[1]} frames")
    lines.append(f"  {'search':<36} {'ms / decode p50':>16} {'p10':>9} {'p90':>9} {'ms / utterance':>15} {'steps':>7} {'us / step':>10} {'p10':>9} {'p90':>9}")
    r = rec[f"batch{B}"] = {}
    for name, _ in routes:
        ms = 1e3 * np.array(T[name])
        st = float(np.mean(steps[name]))
        per = 1e6 * np.array(T[name]) / np.array(steps[name])
        p50, p10, p90 = (float(np.percentile(ms, q)) for q in (50, 10, 90))
        u50, u10, u90 = (float(np.percentile(per, q)) for q in (50, 10, 90))
        lines.append(f"  {name:<36} {p50:16.3f} {p10:9.3f} {p90:9.3f} {p50 / B:15.3f} {st:7.1f} {u50:10.1f} {u10:9.1f} {u90:9.1f}")
        r[name] = dict(ms_per_decode=round(p50, 3), ms_per_decode_p10=round(p10, 3), ms_per_decode_p90=round(p90, 3),
                       ms_per_utterance=round(p50 / B, 3), steps=round(st, 1), us_per_step=round(u50, 1))
    return encs[-1]


def new_slots_per_frame(search, enc, lens, lines, rec, B):
    """eager frames with a host read of the new-slot counts behind each (a diagnostic: not the product path, not timed)"""
    from tavsr.inference import timesync as TS
    old = TS.GRAPH_STEP
    counts = []
    orig = TS.TimeSyncSearch._frame

    def counting(self, b):
        orig(self, b)
        counts.append(b.rows.nkeys.view(enc.shape[0], -1).gt(0).sum(dim=1).cpu())

    TS.GRAPH_STEP, TS.TimeSyncSearch._frame = False, counting
    try:
        with torch.no_grad():
            search.decode(enc, lens, nbest=1)
    finally:
        TS.GRAPH_STEP, TS.TimeSyncSearch._frame = old, orig
    c = torch.stack(counts).float()                               # [frames, U]
    none_utt = float((c == 0).float().mean())
    none_batch = float((c.sum(dim=1) == 0).float().mean())
    lines.append(f"  new slots per frame and utterance (beam {search.K}), batch {B}: mean {float(c.mean()):.2f}, frames of an utterance without a new "
                 f"slot {100 * none_utt:.1f} %, frames where NO utterance of the batch has one {100 * none_batch:.1f} %")
    rec[f"new_slots_batch{B}"] = dict(mean=round(float(c.mean()), 2), frames_without_new_per_utterance=round(none_utt, 3),
                                      frames_without_new_in_batch=round(none_batch, 3))


def kernels_alone(model, enc, lens, lines, rec, K, pen, B):
    """the bookkeeping kernels without scorers, device events around back-to-back launches: the one-launch search (init + search),
    and one frame of the stepped form (NULL scorer operands, the frame counter parked on frame 10)"""
    from tavsr import ops
    ctc = model.ctc
    U, T, _ = enc.shape
    z = ops.linear(enc.reshape(U * T, -1).contiguous(), ctc.ctc_lo.weight, ctc.ctc_lo.bias)
    lpz = ops.log_softmax_rows(z).view(U, T, -1)
    V, C = lpz.shape[2], int(1.5 * K)
    words, _ = ops.timesync_ws(K, V, T, C)
    ws = torch.zeros(U, words, dtype=torch.int32, device=enc.device)
    frame = torch.zeros(1, dtype=torch.int32, device=enc.device)
    lens = lens.to(torch.int64)

    def timed(fn, n):
        us = []
        for _ in range(6):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                fn()
            t1.record()
            torch.cuda.synchronize()
            us.append(1e3 * t0.elapsed_time(t1) / n)
        return float(np.median(us[1:]))

    def whole():
        ops.timesync_init(ws, U, K, V, T, C, model.sos, frame_dev=frame)
        ops.timesync_search(lpz, lens, ws, K, C, model.sos, 1.0, pen)

    t_search = timed(whole, 10)
    ops.timesync_init(ws, U, K, V, T, C, model.sos, frame_dev=frame)
    for _ in range(10):
        ops.timesync_step(lpz, lens, ws, frame, K, C, model.sos, 1.0, 0.0, 0.0, pen)
        frame.add_(1)
    t_step = timed(lambda: ops.timesync_step(lpz, lens, ws, frame, K, C, model.sos, 1.0, 0.0, 0.0, pen), 100)
    lines.append(f"  kernels alone, batch {B} (device events, back-to-back, median of 5): tavsr_timesync_init + tavsr_timesync_search {t_search:.1f} us "
                 f"per search = {t_search / T:.2f} us per frame; tavsr_timesync_step {t_step:.2f} us per launch (one frame, state through device memory)")
    rec[f"kernel_search_us_batch{B}"], rec[f"kernel_step_us_batch{B}"] = round(t_search, 1), round(t_step, 2)


def cpu_restatement(model, enc, lens, lines, rec, K, pen):
    from timesync_ref import timesync_search
    ctc = model.ctc
    with torch.no_grad():
        z = torch.nn.functional.linear(enc[0, : int(lens[0])], ctc.ctc_lo.weight, ctc.ctc_lo.bias)
        lpz = torch.log_softmax(z.double(), dim=-1).cpu().numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        timesync_search(lpz, K, model.sos, w_ctc=1.0, pen=pen)
        ts.append(time.perf_counter() - t0)
    lines.append(f"  CPU restatement (tests/timesync_ref.py, fp64 Python, CTC term alone, one utterance of {lpz.shape[0]} frames): "
                 f"{1e3 * float(np.median(ts)):.1f} ms per utterance, {1e6 * float(np.median(ts)) / lpz.shape[0]:.0f} us per frame (median of 3)")
    rec["cpu_restatement_ms"] = round(1e3 * float(np.median(ts)), 1)


def reading(rec):
    """what the table says about a scorer pass that skipped the frames without a new node - arithmetic on the figures above"""
    out = ["reading: should the scorer pass be skipped on frames without a new node?"]
    for B in (1, 64):
        r, ns = rec[f"batch{B}"], rec[f"new_slots_batch{B}"]
        step, full = rec[f"kernel_step_us_batch{B}"], r["time-sync, decoder + LM"]["us_per_step"]
        idle = ns["frames_without_new_in_batch"]
        out.append(f"  batch {B}: a frame costs {full:.0f} us with decoder + LM, of which the bookkeeping launch is {step:.0f} us; no utterance of the batch has a "
                   f"new slot in {100 * idle:.1f} % of the frames -> at most {idle * (full - step):.0f} us per frame ({100 * idle * (full - step) / full:.0f} %) "
                   "to be had by skipping")
    out.append("  The pass has a fixed launch shape and is bound by its chain of dependent small launches, not by its rows: rows without work are free, a")
    out.append("  launch that returns at once still costs its place in the chain.  Skipping therefore needs the HOST to know that a frame has no new slot -")
    out.append("  a device-to-host read and a second graph per frame, i.e. the host back inside the frame loop.  At batch 64 there is nothing to skip (every")
    out.append("  frame has a new slot somewhere in the batch).  At batch 1 most frames are idle and a host-checked skip would pay; it is NOT done here: the")
    out.append("  search keeps one host read in front of the frame loop and one behind it.")
    out.append("cost relative to the label-synchronous search (ms per decode, p50; a pair whose p10 .. p90 ranges overlap is no measurable difference):")
    for B in (1, 64):
        for what in ("decoder", "decoder + LM"):
            t, l = rec[f"batch{B}"][f"time-sync, {what}"], rec[f"batch{B}"][f"label-sync, {what}"]
            overlap = t["ms_per_decode_p10"] <= l["ms_per_decode_p90"] and l["ms_per_decode_p10"] <= t["ms_per_decode_p90"]
            verdict = "no measurable difference" if overlap else f"{t['ms_per_decode'] / l['ms_per_decode']:.2f}x"
            out.append(f"  batch {B}, {what}: time-sync {t['ms_per_decode']:.1f} ({t['ms_per_decode_p10']:.1f} .. {t['ms_per_decode_p90']:.1f}), "
                       f"label-sync {l['ms_per_decode']:.1f} ({l['ms_per_decode_p10']:.1f} .. {l['ms_per_decode_p90']:.1f}): {verdict}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps1", type=int, default=12)
    ap.add_argument("--reps64", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("timesync_bench.py measures on the MI355X: no GPU here, nothing measured")
    dev = torch.device("cuda", 0)
    model, encode, routes = build(dev)
    lines = [f"Time-synchronous beam search beside the label-synchronous one: tailored AV-Branchformer 12L + 6L decoder + 16 x 512 LM, {DUR_S} s "
             f"utterances (the encoder's frames are given per batch below), V = 41, beam {SEARCH['beam_size']}, ctc_weight {SEARCH['ctc_weight']} (1.0 for CTC alone), lm_weight "
             f"{SEARCH['lm_weight']}, length bonus {SEARCH['penalty']}, f32, random-init weights",
             "one process, the searches alternating per round on the same encoder outputs; host clock around a device synchronise per decode() call; "
             "a step is a frame (time-sync) or a token (label-sync)"]
    rec = {"metric": "timesync_search", "unit": "ms per utterance (p50)"}
    for B, reps in ((1, args.reps1), (64, args.reps64)):
        rs = routes()
        enc, lens = measure(encode, rs, B, reps, dev, lines, rec)
        new_slots_per_frame(rs[2][1], enc, lens, lines, rec, B)
        with torch.no_grad():
            kernels_alone(model, enc, lens, lines, rec, SEARCH["beam_size"], SEARCH["penalty"], B)
        if B == 1:
            cpu_restatement(model, enc, lens, lines, rec, SEARCH["beam_size"], SEARCH["penalty"])
        del rs
        torch.cuda.empty_cache()
    lines += reading(rec)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
