"""Beam search with a reduced scorer set on the BASELINE config-5 model shape (tailored AV-Branchformer 12L, 4 s utterances: 400 mel
frames + 100 lip frames 88 x 88 -> T = 99 encoder frames, random-init weights, beam 10, length bonus 0.5), batch 1 and 64.

Five routes over ONE model and the SAME encoder outputs, alternating inside one process (round r: route i, ii, iii, iv, v; then round r + 1):
  (i)   hybrid, ctc_weight 1.0, no LM   - the only CTC search before the scorer sets: the 6-layer decoder runs at weight 0
  (ii)  CTC only, token by token        - skip_zero_weight, CTC_SEARCH_FUSED = False: prefix step + beam update + commit per token, captured
  (iii) CTC only, one launch            - tavsr_ctc_beam_search: the whole search of an utterance in one workgroup, lattice in LDS
  (iv)  CTC + LM (16 x 512, weight 0.6) - prefix scores of every token beside the LM's chain
  (v)   attention only (ctc_weight 0.0) - decoder chain, plain top-K, nothing of the CTC family
(i) - (iii) are the same search and must return the same hypotheses ((ii) and (iii) bit for bit); (iv) and (v) are other searches with
their own token counts.  Per route: time per decode() call (host clock around a device synchronise, p50 / p10 / p90 over the timed
rounds; the CTC head's GEMM + log-softmax is inside), tokens searched (the longest utterance of the batch), time per token, utterances/s;
and the device time of the one launch of (iii) alone.
Protocol of bench_decode.py: inputs resident in HBM, one warm-up round at the timed batch size (captures every route's graph).

    python scripts/ctc_decode_bench.py [--out profiles/ctc_decode_bench.txt] [--reps1 16] [--reps64 6]
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

from bench_decode import DUR_S, LM_CONF, make_conf, make_utts  # noqa: E402

BEAM, PENALTY = 10, 0.5
ROUTES = ["i hybrid w_dec=0", "ii ctc stepwise", "iii ctc one launch", "iv ctc + lm", "v attention only"]


def build(dev):
    from tavsr.inference.beam_search import BatchBeamSearch, CapturedEncode
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.avsr import AVSRTask
    conf = make_conf()
    torch.manual_seed(1)
    model = AVSRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).eval().to(dev)
    lm = TransformerLM(len(conf["token_list"]), **LM_CONF).eval().to(dev)

    def search(lm_, ctc_weight, lm_weight, skip):
        return BatchBeamSearch(model, lm_, BEAM, ctc_weight, lm_weight, PENALTY, skip_zero_weight=skip)
    # (route, search object, CTC_SEARCH_FUSED while it decodes)
    routes = [(ROUTES[0], search(None, 1.0, 0.0, False), True), (ROUTES[1], search(None, 1.0, 0.0, True), False),
              (ROUTES[2], search(None, 1.0, 0.0, True), True), (ROUTES[3], search(lm, 1.0, 0.6, True), True),
              (ROUTES[4], search(None, 0.0, 0.0, True), True)]
    assert [r[1].scorers for r in routes] == [("decoder", "ctc", "length_bonus"), ("ctc", "length_bonus"), ("ctc", "length_bonus"),
                                              ("ctc", "length_bonus", "lm"), ("decoder", "length_bonus")]
    return model, CapturedEncode(model), routes


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(dev, encode, routes, B, reps, lines, rec):
    from tavsr.inference import beam_search as PBS
    with torch.no_grad():
        encs = []
        for i in range(reps + 1):                                  # batch 0: warm-up round
            e, ol = encode(*make_utts(B, 1234 + i, dev))
            encs.append((e.clone(), ol.clone().to(torch.int64)))
        T = {name: [] for name, _, _ in routes}
        tokens = {name: [] for name, _, _ in routes}
        same_as_hybrid = True
        for rnd, (e, ol) in enumerate(encs):
            outs = {}
            for name, search, fused in routes:
                PBS.CTC_SEARCH_FUSED = fused
                t, out = clock(lambda: search.decode(e, ol, nbest=1))
                PBS.CTC_SEARCH_FUSED = True
                outs[name] = out
                if rnd > 0:
                    T[name].append(t)
                    tokens[name].append(max(search.n_steps))
            assert outs[ROUTES[1]] == outs[ROUTES[2]], "the stepwise and the one-launch CTC search disagree"
            same_as_hybrid &= [[h[0] for h in u] for u in outs[ROUTES[0]]] == [[h[0] for h in u] for u in outs[ROUTES[2]]]
    assert routes[1][1]._captured.graph is not None and routes[2][1]._captured.graph is None      # the routes really taken
    lines.append(f"batch {B}: {reps} timed rounds; (ii) and (iii) return identical hypotheses and scores, (i) the same best token sequences: "
                 f"{'yes' if same_as_hybrid else 'NO'}")
    lines.append(f"  {'route':<22} {'ms / decode p50':>16} {'p10':>9} {'p90':>9} {'tokens':>8} {'us / token':>11} {'utt / s':>10}")
    r = rec[f"batch{B}"] = {}
    for name, _, _ in routes:
        ms = 1e3 * np.array(T[name])
        tok = float(np.mean(tokens[name]))
        us_tok = float(np.median(1e6 * np.array(T[name]) / np.array(tokens[name])))
        p50, p10, p90 = (float(np.percentile(ms, q)) for q in (50, 10, 90))
        lines.append(f"  {name:<22} {p50:16.3f} {p10:9.3f} {p90:9.3f} {tok:8.1f} {us_tok:11.1f} {1e3 * B / p50:10.1f}")
        r[name] = dict(ms_per_decode=round(p50, 3), tokens=round(tok, 1), us_per_token=round(us_tok, 1), utt_per_s=round(1e3 * B / p50, 1))
    a, b, c = (r[ROUTES[k]]["us_per_token"] for k in range(3))
    lines.append(f"  time per token, one launch / hybrid at decoder weight 0: (iii)/(i) = {c / a:.4f}; one launch / stepwise: (iii)/(ii) = {c / b:.4f}")
    r["iii_over_i"], r["iii_over_ii"] = round(c / a, 4), round(c / b, 4)
    # what of (iii) is the launch itself: device events around tavsr_ctc_beam_search alone, on the last batch's buffers (the rest of a
    # decode() call is the CTC head's GEMM + log-softmax, two device-to-host copies and the host's per-token replay of the records)
    from tavsr import ops
    search = routes[2][1]
    cap = search._captured.bufs
    ms = []
    for _ in range(7):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ops.ctc_beam_search(cap.logp_ctc, cap.enc_lens, cap.maxl, cap.hist, cap.n_steps, BEAM, search.sos, search.eos,
                            search.w_ctc, search.w_len, True, -10.0)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    dev_ms, ntok = float(np.median(ms[1:])), int(cap.n_steps.max())
    lines.append(f"  the one launch alone (device events): {dev_ms:.3f} ms for {ntok} tokens = {1e3 * dev_ms / ntok:.1f} us / token")
    r["launch_ms"], r["launch_us_per_token"] = round(dev_ms, 3), round(1e3 * dev_ms / ntok, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps1", type=int, default=16)
    ap.add_argument("--reps64", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_decode_bench.py measures on the MI355X: no GPU here, nothing measured")
    dev = torch.device("cuda", 0)
    model, encode, routes = build(dev)
    lines = [f"Beam search by scorer set, tailored AV-Branchformer 12L + 6L decoder (+ 16 x 512 LM in iv), {DUR_S} s utterances (T = 99 encoder "
             f"frames), beam {BEAM}, length bonus {PENALTY}, f32, random-init weights",
             "one process, routes alternating per round on the same encoder outputs; host clock around a device synchronise per decode() call"]
    rec = {"metric": "ctc_decode", "unit": "us per token (p50)"}
    for B, reps in ((1, args.reps1), (64, args.reps64)):
        measure(dev, encode, routes, B, reps, lines, rec)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
