"""What the n-gram scorer costs inside the beam search, on the BASELINE config-5 search (tailored AV-Branchformer 12L + 6L decoder + 16 x 512
Transformer LM, 4 s utterances -> T = 99 encoder frames, beam 10, ctc_weight 0.1, lm_weight 0.6, length bonus 0.5, random-init weights).

A synthetic order-4 character ARPA over the 41-token list (tests/ngram_ref.py: interpolated absolute discounting over random text) is
scored as a full scorer at weight 0.9.  Two search objects over ONE model and the SAME encoder outputs - without and with the n-gram -
alternate inside one process (round r: without, with; then round r + 1), at batch 1 (time per token) and batch 64 (utterances/s).  The
yardstick is the search without the n-gram in the same call: the difference of the two medians against the spread (p10 .. p90) of either.
The two searches are different searches (the n-gram moves the hypotheses), so with end detection their token counts differ - and a token
late in a search costs more than an early one (attention over a longer history) - so each batch size is measured twice: the search as
config 5 runs it (maxlenratio 0: end detection), and with a fixed budget of 80 tokens for both (maxlenratio -80), where the two do the same
number of steps over histories of the same lengths and the difference is the n-gram row alone.  Then the kernel alone, device events
around 200 back-to-back launches, at N = 10 and N = 640 hypotheses.
Protocol of bench_decode.py: inputs resident in HBM, one warm-up round at the timed batch size (captures both graphs).

    python scripts/ngram_bench.py [--out profiles/ngram_bench.txt] [--reps1 16] [--reps64 6]
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tailored-avsr_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_decode import DUR_S, LM_CONF, SEARCH, make_conf, make_utts  # noqa: E402

ORDER, W_NGRAM, BUDGET = 4, 0.9, 80
ROUTES = ["without n-gram", "with n-gram (full)"]


def synthetic_arpa(path, token_list):
    import ngram_ref
    words = [t for t in token_list if not t.startswith("<")] + ["<space>"]
    sents = ngram_ref.random_sentences(words, 1500, seed=4, max_len=40, skew=1.0)
    ngram_ref.write_arpa(path, sents, ORDER, words)


def build(dev):
    from tavsr.inference.beam_search import BatchBeamSearch, CapturedEncode
    from tavsr.lm.ngram import NgramLM
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.avsr import AVSRTask
    conf = make_conf()
    torch.manual_seed(1)
    model = AVSRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).eval().to(dev)
    lm = TransformerLM(len(conf["token_list"]), **LM_CONF).eval().to(dev)
    with tempfile.TemporaryDirectory() as d:
        synthetic_arpa(os.path.join(d, "chars4.arpa"), conf["token_list"])
        ng = NgramLM.from_arpa(os.path.join(d, "chars4.arpa"), conf["token_list"], dev)

    def routes(maxlenratio):
        r = [(ROUTES[0], BatchBeamSearch(model, lm, **SEARCH, maxlenratio=maxlenratio)),
             (ROUTES[1], BatchBeamSearch(model, lm, **SEARCH, maxlenratio=maxlenratio, ngram=ng, ngram_weight=W_NGRAM))]
        assert r[0][1].scorers == ("decoder", "ctc", "length_bonus", "lm") and r[1][1].scorers == r[0][1].scorers + ("ngram",)
        return r
    return CapturedEncode(model), routes, ng


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(dev, encode, routes, B, reps, lines, rec, what):
    with torch.no_grad():
        encs = []
        for i in range(reps + 1):                                  # batch 0: warm-up round
            e, ol = encode(*make_utts(B, 1234 + i, dev))
            encs.append((e.clone(), ol.clone().to(torch.int64)))
        T = {name: [] for name, _ in routes}
        tokens = {name: [] for name, _ in routes}
        for rnd, (e, ol) in enumerate(encs):
            for name, search in routes:
                t, _ = clock(lambda: search.decode(e, ol, nbest=1))
                if rnd > 0:
                    T[name].append(t)
                    tokens[name].append(max(search.n_steps))
    assert all(s._captured.graph is not None for _, s in routes)
    lines.append(f"batch {B}, {what}: {reps} timed rounds")
    lines.append(f"  {'search':<22} {'ms / decode p50':>16} {'p10':>9} {'p90':>9} {'tokens':>8} {'us / token':>11} {'p10':>9} {'p90':>9} {'utt / s':>10}")
    r = rec[f"batch{B}_{what.split()[0]}"] = {}
    for name, _ in routes:
        ms = 1e3 * np.array(T[name])
        tok = float(np.mean(tokens[name]))
        per = 1e6 * np.array(T[name]) / np.array(tokens[name])
        p50, p10, p90 = (float(np.percentile(ms, q)) for q in (50, 10, 90))
        u50, u10, u90 = (float(np.percentile(per, q)) for q in (50, 10, 90))
        lines.append(f"  {name:<22} {p50:16.3f} {p10:9.3f} {p90:9.3f} {tok:8.1f} {u50:11.1f} {u10:9.1f} {u90:9.1f} {1e3 * B / p50:10.1f}")
        r[name] = dict(ms_per_decode=round(p50, 3), tokens=round(tok, 1), us_per_token=round(u50, 1), us_per_token_p10=round(u10, 1),
                       us_per_token_p90=round(u90, 1), utt_per_s=round(1e3 * B / p50, 1))
    a, b = r[ROUTES[0]], r[ROUTES[1]]
    bar = max(a["us_per_token_p90"] - a["us_per_token_p10"], b["us_per_token_p90"] - b["us_per_token_p10"])
    lines.append(f"  time per token, with - without: {b['us_per_token'] - a['us_per_token']:+.1f} us ({b['us_per_token'] / a['us_per_token']:.4f}x); "
                 f"noise bar of this call (the wider p10 .. p90 of the two): {bar:.1f} us")
    r["delta_us_per_token"], r["noise_bar_us"] = round(b["us_per_token"] - a["us_per_token"], 1), round(bar, 1)


def kernel_alone(dev, ng, V, lines, rec):
    from tavsr import ops
    L, step, launches = 102, 60, 200
    for N in (10, 640):
        yseq = torch.randint(2, V - 1, (N, L), device=dev)
        out = torch.zeros(N, V, device=dev)
        us = []
        for _ in range(6):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                ops.ngram_score(ng, yseq, step, out=out, alpha=W_NGRAM, accumulate=True)
            t1.record()
            torch.cuda.synchronize()
            us.append(1e3 * t0.elapsed_time(t1) / launches)
        lines.append(f"  tavsr_ngram_score alone, N = {N:3d} hypotheses x {V} tokens, order {ng.order}, {ng.n_nodes} n-grams: "
                     f"{float(np.median(us[1:])):.2f} us per launch (back-to-back, device events, median of 5 x {launches})")
        rec[f"kernel_us_N{N}"] = round(float(np.median(us[1:])), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps1", type=int, default=16)
    ap.add_argument("--reps64", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngram_bench.py measures on the MI355X: no GPU here, nothing measured")
    dev = torch.device("cuda", 0)
    encode, routes, ng = build(dev)
    lines = [f"N-gram scorer in the config-5 search: tailored AV-Branchformer 12L + 6L decoder + 16 x 512 LM, {DUR_S} s utterances (T = 99 encoder "
             f"frames), beam {SEARCH['beam_size']}, ctc_weight {SEARCH['ctc_weight']}, lm_weight {SEARCH['lm_weight']}, f32, random-init weights; "
             f"synthetic order-{ORDER} character ARPA ({ng.n_nodes} n-grams) at ngram_weight {W_NGRAM}, full scorer",
             "one process, the two searches alternating per round on the same encoder outputs; host clock around a device synchronise per decode() call"]
    rec = {"metric": "ngram_in_search", "unit": "us per token (p50)"}
    for B, reps in ((1, args.reps1), (64, args.reps64)):
        for what, ratio in (("natural search (end detection)", 0.0), (f"fixed budget of {BUDGET} tokens", -float(BUDGET))):
            measure(dev, encode, routes(ratio), B, reps, lines, rec, what)
    kernel_alone(dev, ng, ng.word_map.numel(), lines, rec)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
