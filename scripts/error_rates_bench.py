"""Validation error rates: time of one eval() forward of the audio-only recipe model (Branchformer 12L + 6L decoder, 80-dim
features, random-init weights) at batch 32 with ``ops.DEVICE_ERROR_RATES`` off - the host route: ids copied to the host, a Python
edit distance per utterance and metric, which is what the forward did before the device route existed and so is the baseline -
and on (csrc/editdist.hip: one launch for cer_ctc, one for cer + wer, nothing read on the host), and of the launches alone.
Three clip lengths: 400 / 1000 / 2000 feature frames (4 / 10 / 20 s: 99 / 249 / 499 encoder frames) with transcripts of 60 / 150 /
300 characters of the 41-token English inventory, a space every sixth character.  A random-init model's CTC argmax is noise:
its collapsed hypothesis has about as many characters as there are frames, longer than a trained model's (about the
transcript's length), so the host route's n x m is on its large side here; the file states the hypothesis lengths.

Forward: host clock around a device synchronise, routes alternating per round, p50 (p10 - p90).  Launches alone: HIP events
around ``ops.error_counts`` (output allocations included) on the ids of that forward.

    python scripts/error_rates_bench.py [--out profiles/error_rates_bench.txt] [--rounds 8]
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

SHAPES = [(400, 60), (1000, 150), (2000, 300)]      # (feature frames, transcript characters)
BATCH = 32


def pct(ms):
    return float(np.percentile(ms, 50)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_rates_bench.py measures on the MI355X: no GPU here, nothing measured")
    from tavsr import ops
    from tavsr.tasks.asr import ASRTask
    from tavsr.utils.tokens import CHAR_ENGLISH
    dev = torch.device("cuda", 0)
    conf = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_transformer_ctc_english.yaml")))
    conf.update(input_size=80, specaug=None, token_list=list(CHAR_ENGLISH))
    conf["model_conf"].update(report_cer=True, report_wer=True)
    torch.manual_seed(0)
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).eval().to(dev)
    calc = model.error_calculator
    space = CHAR_ENGLISH.index("<space>")
    lines = [f"eval() forward of the audio-only recipe model (12L Branchformer + 6L decoder, random init), batch {BATCH}, cer_ctc + cer + wer; "
             f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}",
             "forward: ms, host clock around a device synchronise, routes alternating, p50 (p10 - p90); launches alone: HIP events, p50"]
    rec = {"metric": "error_rates", "unit": "ms (p50)"}

    def forward(batch, on):
        ops.DEVICE_ERROR_RATES = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            _, stats, _ = model(*batch)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), stats

    for frames, chars in SHAPES:
        g = torch.Generator().manual_seed(frames)
        text = torch.randint(14, 40, (BATCH, chars), generator=g)      # letters
        text[:, 5::6] = space
        batch = [torch.randn((BATCH, frames, 80), generator=g).to(dev), torch.full((BATCH,), frames, device=dev), text.to(dev),
                 torch.full((BATCH,), chars, device=dev)]
        ms, values = {False: [], True: []}, {}
        for rnd in range(args.rounds + 2):      # two warm-up rounds
            for on in (False, True):
                t, stats = forward(batch, on)
                if rnd >= 2:
                    ms[on].append(t)
                else:
                    values[on] = [float(stats[k]) for k in ("cer_ctc", "cer", "wer")]
        same = values[False] == values[True]
        ops.DEVICE_ERROR_RATES = True
        with torch.no_grad():
            enc, _ = model.encode(batch[0], batch[1])
            ys_hat = model.ctc.argmax(enc)
        tb = calc._tables(ys_hat, batch[2], 1)
        n_hyp = float((ys_hat[:, 1:] != ys_hat[:, :-1]).sum() + BATCH) / BATCH      # runs per row: an upper bound of the kept tokens
        att = torch.cat([batch[2], batch[2][:, :1]], 1)
        alone = {}
        for name, fn in (("cer_ctc", lambda: ops.error_counts(ys_hat, batch[2], tb, 1)), ("cer + wer", lambda: ops.error_counts(att, batch[2], tb, 6))):
            for _ in range(3):
                fn()
            t = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
            alone[name] = pct(t)[0]
        off, on = pct(ms[False]), pct(ms[True])
        lines.append(f"{frames} frames -> {ys_hat.shape[1]} encoder frames, {chars}-character transcripts ({n_hyp:.0f} id runs per CTC hypothesis row); "
                     f"both routes return the same cer_ctc / cer / wer: {'yes' if same else 'NO'}")
        lines.append(f"  host route   (DEVICE_ERROR_RATES off) {off[0]:10.2f}  ({off[1]:.2f} - {off[2]:.2f})")
        lines.append(f"  device route (DEVICE_ERROR_RATES on)  {on[0]:10.2f}  ({on[1]:.2f} - {on[2]:.2f})    device / host = {on[0] / off[0]:.3f}")
        lines.append(f"  launches alone: cer_ctc {alone['cer_ctc']:.3f} ms, cer + wer (one launch) {alone['cer + wer']:.3f} ms")
        rec[f"T{frames}_C{chars}"] = {"host_ms": round(off[0], 2), "device_ms": round(on[0], 2), "ratio": round(on[0] / off[0], 4),
                                     "cer_ctc_launch_ms": round(alone["cer_ctc"], 3), "cer_wer_launch_ms": round(alone["cer + wer"], 3),
                                     "same_values": bool(same)}
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
