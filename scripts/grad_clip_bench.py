"""What gradient clipping costs on the optimizer step and on an epoch: the audio-only recipe's parameter set
(configs/asr_branchformer_transformer_ctc_english.yaml, random-init weights, random gradients) under ``FusedAdam``.

Three tables, every arm of a table alternated with the others in one process:
  1. ``optimizer.step()`` between device events (pack launches included), the queue drained before every repetition so that all
     arms start alike: clipping off / on with a max_norm that never binds / on with one that always binds.
  2. the update launches alone over the whole flat buffer, between device events: ``tavsr_adamw_step``, the three clipped
     launches (norm partials, finalize, ``tavsr_adamw_step_clip``), and - with ``--parent-lib`` - ``tavsr_adamw_step`` of another
     build of the library (the commit before clipping existed) loaded beside this one.
  3. one epoch of ``training()`` over ``--batches`` synthetic batches at accum_grad 1, grad_clip off against on: host clock around
     the epoch with a synchronisation at its end.

    python scripts/grad_clip_bench.py [--out profiles/grad_clip_bench.txt] [--reps 50] [--parent-lib PATH] [--no-epoch]
"""
import argparse
import copy
import ctypes
import json
import os
import random
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
    conf = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "asr_branchformer_transformer_ctc_english.yaml")))
    conf.update(input_size=N_MEL, specaug=None)
    torch.manual_seed(0)
    return ASRTask.build_model(argparse.Namespace(**copy.deepcopy(conf))).to(dev).train()


def stats(x):
    x = np.asarray(x)
    return tuple(float(np.percentile(x, q)) for q in (50, 10, 90))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(arms, reps, warmup):
    for _ in range(warmup):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    T = {name: [] for name, _ in arms}
    order, rng = list(arms), random.Random(0)
    for _ in range(reps):
        # a new order every round: what an arm finds in the Infinity Cache depends on the arm before it (the one after "norm
        # partials alone" finds part of the gradient there), and a fixed order would hand that to one arm every time
        rng.shuffle(order)
        for name, fn in order:
            T[name].append(event_ms(fn))
    return T


def table(title, unit, arms, T, base):
    lines = [title, f"  {unit:<44} {'p50':>9} {'p10':>9} {'p90':>9} {'p50 / ' + base:>18}"]
    b50 = stats(T[base])[0]
    for name, _ in arms:
        p50, p10, p90 = stats(T[name])
        lines.append(f"  {name:<44} {p50:9.4f} {p10:9.4f} {p90:9.4f} {p50 / b50:18.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per arm of table 3, alternated")
    ap.add_argument("--parent-lib", default=None, help="another build of libtavsr_hip.so whose tavsr_adamw_step joins table 2")
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench.py measures on the MI355X: no GPU here, nothing measured")
    from tavsr import _lib as L
    from tavsr.train import FusedAdam, get_noam_scheduler, training
    dev = torch.device("cuda", 0)
    model = build(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=1e-4, betas=(0.9, 0.98), eps=1e-9)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    n = opt.flat.numel()
    lines = [f"Gradient clipping on the optimizer step: audio-only Branchformer 12L + 6L decoder, {len(params)} tensors, {n} floats in "
             f"the flat buffer ({n * 4 / 2**20:.1f} MiB), f32, random gradients",
             f"{args.reps} repetitions per arm after {args.warmup} warm-up rounds, arms alternated in one process; device events", ""]
    rec = {"metric": "grad_clip_overhead", "floats": n, "tensors": len(params), "reps": args.reps}

    # ---- 1. optimizer.step()
    def stepper(max_norm):
        def fn():
            opt.set_grad_clip(max_norm)
            opt.step()
        return fn

    arms = [("clipping off", stepper(-1.0)), ("on, max_norm 1e9 (never binds)", stepper(1e9)),
            ("on, max_norm 1e-3 (always binds)", stepper(1e-3))]
    T = alternate(arms, args.reps, args.warmup)
    lines += table("1. optimizer.step() (pack + update), queue drained before every repetition", "ms per step", arms, T, "clipping off") + [""]
    rec["step_ms_p50"] = {name: round(stats(T[name])[0], 4) for name, _ in arms}
    st = opt.clip_stats()
    assert st["skipped"] == 0 and st["clipped"] == (args.reps + args.warmup), st
    lines += [f"  (clip_stats after table 1: {st})", ""]

    # ---- 2. the update launches alone
    lib = L.lib()
    flat, grad, m, v = (t.data_ptr() for t in (opt.flat, opt.grad, opt.exp_avg, opt.exp_avg_sq))
    nparts = lib.tavsr_grad_norm_nparts(n)
    parts = torch.zeros(nparts, dtype=torch.float64, device=dev)
    out, counters = torch.zeros(3, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    count = [opt._step]

    def plain(which):
        def fn():
            count[0] += 1
            L.check(which.tavsr_adamw_step(flat, grad, m, v, n, 1e-4, 0.9, 0.98, 1e-9, 0.0, count[0], 1.0, L.stream()), "tavsr_adamw_step")
        return fn

    def clipped():
        count[0] += 1
        L.check(lib.tavsr_grad_norm_parts(grad, n, 2, parts.data_ptr(), 0, L.stream()), "tavsr_grad_norm_parts")
        L.check(lib.tavsr_grad_clip_coef(parts.data_ptr(), nparts, 2, 1e-3, out.data_ptr(), counters.data_ptr(), L.stream()),
                "tavsr_grad_clip_coef")
        L.check(lib.tavsr_adamw_step_clip(flat, grad, m, v, n, 1e-4, 0.9, 0.98, 1e-9, 0.0, count[0], 1.0, out.data_ptr(), L.stream()),
                "tavsr_adamw_step_clip")

    def norm_only():
        L.check(lib.tavsr_grad_norm_parts(grad, n, 2, parts.data_ptr(), 0, L.stream()), "tavsr_grad_norm_parts")

    arms = [("tavsr_adamw_step", plain(lib)), ("norm + finalize + tavsr_adamw_step_clip", clipped), ("norm partials alone", norm_only)]
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.tavsr_adamw_step.restype, parent.tavsr_adamw_step.argtypes = L.PROTOTYPES["tavsr_adamw_step"]
        arms.insert(1, ("tavsr_adamw_step, parent build", plain(parent)))
    T = alternate(arms, args.reps, args.warmup)
    lines += table("2. the update launches over the whole flat buffer", "ms", arms, T, "tavsr_adamw_step")
    p50 = stats(T["tavsr_adamw_step"])[0]
    lines += [f"  (tavsr_adamw_step: 28 bytes per float -> {28 * n / p50 / 1e9:.2f} TB/s; norm partials: 4 bytes per float -> "
              f"{4 * n / stats(T['norm partials alone'])[0] / 1e9:.2f} TB/s)", ""]
    rec["update_ms_p50"] = {name: round(stats(T[name])[0], 4) for name, _ in arms}

    # ---- 3. an epoch of training()
    if not args.no_epoch:
        del opt
        model = build(dev)
        noam = get_noam_scheduler(model.parameters(), 0.05, 256, 25000)
        g = torch.Generator().manual_seed(1234)
        batch = dict(speech=torch.randn(B, T_IN, N_MEL, generator=g), speech_lengths=torch.full((B,), T_IN, dtype=torch.int64),
                     text=torch.randint(1, 40, (B, L_TXT), generator=g), text_lengths=torch.full((B,), L_TXT, dtype=torch.int64))
        batch = {k: t.to(dev) for k, t in batch.items()}
        loader = [batch] * args.batches

        def epoch(grad_clip):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = training(model, loader, noam, None, 1, device=dev, grad_clip=grad_clip)
            torch.cuda.synchronize()
            assert np.isfinite(loss), loss
            return time.perf_counter() - t0

        training(model, loader[:5], noam, None, 1, device=dev)
        training(model, loader[:5], noam, None, 1, device=dev, grad_clip=5.0)
        E = {"grad_clip off": [], "grad_clip 5.0": []}
        for _ in range(args.epochs):
            E["grad_clip off"].append(epoch(-1.0))
            E["grad_clip 5.0"].append(epoch(5.0))
        lines += [f"3. one epoch of training(): {args.batches} batches of {B} x {T_IN} mel frames x {N_MEL}, {L_TXT} tokens, accum_grad 1, "
                  f"Noam + FusedAdam, recipe dropout; host clock, {args.epochs} epochs per arm, alternated",
                  f"  {'s per epoch':<44} {'median':>9} {'min':>9} {'max':>9}   each"]
        for name, x in E.items():
            lines.append(f"  {name:<44} {np.median(x):9.3f} {min(x):9.3f} {max(x):9.3f}   {' '.join(f'{t:.3f}' for t in x)}")
        lines += [f"  (clip_stats at the end: {noam.clip_stats()})", ""]
        rec["epoch_s"] = {k: [round(t, 3) for t in x] for k, x in E.items()}
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
