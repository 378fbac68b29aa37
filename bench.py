"""Headline benchmark (BASELINE.json: "utterances/sec fwd+bwd, 12L AV-Branchformer, 4 s clips, batch 32, 1->8 MI355X"):
utterances/s, forward+backward, of the tailored audio-visual Branchformer (BASELINE configs[2]/[3]: Conv3d + ResNet-18
lip frontend, Conv2dSubsampling audio embed, 12 tailored AV layers, adaptive fusion, CTC + 6-layer Transformer decoder,
configs/AVSR/tailored_transformer+ctc_english.yaml), batch 32 x 4 s clips (400 mel frames x 80 + 100 lip frames 88 x 88)
per GPU, fp32, train mode with the recipe's dropout, synthetic data, random-init weights.  Weak scaling: every rank steps
its own batch of 32; ranks exchange gradients once per step (RCCL all-reduce, tavsr.dp).
``--workload asr`` runs BASELINE configs[1] instead (audio-only 12-layer Branchformer + CTC + decoder, same batch).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_out/outputs
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets the step up, warms it up, times K steps and prints ONE JSON line on rank 0: metric, value, unit,
higher_is_better, dtype, ms_per_step (the milliseconds one timed step took), the step's configuration, and
rccl_world, dist_world, dist_backend, hbm_peak_gb_per_rank - which exchange really ran (ranks of the C ABI's RCCL
communicator, 0 = none) and every rank's peak device memory: the first things to read on an N > 1 line.
``--dump-outputs DIR`` writes what the last timed step computed (the loss and the parameter gradients a caller of the step
receives) as DIR/<name>.npy; the inputs and weights are seeded, so two builds given the same arguments can be compared
output for output.  ``--full`` adds every other measurement to the line, each taken outside the timed steps:
  sustained    - the same step for --sustain-s seconds more (default 12 under --full);
  eager        - the same step as eager launches, taken before the capture (1 GPU);
  grad_exchange_exposed_ms_per_step - N > 1 or --force-rccl: the exchange's stream time that nothing hides;
  box          - in-process calibration of THIS device before the model is built (fp32 MFMA microbench, HBM copy);
  asr          - BASELINE configs[1] (the audio-only step) under the same protocol, so the driver's record holds it too (with its own
                 CPU figure);
  decode       - BASELINE configs[4] (beam 10 + 16 x 512 LM on the AV model): batch-1 p50 RTF over 8 utterances of 4 s and batch-64
                 utterances/s over 128, taken by a child `bench_decode.py --driver-record` BEFORE this process touches the GPU (a second HIP
                 context on the device, even an idle one, costs a batch-1 search 11 - 19 % per token);
  fwd_encoder  - north_star's forward target (12-layer Branchformer forward, batch 32);
  roofline     - the dominant kernel (fp32 MFMA GEMM instantiation with the largest total time): algorithmic
                 FLOPs / HIP-event launch durations, measured in a separate instrumented replay of the same step;
  cpu_baseline - the oracle (CPU restatement, eager torch fp32) timed on this box's host cores on a bounded sample.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "tailored-avsr_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 256 FLOP/clk x 2.4 GHz
# Algorithmic work, forward, per utterance (BASELINE.md section 2 / SURVEY Appendix C).  fwd+bwd = 3x fwd MINUS the data
# gradients nobody needs and the step never computes: the inputs' own (Conv3d stem 1->64, k 5x7x7 on 100x44x44 outputs:
# 2*245*64*193600 = 6.07 GFLOP/utt; Conv2dSubsampling conv1 1->256 k3 on 199x39 outputs: 0.036 GFLOP/utt).
GFLOP_PER_UTT_FWD = {"asr": 11.35, "avsr": 79.14}
GFLOP_PER_UTT_STEP = {"asr": 3 * 11.35 - 0.036, "avsr": 3 * 79.14 - 6.07 - 0.036}
GFLOP_12L_FWD_PER_UTT = 7.95      # the 12 MyBranchformerEncoderLayers alone: 254 GFLOP at B = 32 (north_star's forward target)
GFLOP_EMBED_FWD_PER_UTT = 2.50    # Conv2dSubsampling
B_PER_GPU, T_IN, N_MEL, L_TXT, T_VID, HW = 32, 400, 80, 40, 100, 88
WORKLOAD = "avsr"  # set by --workload: "avsr" = BASELINE configs[2]/[3] (the AV-Branchformer the metric names), "asr" = configs[1]


def hbm_traffic(layout_key):
    """HBM bytes per launch of the dominant GEMM family, from the committed rocprofv3 PMC pass over this same step
    (scripts/gpu_pmc_hbm.sh -> profiles/summarize_pmc.py: FETCH_SIZE x2 on gfx950 + WRITE_SIZE, KiB -> bytes).  PMC
    counters cannot be read from inside the process, so this is the profile's number, or None if it is absent."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_hbm_" + ("av" if WORKLOAD == "avsr" else "asr") + ".json")))
    if not cands:
        return None
    path = cands[-1]              # the latest round's pass
    ak, bkm = {"NT": ("false", "false"), "NN": ("false", "true"), "TN": ("true", "true"), "TT": ("true", "false")}[layout_key[-3:-1]]
    tot = calls = 0.0
    for name, v in json.load(open(path)).items():
        if "gemm_glds_kernel" in name and [t for t in name.rstrip(">").split(", ") if t in ("true", "false")] == [ak, bkm]:
            tot += v["calls"] * (v["read_bytes_per_launch"] + v["write_bytes_per_launch"])
            calls += v["calls"]
    return round(tot / calls) if calls else None


def _zero_dropout(d):
    for k, v in d.items():
        if isinstance(v, dict):
            _zero_dropout(v)
        elif k.endswith("dropout_rate"):
            d[k] = 0.0


DROPOUT = True   # --no-dropout sets every rate to 0 (parity-style run)


def make_conf():
    """The recipe as shipped: train mode WITH the reference's dropout rates (0.1 everywhere), on the GPU and in the
    CPU baseline alike."""
    if WORKLOAD == "avsr":
        conf = yaml.safe_load(open(os.path.join(PKG, "configs", "avsr_tailored_transformer_ctc_english.yaml")))
        conf.update(acoustic_input_size=N_MEL, visual_input_size=None, specaug=None)
    else:
        conf = yaml.safe_load(open(os.path.join(PKG, "configs", "asr_branchformer_transformer_ctc_english.yaml")))
        conf.update(input_size=N_MEL, specaug=None)
    if not DROPOUT:
        _zero_dropout(conf)
    return conf


def make_batch(batch, seed, device):
    g = torch.Generator().manual_seed(seed)
    speech = torch.randn(batch, T_IN, N_MEL, generator=g)
    slens = torch.full((batch,), T_IN, dtype=torch.int64)
    text = torch.randint(1, 40, (batch, L_TXT), generator=g)
    tlens = torch.full((batch,), L_TXT, dtype=torch.int64)
    if WORKLOAD == "avsr":
        video = torch.randn(batch, T_VID, HW, HW, generator=g)
        vlens = torch.full((batch,), T_VID, dtype=torch.int64)
        return [t.to(device) for t in (speech, slens, video, vlens, text, tlens)]
    return [t.to(device) for t in (speech, slens, text, tlens)]


def build_product_model():
    import copy as _copy
    if WORKLOAD == "avsr":
        from tavsr.tasks.avsr import AVSRTask
        return AVSRTask.build_model(argparse.Namespace(**_copy.deepcopy(make_conf())))
    from tavsr.tasks.asr import ASRTask
    return ASRTask.build_model(argparse.Namespace(**_copy.deepcopy(make_conf())))


def host_cores():
    """(physical cores of the box per lscpu, hardware threads this process may run on)."""
    import re
    import subprocess
    phys = None
    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        get = lambda k: int(re.search(rf"^{k}:\s*(\d+)", txt, re.M).group(1))
        phys = get(r"Core\(s\) per socket") * get(r"Socket\(s\)")
    except Exception:
        pass
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count() or 1
    return phys or allowed, allowed


def cpu_baseline(budget_s=30.0, workload=None, bs=None):
    """The oracle's fwd+bwd of the same model/workload on the host cores (bounded sample, SURVEY 8d / task section 4).
    Threads = the physical cores this process may use (lscpu cores, capped by the affinity mask).  Batch: the GPU
    run's batch of 32 costs the oracle ~80 s per AV step on this class of host, far beyond the bounded sample the default
    run allows, so the sample is batch 4 (AV) / 8 (audio-only) of the same clips: 1 warm-up + >= 3 timed steps, median."""
    from oracle.av import build_avsr_oracle
    from oracle.model import build_asr_oracle
    from tavsr.utils.tokens import CHAR_ENGLISH

    global WORKLOAD
    phys, allowed = host_cores()
    threads = max(1, min(phys, allowed))
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    saved, WORKLOAD = WORKLOAD, workload or WORKLOAD       # (the `asr` object's own CPU figure: configs[1] beside the headline)
    try:
        build = build_avsr_oracle if WORKLOAD == "avsr" else build_asr_oracle
        model = build(copy.deepcopy(make_conf()), CHAR_ENGLISH).train()
        bs = bs or (4 if WORKLOAD == "avsr" else 8)
        batch = make_batch(bs, 1234, "cpu")
    finally:
        WORKLOAD = saved

    def step():
        for p in model.parameters():
            p.grad = None
        loss, _, _ = model(*batch)
        loss.backward()

    torch.set_num_threads(min(16, threads))
    step()  # warm-up (allocator, oneDNN primitives)
    # how many threads?  The lscpu core count is the HOST's; a pool box hands a job a share of it (16 CPUs for one GPU), and the oracle on
    # 128 threads over that share ran 6 - 10x SLOWER than on 16 (audio-only batch 4: 0.85 vs 8.8 utt/s; AV: 0.40 vs 2.4): one probe step
    # per candidate count, the fastest is the baseline's thread count (reported as `threads`; `cores` stays the host's physical cores)
    best = (float("inf"), threads)
    for th in sorted({t for t in (8, 16, 32, 64, threads) if t <= threads}):
        torch.set_num_threads(th)
        t0 = time.perf_counter()
        step()
        dt = time.perf_counter() - t0
        if dt < best[0]:
            best = (dt, th)
    threads = best[1]
    torch.set_num_threads(threads)
    times = []
    t_all = time.perf_counter()
    while len(times) < 3 or (time.perf_counter() - t_all < budget_s and len(times) < 10):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    return {"value": round(bs / med, 3), "unit": "utterances/s", "cores": phys, "threads": threads, "kind": "port",
            "sample": f"median of {len(times)} timed fwd+bwd steps (1 warm-up) of batch {bs} x 4 s clips (same model/config, "
                      f"same dropout rates; batch 32 would take ~{32 / (bs / med):.0f} s per step), eager torch fp32 oracle, "
                      f"{threads} threads (the fastest of 8 / 16 / 32 / 64 / all on a probe step) on a host of {phys} physical cores "
                      f"({allowed} hardware threads allowed), {sum(times):.1f} s timed"}


def bench_fwd_encoder(dev, steps=20, warmup=5):
    """north_star's forward target: the 12-layer Branchformer encoder FORWARD at batch 32 (T = 99 after Conv2dSubsampling),
    BASELINE configs[1] shapes.  Times (a) the 12 MyBranchformerEncoderLayers + after_norm alone - the 254 GFLOP the
    ">= 50 % MFMA" target is stated on - and (b) the whole MyBranchformerEncoder.forward incl. Conv2dSubsampling, each in
    eval mode and in train mode (recipe dropout; everything the backward needs is kept), as hipGraph replays and as eager
    launches.  fp32; HIP events on the launch stream."""
    global WORKLOAD
    saved = WORKLOAD
    WORKLOAD = "asr"
    try:
        torch.manual_seed(0)
        model = build_product_model().to(dev)
    finally:
        WORKLOAD = saved
    enc = model.encoder
    from tavsr import ops
    from tavsr.layers import make_pad_mask
    g = torch.Generator().manual_seed(1234)
    speech = torch.randn(B_PER_GPU, T_IN, N_MEL, generator=g).to(dev)
    ilens = torch.full((B_PER_GPU,), T_IN, dtype=torch.int64, device=dev)
    res = {"batch": B_PER_GPU, "T": None, "dtype": "f32", "peak_tflops": PEAK_FP32_MFMA_TFLOPS,
           "gflop_12_layers": round(GFLOP_12L_FWD_PER_UTT * B_PER_GPU, 1),
           "gflop_encoder_forward": round((GFLOP_12L_FWD_PER_UTT + GFLOP_EMBED_FWD_PER_UTT) * B_PER_GPU, 1)}

    def timed(fn, graph):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        run = fn
        if graph:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep = fn()      # noqa: F841  (graph-owned outputs)
            run = gr.replay
        for _ in range(warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for mode in ("eval", "train"):
        model.train(mode == "train")
        with torch.set_grad_enabled(mode == "train"):
            masks = (~make_pad_mask(ilens, speech.size(1))[:, None, :]).to(dev)
            with torch.no_grad():
                (x0, pos), m0 = enc.embed(speech, masks)
            lens = m0.squeeze(1).sum(1).to(torch.int64)
            res["T"] = int(x0.shape[1])
            x0 = x0.detach().requires_grad_(mode == "train")

            def layers():
                ops.rng_step_begin(dev)
                xs = (x0, pos)
                for layer in enc.encoders:
                    xs, _ = layer(xs, m0, lens=lens)
                return enc.after_norm(xs[0])

            def whole():
                ops.rng_step_begin(dev)
                return enc(speech, ilens)[0]

            for name, fn, gf in (("layers12", layers, GFLOP_12L_FWD_PER_UTT),
                                 ("encoder_forward", whole, GFLOP_12L_FWD_PER_UTT + GFLOP_EMBED_FWD_PER_UTT)):
                for launch, graph in (("graph", True), ("eager", False)):
                    ms = timed(fn, graph)
                    tf = gf * B_PER_GPU / ms          # GFLOP / ms = TFLOP/s
                    res[f"{name}_{mode}_{launch}"] = {"ms": round(ms, 3), "tflops": round(tf, 2),
                                                      "frac_of_fp32_mfma_peak": round(tf / PEAK_FP32_MFMA_TFLOPS, 4)}
    del model
    torch.cuda.empty_cache()
    return res


def box_calibration(dev):
    """What THIS box delivers, measured in-process before any model exists (boxes of one pool differ by ~5 %, which is more
    than a round's gain: without this a slower box cannot be told from a regression): (a) the fp32 matrix rate - every CU
    issuing nothing but independent v_mfma_f32_32x32x2_f32 (tavsr_mfma_peak_f32, csrc/probe.hip), ~200 ms; (b) an HBM copy
    (tavsr_axpby with a = 1: 1 GiB read + 1 GiB written per launch).  HIP events on the launch stream."""
    import ctypes as C
    from tavsr import ops
    from tavsr._lib import check, lib, ptr, stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sink = torch.zeros(1, device=dev)
    blocks, iters = 2 * cus, 200000          # 8 waves per CU, ~50 ms per launch at the nominal peak

    def mfma():
        check(lib().tavsr_mfma_peak_f32(iters, blocks, ptr(sink), stream()), "tavsr_mfma_peak_f32")

    def timed(fn, n):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    t_m = timed(mfma, 4)
    tf = blocks * 4 * iters * 4 * 4096.0 / t_m / 1e12
    # the same instruction stream on random operands (a different A / B pair for every consecutive instruction): what the
    # device's power management leaves of that rate once the multiplier inputs toggle the way activations do
    gen = torch.Generator(device="cpu").manual_seed(1234)
    operands = torch.randn(16, 256, generator=gen).to(dev)

    def mfma_data():
        check(lib().tavsr_mfma_peak_f32_data(iters, blocks, ptr(operands), ptr(sink), stream()), "tavsr_mfma_peak_f32_data")

    t_d = timed(mfma_data, 4)
    tf_d = blocks * 4 * iters * 4 * 4096.0 / t_d / 1e12
    n = 1 << 28
    x, y = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ops.fill_(x, 1.0)
    t_c = timed(lambda: ops.axpby(x, None, 1.0, 0.0, out=y), 20)
    del x, y
    torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(dev), "cus": cus,
            "fp32_mfma_tflops": round(tf, 1), "fp32_mfma_frac_of_nominal": round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
            "mfma_ms_per_launch": round(1e3 * t_m, 2),
            "fp32_mfma_tflops_data": round(tf_d, 1), "fp32_mfma_data_frac_of_nominal": round(tf_d / PEAK_FP32_MFMA_TFLOPS, 4),
            "hbm_copy_gb_per_s": round(2 * 4 * n / t_c / 1e9, 1),
            "note": "in-process calibration before the model is built: back-to-back v_mfma_f32_32x32x2_f32 on every CU "
                    "(8 waves/CU, 4 independent accumulator tiles per wave, ~0.2 s; `_data`: the same stream on random operands "
                    "instead of constants) and a 1 GiB -> 1 GiB copy kernel"}


def bench_asr_step(dev, steps=20, warmup=5):
    """BASELINE configs[1] (audio-only 12-layer Branchformer + Conv2dSubsampling + CTC + 6L decoder, batch 32 x 4 s, fwd+bwd,
    recipe dropout) under the headline's protocol - whole step captured as one hipGraph, W warm-up replays, K timed ones
    bracketed by synchronisation - so that the driver's record carries the audio-only step too; plus a few eager steps."""
    global WORKLOAD
    from tavsr import ops
    saved, WORKLOAD = WORKLOAD, "asr"
    try:
        torch.manual_seed(0)
        model = build_product_model().to(dev).train()
        batch = make_batch(B_PER_GPU, 1234, dev)
    finally:
        WORKLOAD = saved
    params = [p for p in model.parameters() if p.requires_grad]

    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(*batch)[0]
        loss.backward()
        return loss

    def run(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for _ in range(3):
        fwd_bwd()
    t_eager = run(fwd_bwd, 5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = fwd_bwd()      # noqa: F841
    run(graph.replay, warmup)
    t = run(graph.replay, steps)
    t_sus = run(graph.replay, max(steps, int(2.0 / t)))       # ~2 s more, back to back
    gf = GFLOP_PER_UTT_STEP["asr"]
    out = {"workload": "BASELINE configs[1]: audio-only 12-layer Branchformer d=256 + Conv2dSubsampling + CTC + 6L Transformer "
                       "decoder, batch 32 x 400 mel frames x 80, text length 40, fwd+bwd, dropout 0.1, hipGraph replay",
           "value": round(B_PER_GPU / t, 2), "unit": "utterances/s", "ms_per_step": round(1e3 * t, 3), "steps": steps, "warmup": warmup,
           "sustained": round(B_PER_GPU / t_sus, 2),
           "eager": {"value": round(B_PER_GPU / t_eager, 2), "ms_per_step": round(1e3 * t_eager, 3), "steps": 5},
           "gflop_per_utt_step": round(gf, 2),
           "frac_of_fp32_mfma_peak_whole_step": round(B_PER_GPU / t * gf / 1e3 / PEAK_FP32_MFMA_TFLOPS, 4)}
    del graph, static_loss, model
    torch.cuda.empty_cache()
    return out


DUMP_SAMPLE = 1 << 23       # gradient entries kept by --dump-outputs (32 MB of float32)


def dump_outputs(out_dir, loss, params):
    """What one step hands its caller, as float32 / float64 .npy files (about 32 MB in all):
      loss.npy        - the step's loss (float32, shape (1,));
      grad_norm.npy   - the L2 norm of every parameter's gradient, in model.parameters() order (float64);
      grad_sample.npy - every parameter's gradient flattened and concatenated in that order, all of it when it holds at most
                        DUMP_SAMPLE entries, else the entries at DUMP_SAMPLE fixed positions (ascending, drawn with seed 0).
    A parameter without a gradient counts as zeros of its size, so the positions stay aligned between builds."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    grads = [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params]
    flat = torch.cat(grads).float()
    if flat.numel() > DUMP_SAMPLE:
        idx = torch.randint(flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        flat = flat[idx.to(flat.device)]
    arrays = {"loss": loss.detach().float().reshape(1).cpu().numpy(),
              "grad_norm": torch.stack([g.double().norm() for g in grads]).cpu().numpy(),
              "grad_sample": flat.cpu().numpy()}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of one captured hipGraph per step")
    ap.add_argument("--split-backward", action="store_true",
                    help="replay the step as two hipGraphs around the model's dp.cut also with one rank (the N > 1 default)")
    ap.add_argument("--no-split-backward", action="store_true", help="N > 1: one hipGraph per step, all buckets leave after it")
    ap.add_argument("--force-rccl", action="store_true",
                    help="--gpus 1 only: drive a ONE-rank RCCL communicator through the whole exchange path (tavsr_dp_allreduce on the "
                         "communication stream, bucket pack / unpack, with --split-backward between the two graph replays) - a rehearsal "
                         "of the N > 1 step's plumbing on one GPU; the line says so in config.grad_exchange")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-dropout", action="store_true", help="all dropout rates 0 (the parity configuration)")
    ap.add_argument("--mode", choices=("step", "fwd-encoder"), default="step",
                    help="step: the fwd+bwd training step (the metric); fwd-encoder: ONLY the 12-layer encoder forward "
                         "measurement (north_star's >= 50 %% MFMA target), printed as its own JSON line (profiling runs)")
    ap.add_argument("--no-fwd-encoder", action="store_true", help="skip the fwd_encoder object of the default run")
    ap.add_argument("--no-eager", action="store_true", help="skip the eager (no-graph) timing beside the graph number")
    ap.add_argument("--no-asr", action="store_true", help="skip the `asr` object (BASELINE configs[1] step) of the default AV run")
    ap.add_argument("--no-decode", action="store_true", help="skip the `decode` object (BASELINE configs[4]: batch-1 p50 RTF, batch-64 utt/s)")
    ap.add_argument("--no-box", action="store_true", help="skip the `box` calibration object (fp32 MFMA microbench, HBM copy)")
    ap.add_argument("--workload", choices=("asr", "avsr"), default="avsr",
                    help="asr: BASELINE configs[1] (headline); avsr: configs[2] tailored AV-Branchformer incl. the visual frontend")
    ap.add_argument("--sustain-s", type=float, default=None,
                    help="after the timed steps keep stepping for this many seconds more and report that rate as `sustained` "
                         "(clocks settle within a few seconds of MFMA-dense load); 0 = off; default 12 with --full, else 0")
    ap.add_argument("--full", action="store_true",
                    help="also take every measurement beside the headline (box, eager, sustained, exposed exchange, roofline, "
                         "fwd_encoder, asr, decode, cpu_baseline; the --no-* options still drop single ones)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's loss and parameter gradients to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.sustain_s is None:
        args.sustain_s = 12.0 if args.full else 0.0
    global WORKLOAD, DROPOUT
    WORKLOAD = args.workload
    DROPOUT = not args.no_dropout

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU under torch.distributed.run) as a
        # CHILD process - nothing in this process has touched the GPU yet (no HIP call, the tavsr library is not loaded) - and
        # leave with its exit code; rank 0's JSON line reaches our stdout through the inherited descriptor.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))

    decode_obj = None
    if (args.full and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and WORKLOAD == "avsr" and args.mode == "step"
            and not args.no_decode and not args.no_fwd_encoder):
        # BASELINE configs[4] on the driver's record (replicas only; nothing to scale here), taken by a CHILD process BEFORE this process
        # touches the GPU.  A batch-1 search is a chain of ~140 dependent launches per token; it runs 11 - 19 % slower per token when a second
        # process holds a HIP context on the same GPU, idle or not (scripts/decode_after_load_probe.sh: 632 us per token alone, 693 beside an
        # idle process with 8 streams; behind this file's training legs as a child of this process: 749) - and 14 % slower inside a process
        # that has run the training legs.  Heat is not it: right behind 30 s of training steps a fresh process decodes at 629.  Never an exec.
        import subprocess
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_decode.py"), "--driver-record"], capture_output=True, text=True,
                               timeout=600, env=dict(os.environ))
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            decode_obj = json.loads(line[-1]) if r.returncode == 0 and line else {"error": (r.stderr or r.stdout)[-400:]}
        except Exception as e:      # noqa: BLE001 - the headline line must still be printed
            decode_obj = {"error": repr(e)[:400]}

    from tavsr import dp, ops

    rank, local, world = dp.init_from_env(force_rccl=args.force_rccl)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    if args.mode == "fwd-encoder":
        if rank == 0:
            print(json.dumps({"metric": "ms per forward of the 12-layer Branchformer encoder, batch 32 x 4 s (north_star target: "
                                        ">= 50 % of fp32 MFMA peak on the 254 GFLOP of the 12 layers)", "unit": "ms",
                              "n_gpus": 1, "higher_is_better": False, "data": "synthetic",
                              "fwd_encoder": bench_fwd_encoder(dev, args.steps, args.warmup)}), flush=True)
        return

    box = box_calibration(dev) if (args.full and rank == 0 and not args.no_box) else None      # before the model exists: the box, not the code
    if world > 1:
        torch.distributed.barrier()
    torch.manual_seed(0)
    model = build_product_model().to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    buckets = dp.GradBuckets(params)
    buckets.broadcast_parameters(0)
    buckets.attach_overlap_hooks()     # eager steps: a bucket's all-reduce leaves from a gradient hook, under the backward pass
    buckets.overlap = args.no_graph    # a captured step replays fwd+bwd as one hipGraph; its buckets leave right after the replay
    batch = make_batch(B_PER_GPU, 1234 + rank, dev)

    def fwd_bwd():
        for p in params:
            p.grad = None
        loss, _, _ = model(*batch)
        loss.backward()
        return loss

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            return float(t)
        return x

    eager_out = None
    # (1 GPU only: with N ranks the un-captured loop is measured by --no-graph; running hook-driven exchanges in front of the
    # capture made the gloo rehearsal's captured steps slower from step to step - 0.2 s, 1.7 s, 5.5 s of host time in the
    # exchange - so the N > 1 line keeps the order that was rehearsed: capture first, nothing before it)
    if args.full and not args.no_graph and not args.no_eager and world == 1:
        # the same step as eager launches (what a ragged, un-captured training loop pays): reported beside the graph number.
        # Taken BEFORE the capture, in the allocator / interpreter state a training loop would run in.
        n_eager = max(3, args.steps // 4)
        buckets.overlap = True

        def eager_step():
            buckets.begin_step()
            fwd_bwd()
            buckets.allreduce_mean()

        for _ in range(3):
            eager_step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(n_eager):
            eager_step()
        barrier()
        el = max_over_ranks(time.perf_counter() - t0)
        eager_out = {"value": round(B_PER_GPU * world * n_eager / el, 2), "unit": "utterances/s",
                     "ms_per_step": round(1e3 * el / n_eager, 3), "steps": n_eager}
        buckets.overlap = args.no_graph

    graph = None
    graph_b = None          # N > 1: the backward pass below the model's dp.cut as a second hipGraph
    n_ready = 0             # ... and the number of gradient buckets the first graph completes
    static_loss = None
    if not args.no_graph:
        # Capture the whole forward+backward (≈2.5k kernel launches) into one hipGraph: the step is
        # launch-bound in eager mode.  Gradients land in graph-owned buffers that are stable across replays.
        # With N > 1 ranks the step is TWO graphs (tavsr.dp.TwoPhaseBackward): forward + the backward pass above the model's cut
        # (AV: everything but the front-ends), then the rest.  The buckets complete after the first are packed and their
        # all-reduces enqueued on the communication stream before the second graph is replayed, so they run under it.
        two = dp.TwoPhaseBackward() if (world > 1 or args.split_backward) and not args.no_split_backward else None

        def fwd_bwd_capture():
            for p in params:
                p.grad = None
            if two is None:
                loss = model(*batch)[0]
                loss.backward()
                return loss, []
            with two.forward():
                loss = model(*batch)[0]
            late = two.late_params(params)
            two.phase_a(loss)
            two.phase_b()
            return loss, late

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                _, late = fwd_bwd_capture()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        for p in params:
            p.grad = None
        if two is not None and late:
            with torch.cuda.graph(graph):
                with two.forward():
                    static_loss = model(*batch)[0]
                two.phase_a(static_loss)
            graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_b, pool=graph.pool()):
                two.phase_b()
            n_ready = buckets.replan(late)      # the parameters below the cut: buckets of their own at the end of the issue order
            if rank == 0:
                print(f"[bench] two-graph step: {len(late)} of {len(params)} parameters below the cut, "
                      f"{n_ready} of {len(buckets.buckets)} buckets leave under the second graph", file=sys.stderr, flush=True)
        else:
            with torch.cuda.graph(graph):
                static_loss = model(*batch)[0]
                static_loss.backward()

    trace = os.environ.get("TAVSR_BENCH_TRACE") == "1"     # diagnostic: synchronous per-phase times of every step on stderr
    last = {"loss": static_loss}      # the loss of the latest step (eager: kept without its autograd graph)

    def step():
        t0 = time.perf_counter()
        if graph is not None:
            graph.replay()
            if graph_b is not None:
                buckets.launch_prefix(n_ready)     # their all-reduces run on the communication stream under the second graph
                graph_b.replay()
        else:
            buckets.begin_step()       # the hooks enqueue buckets under the backward pass
            last["loss"] = fwd_bwd().detach()
        if trace:
            if os.environ.get("TAVSR_BENCH_TRACE_SYNC", "1") == "1":
                torch.cuda.synchronize()
            t1 = time.perf_counter()
        buckets.allreduce_mean()
        if trace:
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            print(f"[rank {rank}] step: compute {1e3 * (t1 - t0):.1f} ms, exchange {1e3 * (t2 - t1):.1f} ms, "
                  f"drain {1e3 * (time.perf_counter() - t2):.1f} ms", file=sys.stderr, flush=True)

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last["loss"], params)      # (N > 1: the gradients after the exchange)

    sustained = None
    if args.sustain_s > 0:
        # the same step, replayed for >= --sustain-s seconds more: the rate the chip holds once its clocks have settled
        n_sus = max(args.steps, int(args.sustain_s / (elapsed / args.steps)) + 1)
        barrier()
        t0 = time.perf_counter()
        for _ in range(n_sus):
            step()
        barrier()
        el_s = max_over_ranks(time.perf_counter() - t0)
        sustained = {"value": round(B_PER_GPU * world * n_sus / el_s, 2), "unit": "utterances/s", "steps": n_sus,
                     "ms_per_step": round(1e3 * el_s / n_sus, 3), "seconds": round(el_s, 2),
                     "note": "same step, run back to back right after the timed region"}
    exposed_ms = None
    if args.full and (world > 1 or dp.FORCE_WORLD1):
        # stream time of the exchange that nothing hides (pack + all-reduce + unpack behind the last gradient): a few steps
        # with one event pair each, outside the timed region
        pairs = []
        for _ in range(5):
            if graph is not None:
                graph.replay()
                if graph_b is not None:
                    buckets.launch_prefix(n_ready)
                    graph_b.replay()
            else:
                buckets.begin_step()
                fwd_bwd()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            buckets.allreduce_mean()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        exposed_ms = max_over_ranks(sorted(a.elapsed_time(b) for a, b in pairs)[len(pairs) // 2])

    utts = B_PER_GPU * world * args.steps
    value = utts / elapsed
    out = {
        "metric": ("utterances/sec fwd+bwd, 12L tailored AV-Branchformer (Conv3d+ResNet-18 lip frontend, fusion, CTC+6L decoder), "
                   "4 s clips, batch 32/GPU") if WORKLOAD == "avsr" else
                  "utterances/sec fwd+bwd, 12L Branchformer ASR (Conv2dSubsampling+CTC+6L decoder), 4 s clips, batch 32/GPU",
        "value": round(value, 2), "unit": "utterances/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("BASELINE configs[2]: tailored AV-Branchformer 12L (400 mel frames x 80 + 100 lip frames 88x88, "
                                "Conv3d+ResNet-18 frontend, adaptive fusion), CTC/attention joint loss, batch 32 per GPU, fwd+bwd")
                   if WORKLOAD == "avsr" else
                   "BASELINE configs[1]: audio-only 12-layer Branchformer d=256 + Conv2dSubsampling + CTC + "
                   "6L Transformer decoder, batch 32 x 400 mel frames x 80 per GPU, text length 40, fwd+bwd",
                   "global_batch": B_PER_GPU * world, "parallelism": f"dp{world}",
                   "dropout": 0.1 if DROPOUT else 0.0,
                   "launch": "eager" if graph is None else ("hipGraph replay (whole fwd+bwd)" if graph_b is None else
                                                            f"two hipGraphs (fwd + upper bwd | lower bwd), {n_ready} of "
                                                            f"{len(buckets.buckets)} buckets exchanged under the second"),
                   "grad_exchange": ("tavsr_dp_allreduce (RCCL, world 1: one-GPU rehearsal of the exchange path), 64 MB flat buckets"
                                     if dp.FORCE_WORLD1 else "none (1 GPU)" if world == 1 else
                                     ("tavsr_dp_allreduce (RCCL, C ABI)" if dp.RCCL_ABI else
                                      f"torch.distributed all_reduce ({'RCCL' if torch.distributed.get_backend() == 'nccl' else torch.distributed.get_backend()})")
                                     + (", staged through pinned host buffers" if torch.distributed.get_backend() == "gloo"
                                        and dp.GLOO_HOST_STAGED and not dp.RCCL_ABI else "")
                                     + ", 64 MB flat buckets")},
        "hbm_peak_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1),
        "model_tflops_per_s": round(value * GFLOP_PER_UTT_STEP[WORKLOAD] / 1e3, 2),
        "frac_of_fp32_mfma_peak_whole_step": round(value * GFLOP_PER_UTT_STEP[WORKLOAD] / 1e3 / (PEAK_FP32_MFMA_TFLOPS * world), 4),
        "gflop_per_utt_step": round(GFLOP_PER_UTT_STEP[WORKLOAD], 2),
    }
    # what the exchange really ran on: ranks of the C ABI's RCCL communicator (0: none), ranks torch.distributed sees, peak HBM per rank
    out.update(dp.world_report(torch.cuda.max_memory_allocated()))
    if sustained is not None:
        out["sustained"] = sustained
    if exposed_ms is not None:
        out["grad_exchange_exposed_ms_per_step"] = round(exposed_ms, 3)

    if eager_out is not None:
        out["eager"] = eager_out

    buckets.overlap = False       # the legs below run on rank 0 alone: no collective may leave from a hook
    if args.full and rank == 0 and not args.no_roofline:
        # Instrumented eager replay of the same step: HIP events around every tavsr_gemm launch on the launch stream.
        prof = ops.GemmProfile()
        ops.PROFILE = prof
        nprof = 3
        for _ in range(nprof):
            fwd_bwd()
        ops.PROFILE = None
        summ = prof.summary()
        key = max(summ, key=lambda k: summ[k]["seconds"])
        d = summ[key]
        achieved = d["flops"] / d["seconds"] / 1e12
        gemm_s = sum(v["seconds"] for v in summ.values()) / nprof
        out["roofline"] = {
            "bound": "mfma", "kernel": key, "achieved": round(achieved, 2), "peak": PEAK_FP32_MFMA_TFLOPS,
            "unit": "TFLOP/s", "frac": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": hbm_traffic(key),
            "launches_per_step": d["calls"] // nprof,
            "avg_launch_us": round(1e6 * d["seconds"] / d["calls"], 2),
            "algorithmic_gflop_per_launch": round(d["flops"] / d["calls"] / 1e9, 4),
            "algorithmic_bytes_per_launch": round(d["bytes"] / d["calls"]),   # every operand and the output once
            "all_gemm_ms_per_step": round(1e3 * gemm_s, 3),
            "all_gemm_tflops": round(sum(v["flops"] for v in summ.values()) / nprof / gemm_s / 1e12, 2),
            "by_kernel": {k: {"calls_per_step": v["calls"] // nprof, "ms_per_step": round(1e3 * v["seconds"] / nprof, 3),
                              "tflops": round(v["flops"] / v["seconds"] / 1e12, 2)} for k, v in summ.items()},
        }
    if args.full and rank == 0 and world == 1 and not args.no_fwd_encoder:
        del graph, graph_b, static_loss
        for p in params:
            p.grad = None
        model = None
        torch.cuda.empty_cache()
        out["fwd_encoder"] = bench_fwd_encoder(dev)
        if WORKLOAD == "avsr" and not args.no_asr:
            out["asr"] = bench_asr_step(dev)
    if decode_obj is not None and rank == 0:
        out["decode"] = decode_obj
    if box is not None:
        out["box"] = box
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
        if "asr" in out:
            out["asr"]["cpu_baseline"] = cpu_baseline(budget_s=8.0, workload="asr", bs=4)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        dp.shutdown()
    elif dp.FORCE_WORLD1:
        torch.cuda.synchronize()
        dp.shutdown()


if __name__ == "__main__":
    main()
