"""Language-model training step on one MI355X: the recipe LM (configs/lm/lm_english.yaml: 16 layers x 512, 8 heads, 2048 units,
V = 41) on synthetic ids with a fixed length mix, forward + backward + FusedAdam step, eager and with the forward + backward
replayed as one graph (the FusedAdam update is launched behind the replay: its step count is a host argument of the launch).

Prints a short table and one JSON line: tokens/s (real tokens: sum(len + 1)), ms per step, achieved TFLOP/s against the fp32
MFMA peak bench.py uses, and the CPU oracle's tokens/s on 16 threads (same model, same arithmetic, torch on the host, a slice of
the batch).  The TFLOP/s figure counts the matrix work of the rows the kernels process (B x (W + 1), padding included):
3 x (2 x matrix parameters per row + the causal attention products), the usual forward + backward count.

    python bench_lm.py [--steps 20] [--warmup 3] [--batch 64] [--mode both|eager|graph] [--no-oracle] [--layers N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tailored-avsr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3      # bench.py: v_mfma_f32_32x32x2_f32, 256 CU x 256 FLOP/clk x 2.4 GHz
LENGTH_MIX = (200, 180, 150, 120, 100, 90, 64, 40)      # tokens per sentence, cycled over the batch: W = 200, 59 % real rows


def batch_of(B, V, seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([LENGTH_MIX[b % len(LENGTH_MIX)] for b in range(B)], dtype=torch.int64)
    text = torch.randint(1, V - 1, (B, max(LENGTH_MIX)), generator=g, dtype=torch.int64)
    for b in range(B):
        text[b, int(lens[b]):] = -1
    return text, lens


def gflop_per_step(conf, V, B, L):
    """forward + backward matrix work of B rows of L positions, GFLOP"""
    c = conf["lm_conf"]
    D, K, E, nb = c["att_unit"], c["unit"], c["embed_unit"], c["layer"]
    per_row = 2 * (E * D + nb * (4 * D * D + 2 * D * K) + D * V)
    attn = nb * 4 * D * (L + 1) / 2                      # q k^T and p v over the causal half, per row on average
    return 3 * B * L * (per_row + attn) / 1e9


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def oracle_tokens_per_s(conf, V, state, text, lens, steps=2):
    """the CPU oracle (oracle.beam_search.TransformerLMOracle, fp32, at most 16 threads) on the same step"""
    import torch.nn.functional as F
    from oracle.beam_search import TransformerLMOracle
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lm = TransformerLMOracle(V, **conf["lm_conf"]).train()
    lm.load_state_dict({k[3:]: v for k, v in state.items()})
    opt = torch.optim.Adam(lm.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    B, W = text.shape
    x = torch.zeros((B, W + 1), dtype=torch.int64)
    t = torch.full((B, W + 1), -1, dtype=torch.int64)
    x[:, 0] = V - 1
    for b in range(B):
        n = int(lens[b])
        x[b, 1: n + 1] = text[b, :n]
        t[b, :n] = text[b, :n]
        t[b, n] = V - 1
    ntok = int(lens.sum()) + B

    def step():
        opt.zero_grad()
        y, _ = lm(x, None)
        loss = F.cross_entropy(y.view(-1, V), t.view(-1), ignore_index=-1, reduction="sum") / ntok
        loss.backward()
        opt.step()
        return float(loss.detach())

    step()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    return ntok * steps / (time.perf_counter() - t0), loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="sentences per step (default: the recipe's training batch size)")
    ap.add_argument("--layers", type=int, default=None, help="override lm_conf.layer (quick runs)")
    ap.add_argument("--mode", choices=("both", "eager", "graph"), default="both")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--oracle-batch", type=int, default=8)
    args = ap.parse_args()

    from tavsr.tasks.lm import LMTask
    from tavsr.train import FusedAdam
    conf = yaml.safe_load(open(os.path.join(ROOT, "tailored-avsr_amd", "configs", "lm", "lm_english.yaml")))
    if args.layers:
        conf["lm_conf"]["layer"] = args.layers
    B = args.batch or conf["training_settings"]["batch_size"]
    torch.manual_seed(0)
    model = LMTask.build_model(argparse.Namespace(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in conf.items()}))
    V = model.lm.decoder.weight.shape[0]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    text, lens = batch_of(B, V)
    W = text.shape[1]
    ntok = int(lens.sum()) + B
    gf = gflop_per_step(conf, V, B, W + 1)
    text_d, lens_d = text.cuda(), lens.cuda()
    opt = FusedAdam(model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    params = list(model.parameters())
    c = conf["lm_conf"]
    head = (f"LM training step, {c['layer']} layers x {c['att_unit']}, {c['head']} heads, {c['unit']} units, embed {c['embed_unit']}, V = {V}, f32; "
            f"{B} sentences of {'/'.join(str(l) for l in LENGTH_MIX)} tokens: {B} x {W + 1} = {B * (W + 1)} rows, {ntok} real tokens "
            f"({100.0 * ntok / (B * (W + 1)):.0f} %); {gf:.0f} GFLOP per step over all rows")
    print(head)
    res = {"workload": "lm_train", "layers": c["layer"], "batch": B, "rows": B * (W + 1), "tokens_per_step": ntok,
           "gflop_per_step": round(gf, 1), "peak_tflops": PEAK_FP32_MFMA_TFLOPS, "steps": args.steps}
    last = {}

    def report(name, s):
        tf = gf / s / 1e3
        res[name] = {"ms_per_step": round(1e3 * s, 3), "tokens_per_s": round(ntok / s, 1), "tflops": round(tf, 2),
                     "frac_of_fp32_mfma_peak": round(tf / PEAK_FP32_MFMA_TFLOPS, 4), "loss": round(float(last["loss"]), 5)}
        print(f"  {name:<6} {1e3 * s:9.3f} ms / step  {ntok / s:12.0f} tokens/s  {tf:7.2f} TFLOP/s = "
              f"{100 * tf / PEAK_FP32_MFMA_TFLOPS:5.1f} % of the fp32 MFMA peak ({PEAK_FP32_MFMA_TFLOPS})   loss {float(last['loss']):.4f}")

    if args.mode in ("both", "eager"):
        def eager():
            opt.zero_grad()
            loss = model(text_d, lens_d)[0]
            loss.backward()
            opt.step()
            last["loss"] = loss.detach()
        report("eager", timed(eager, args.steps, args.warmup))

    if args.mode in ("both", "graph"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                opt.zero_grad()
                model(text_d, lens_d)[0].backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = model(text_d, lens_d)[0]
            static_loss.backward()
        last["loss"] = static_loss.detach()

        def replay():
            graph.replay()
            opt.step()
        report("graph", timed(replay, args.steps, args.warmup))

    if not args.no_oracle:
        nb = min(B, args.oracle_batch)
        tps, loss = oracle_tokens_per_s(conf, V, state, text[:nb], lens[:nb])
        res["cpu_oracle"] = {"tokens_per_s": round(tps, 1), "threads": torch.get_num_threads(), "sentences": nb}
        print(f"  CPU oracle (torch, fp32, {torch.get_num_threads()} threads, {nb} sentences of the batch): {tps:10.0f} tokens/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
