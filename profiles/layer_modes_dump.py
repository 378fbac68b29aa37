"""Every route of the encoder layers' sequencing (tavsr/functional.py BranchformerLayerFn, tavsr/functional_av.py TailoredLayerFn; the C
sequencers of csrc/layer.hip where they apply) on small encoders with fixed weights and inputs, results written as JSON (sha256 of the
bytes of the output, of the input gradient, of weight_global / weight_local and of every parameter gradient) - run once on each of two
versions of the package and compare: a refactor of the sequencing must leave the two files identical.

Branchformer cases (MyBranchformerEncoder, two layers, d_model 256, 4 heads, train mode), the cross product of: merge form (learned_ave,
fixed_ave 0.3 / 0.0 / 1.0, concat, learned_ave with attn_branch_drop_rate 1.0) x dropout (0, 0.1) x (B, T) in ((1, 5), (3, 40) ragged,
(2, 150) ragged: T <= 128 and T > 128 take different merge launches) x ops.LAYER_C x ops.ATTN_FUSED x ops.CSGU_FUSED x ops.MERGE_PROJ x
ops.WGRAD_BESIDE x functional._POS_DW_BESIDE x _lib.SINGLE_STREAM; plus, per merge form, shape and LAYER_C, one forward with dropout 0.1
under torch.no_grad() (nothing saved for a backward).  Tailored cases (TailoredEncoder, one layer, B 3, T 50, ragged): the four
(acoustic_use_attn, visual_use_attn) pairs x dropout (0, 0.1) x LAYER_C x ATTN_FUSED x CSGU_FUSED x ops.BLOCKS_C.

usage: python profiles/layer_modes_dump.py OUT.json [I/N]      (shard I of N: every N-th case; the shards' files are merged by --cmp)
       python profiles/layer_modes_dump.py --cmp A.json[,A2.json...] B.json[,B2.json...] [REPORT.txt]"""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tailored-avsr_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

FORMS = [("learned_ave", 0.5, 0.0), ("fixed_ave", 0.3, 0.0), ("fixed_ave", 0.0, 0.0), ("fixed_ave", 1.0, 0.0), ("concat", 0.5, 0.0),
         ("learned_ave", 0.5, 1.0)]
SHAPES = [(1, 5, (5,)), (3, 40, (40, 27, 20)), (2, 150, (150, 97))]
BF_SWITCHES = ("LAYER_C", "ATTN_FUSED", "CSGU_FUSED", "MERGE_PROJ", "WGRAD_BESIDE", "_POS_DW_BESIDE", "SINGLE_STREAM")
AV_SWITCHES = ("LAYER_C", "ATTN_FUSED", "CSGU_FUSED", "BLOCKS_C")


def compare(a_files, b_files, report):
    def load(files):
        out = {}
        for f in files.split(","):
            out.update(json.load(open(f)))
        return out
    a, b = load(a_files), load(b_files)
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    cases = [k for k in a if not k.startswith("names ")]
    text = (f"layer_modes_dump: {len(cases)} cases in A ({sum(k.startswith('bf ') for k in cases)} Branchformer, "
            f"{sum(k.startswith('bf-nograd ') for k in cases)} without grad, {sum(k.startswith('av ') for k in cases)} tailored), "
            f"{len(b) - (len(a) - len(cases))} in B, {sum(len(a[k]) for k in cases)} digests; {len(diff)} cases differ\n")
    for k in diff[:50]:
        va, vb = a.get(k), b.get(k)
        where = "missing on one side" if va is None or vb is None else [i for i, (x, y) in enumerate(zip(va, vb)) if x != y][:8]
        text += f"  differs: {k}: entries {where}\n"
    print(text, end="")
    if report:
        open(report, "w").write(text)
    return 1 if diff or not a else 0


def main(out_path, shard):
    import torch

    from oracle.model import fill_parameters_, synth
    from tavsr import _lib, ops
    from tavsr import functional as F_
    from tavsr.encoder.audiovisual.tailored.encoder import TailoredEncoder
    from tavsr.encoder.branchformer.encoder import MyBranchformerEncoder
    from tavsr.layers import RelPositionalEncoding

    D = 256
    pe = RelPositionalEncoding(D, 0.0)
    out = {}

    def switch(name, on):
        if name == "SINGLE_STREAM":
            _lib.SINGLE_STREAM = on
        else:
            setattr(F_ if name == "_POS_DW_BESIDE" else ops, name, on)

    def digests(tensors):
        """sha256 (first 16 hex digits) of each tensor's bytes through ONE device-to-host copy; None and plain floats by value"""
        live = [t for t in tensors if torch.is_tensor(t)]
        host = torch.cat([t.detach().reshape(-1).float() for t in live]).cpu().numpy() if live else None
        res, o = [], 0
        for t in tensors:
            if not torch.is_tensor(t):
                res.append(repr(t))
                continue
            res.append(hashlib.sha256(host[o: o + t.numel()].tobytes()).hexdigest()[:16])
            o += t.numel()
        return res

    def inputs(B, T, lens, seed):
        x, pos = pe(synth((B, T, D), seed=seed).cuda())
        lens = torch.tensor(lens, device="cuda")
        return x.detach(), pos, (torch.arange(T, device="cuda")[None, :] < lens[:, None])[:, None, :]

    i, n = (int(v) for v in shard.split("/"))
    c = 0

    def mine():
        nonlocal c
        c += 1
        return (c - 1) % n == i

    bf_in = {(B, T): inputs(B, T, lens, 8) for B, T, lens in SHAPES}
    bf_dy = {(B, T): synth((B, T, D), seed=10).cuda() for B, T, _ in SHAPES}
    for fi, (merge, cgw, abd) in enumerate(FORMS):
        for p in (0.0, 0.1):
            enc = MyBranchformerEncoder(input_size=D, output_size=D, attention_heads=4, num_blocks=2, input_layer=None, dropout_rate=p,
                                        positional_dropout_rate=0.0, attention_dropout_rate=p, ffn_activation_type="swish",
                                        merge_method=merge, cgmlp_weight=cgw, attn_branch_drop_rate=abd)
            fill_parameters_(enc, seed=17)
            enc = enc.cuda().train()
            named = sorted(enc.named_parameters())
            out[f"names bf form={fi}"] = ["y", "dx"] + [f"layer{j}.{w}" for j in range(2) for w in ("weight_global", "weight_local")] + \
                                         [k for k, _ in named]

            def run(B, T, grad):
                x, pos, mask = bf_in[(B, T)]
                xs = x.clone().requires_grad_(grad)
                enc.zero_grad(set_to_none=True)
                for layer in enc.encoders:
                    layer.weight_global = layer.weight_local = None
                ops.manual_seed(123)
                h, m = (xs, pos), mask
                with torch.set_grad_enabled(grad):
                    for layer in enc.encoders:
                        h, m = layer(h, m)
                if grad:
                    (h[0] * bf_dy[(B, T)]).sum().backward()
                torch.cuda.synchronize()
                return digests([h[0], xs.grad] + [w for layer in enc.encoders for w in (layer.weight_global, layer.weight_local)] +
                               [q.grad for _, q in named])

            for (B, T, _), *sw in itertools.product(SHAPES, *[[True, False]] * len(BF_SWITCHES)):
                if not mine():
                    continue
                for k, v in zip(BF_SWITCHES, sw):
                    switch(k, v)
                out[f"bf form={fi} p={p} B={B} T={T} " + " ".join(f"{k}={int(v)}" for k, v in zip(BF_SWITCHES, sw))] = run(B, T, True)
            for k in BF_SWITCHES:
                switch(k, k != "SINGLE_STREAM")
            if p > 0.0:
                for (B, T, _), layer_c in itertools.product(SHAPES, [True, False]):
                    if not mine():
                        continue
                    ops.LAYER_C = layer_c
                    out[f"bf-nograd form={fi} p={p} B={B} T={T} LAYER_C={int(layer_c)}"] = run(B, T, False)
                ops.LAYER_C = True
        print(f"form {fi}: {len(out)} entries", flush=True)

    B, T = 3, 50
    xa, pos, am = inputs(B, T, (50, 37, 20), 11)
    xv, _, vm = inputs(B, T, (50, 50, 31), 12)
    dya, dyv = synth((B, T, D), seed=13).cuda(), synth((B, T, D), seed=14).cuda()
    for (ua, uv), p in itertools.product([(True, False), (False, True), (True, True), (False, False)], (0.0, 0.1)):
        enc = TailoredEncoder("rel_pos", "latest", num_blocks=1, dropout_rate=p, positional_dropout_rate=0.0, attention_dropout_rate=p,
                              acoustic_use_attn=[ua], visual_use_attn=[uv])
        fill_parameters_(enc, seed=19)
        layer = enc.cuda().train().encoders[0]
        named = sorted(layer.named_parameters())
        out[f"names av ua={int(ua)} uv={int(uv)}"] = ["ya", "yv", "dxa", "dxv"] + [k for k, _ in named]
        for sw in itertools.product(*[[True, False]] * len(AV_SWITCHES)):
            if not mine():
                continue
            for k, v in zip(AV_SWITCHES, sw):
                switch(k, v)
            a, v = xa.clone().requires_grad_(True), xv.clone().requires_grad_(True)
            layer.zero_grad(set_to_none=True)
            ops.manual_seed(321)
            ops.rng_step_begin(a.device)
            (ya, _), _, (yv, _), _ = layer((a, pos), am, (v, pos), vm)
            ((ya * dya).sum() + (yv * dyv).sum()).backward()
            torch.cuda.synchronize()
            out[f"av ua={int(ua)} uv={int(uv)} p={p} " + " ".join(f"{k}={int(v_)}" for k, v_ in zip(AV_SWITCHES, sw))] = digests(
                [ya, yv, a.grad, v.grad] + [q.grad for _, q in named])
        for k in AV_SWITCHES:
            switch(k, True)
    json.dump(out, open(out_path, "w"))
    print(f"wrote {len(out)} entries to {out_path}")


if __name__ == "__main__":
    if sys.argv[1] == "--cmp":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "0/1")
