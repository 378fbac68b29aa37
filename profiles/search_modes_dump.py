"""Every route of the beam search (tavsr/inference/beam_search.py) on the small models of tests/test_gpu_search_modes.py, fixed
inputs, results written as JSON (token lists, scores as float32 hex bits, tokens searched) - run once on each of two versions of the
search and compare: a refactor of the search must leave the two files identical.

The matrix is the cross product of: model (hybrid, CTC only, attention only) x LM (with, without) x ctc_weight (0, 0.3, 1.0; a
combination the search refuses is recorded as refused) x skip_zero_weight x maxlenratio (0, -12, 0.5) x GRAPH_STEP x CTC_BESIDE_SCORERS
x PREBEAM_FUSED x CTC_SEARCH_FUSED x SINGLE_STREAM.  Beam 5, lm_weight 0.6, length bonus 0.5; three utterances of 25 / 20 / 14 encoder
frames.  Every case decodes twice on one search object (the second call re-uses the first one's capture).

usage: python profiles/search_modes_dump.py OUT.json [I/N]      (shard I of N: every N-th case; the shards' files are merged by --cmp)
       python profiles/search_modes_dump.py --cmp A.json[,A2.json...] B.json[,B2.json...] [REPORT.txt]"""
import argparse
import itertools
import json
import os
import struct
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tailored-avsr_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)


def compare(a_files, b_files, report):
    def load(files):
        out = {}
        for f in files.split(","):
            out.update(json.load(open(f)))
        return out
    a, b = load(a_files), load(b_files)
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    refused = sum(1 for v in a.values() if v == "refused")
    text = (f"search_modes_dump: {len(a)} cases in A ({refused} refused by the search), {len(b)} in B, two decodes each; "
            f"{len(diff)} differ\n" + "".join(f"  differs: {k}\n" for k in diff[:50]))
    print(text, end="")
    if report:
        open(report, "w").write(text)
    return 1 if diff or not a else 0


def main(out_path, shard):
    import torch

    from helpers import TOKENS_EN, asr_conf
    from oracle.model import fill_parameters_, synth
    from tavsr import _lib
    from tavsr.inference import beam_search as PBS
    from tavsr.lm.transformer_lm import TransformerLM
    from tavsr.tasks.asr import ASRTask

    def model(model_ctc_weight):
        conf = asr_conf(num_blocks=2, dec_blocks=2)
        if model_ctc_weight is not None:
            conf["model_conf"]["ctc_weight"] = model_ctc_weight
        conf["token_list"] = TOKENS_EN
        pm = ASRTask.build_model(argparse.Namespace(**conf)).eval()
        fill_parameters_(pm, seed=5)
        return pm.cuda()

    models = dict(hybrid=model(None), ctc_only=model(1.0), att_only=model(0.0))
    lm = TransformerLM(len(TOKENS_EN), pos_enc=None, embed_unit=32, att_unit=64, head=4, unit=128, layer=2, dropout_rate=0.0).eval()
    fill_parameters_(lm, seed=6)
    lm = lm.cuda()
    with torch.no_grad():
        enc, olens = models["hybrid"].encode(synth((3, 104, 80), seed=7).cuda(), torch.tensor([104, 80, 56]).cuda())
    assert olens.tolist() == [25, 20, 14], olens
    flags = ("GRAPH_STEP", "CTC_BESIDE_SCORERS", "PREBEAM_FUSED", "CTC_SEARCH_FUSED")
    axes = [list(models), [True, False], [0.0, 0.3, 1.0], [False, True], [0.0, -12, 0.5]] + [[True, False]] * 5
    i, n = (int(v) for v in shard.split("/"))
    out = {}
    for c, (name, with_lm, ctc_w, skip, ratio, *sw) in enumerate(itertools.product(*axes)):
        if c % n != i:
            continue
        case = f"{name} lm={int(with_lm)} ctc_w={ctc_w} skip={int(skip)} ratio={ratio} " + " ".join(
            f"{k}={int(v)}" for k, v in zip(flags + ("SINGLE_STREAM",), sw))
        for k, v in zip(flags, sw):
            setattr(PBS, k, v)
        _lib.SINGLE_STREAM = sw[4]
        try:
            search = PBS.BatchBeamSearch(models[name], lm if with_lm else None, 5, ctc_w, 0.6, 0.5, maxlenratio=ratio, skip_zero_weight=skip)
        except ValueError:
            out[case] = "refused"
            continue
        runs = []
        for _ in range(2):
            hyps = search.decode(enc, olens)
            runs.append(dict(n_steps=search.n_steps,
                             hyps=[[(ys, struct.pack("<f", sc).hex()) for ys, sc in u] for u in hyps]))
        out[case] = runs
        if len(out) % 100 == 0:
            print(f"{len(out)} cases", flush=True)
    json.dump(out, open(out_path, "w"))
    print(f"wrote {len(out)} cases to {out_path}")


if __name__ == "__main__":
    if sys.argv[1] == "--cmp":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "0/1")
