"""GPU: ``python -m tavsr.lm_main`` in-process on a tiny recipe and a ten-sentence text file - the epoch loop, the checkpoints, the
average of the best ones and the evaluation mode."""
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

SENTENCES = ["hello world", "it's nine o'clock", "a", "the quick brown fox", "jumps over {the} lazy dog", "42 is the answer",
             "language models score text", "one more line", "short", "the last sentence of the file"]


def test_lm_main_trains_saves_averages_and_evaluates(tmp_path, capsys):
    from tavsr import lm_main
    conf = dict(lm="transformer", lm_conf=dict(att_unit=64, dropout_rate=0.1, embed_unit=32, head=4, layer=1, pos_enc=None, unit=128),
                model_conf=dict(ignore_id=-1), token_list="char/english", token_type="char", bpemodel=None, init=None,
                training_settings=dict(batch_size=4, num_workers=0, optimizer="adamw", scheduler="onecycle", learning_rate=0.01, epochs=3,
                                       accum_grad=2),
                epochs=3, accum_grad=2, average_epochs=2, device="cuda", dtype="float32")
    recipe, text, out = tmp_path / "lm.yaml", tmp_path / "text.txt", str(tmp_path / "out")
    recipe.write_text(yaml.safe_dump(conf))
    text.write_text("\n".join(SENTENCES))
    data = ["--training-dataset", str(text), "--validation-dataset", str(text), "--test-dataset", str(text)]
    lm_main.main(["--lm-config-file", str(recipe), "--mode", "training", "--output-dir", out] + data)
    log = capsys.readouterr().out
    epochs = [l for l in log.splitlines() if l.startswith("Epoch ")]
    assert len(epochs) == 3 and all("TRAIN LOSS=" in l and "VAL LOSS=" in l and "TEST LOSS=" in l for l in epochs)
    val = [float(l.split("VAL LOSS=")[1].split(" ")[0]) for l in epochs]
    assert all(v == round(v, 3) for v in val) and val[-1] < val[0]                      # 3 decimals; three epochs on ten sentences learn something
    paths = [os.path.join(out, "models", f"model_{s}.pth") for s in ("001", "002", "003", "average")]
    assert all(os.path.exists(p) for p in paths) and os.path.exists(os.path.join(out, "val_stats.csv"))
    states = [torch.load(p, map_location="cpu") for p in paths]
    best = sorted(range(3), key=lambda i: val[i])[:2]
    for k, avg in states[3].items():
        want = (states[best[0]][k] + states[best[1]][k]) / 2
        assert torch.allclose(avg, want, rtol=1e-6, atol=1e-7), k
    lm_main.main(["--lm-config-file", str(recipe), "--mode", "evaluation", "--load-lm", paths[2], "--output-dir", out] + data)
    log = capsys.readouterr().out
    line = [l for l in log.splitlines() if l.startswith("VAL LOSS=")]
    assert len(line) == 1 and float(line[0].split("VAL LOSS=")[1].split(" ")[0]) == val[2]
