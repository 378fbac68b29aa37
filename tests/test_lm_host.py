"""Host side of language-model training: the plain-Python ``lm_shift`` (tests/lm_ref.py) against hand-written rows, the text
dataset and its collate function, the recipe keys, and the two loops of ``tavsr.train`` on a stub model."""
import argparse
import os

import pytest
import torch
import yaml

import lm_ref as R
from helpers import ROOT, TOKENS_EN

LM_DIR = os.path.join(ROOT, "tailored-avsr_amd", "configs", "lm")


def test_lm_shift_reference_against_hand_written_rows():
    text = [[5, 6, 7, -1], [9, -1, -1, -1], [1, 2, 3, 4], [-1, -1, -1, -1]]
    x, t, xl, n = R.lm_shift(text, [3, 1, 4, 0], 40)
    assert x.tolist() == [[40, 5, 6, 7, 0], [40, 9, 0, 0, 0], [40, 1, 2, 3, 4], [40, 0, 0, 0, 0]]
    assert t.tolist() == [[5, 6, 7, 40, -1], [9, 40, -1, -1, -1], [1, 2, 3, 4, 40], [40, -1, -1, -1, -1]]
    assert xl.tolist() == [4, 2, 5, 1] and n.tolist() == [4, 2, 5, 1]
    assert xl.dtype == torch.int64 and n.dtype == torch.int32 and x.dtype == t.dtype == torch.int64
    for pad in (0, 7):          # the rows are delimited by the lengths: the pad value never shows
        other = [[pad if v == -1 else v for v in row] for row in text]
        for a, b in zip(R.lm_shift(other, [3, 1, 4, 0], 40), (x, t, xl, n)):
            assert torch.equal(a, b)
    xw, tw, _, _ = R.lm_shift(text, [3, 1, 4, 0], 40, width=7)      # nll(max_length=6)
    assert torch.equal(xw[:, :5], x) and torch.equal(tw[:, :5], t) and int(xw[:, 5:].abs().sum()) == 0 and bool((tw[:, 5:] == -1).all())


def test_lm_dataset_reads_text_files_and_split_csvs(tmp_path):
    from tavsr.datasets import LMDataset
    raw = tmp_path / "train.txt"
    raw.write_text("hello {world}\n  it's 9 o'clock  \nlast line", encoding="utf-8")
    ds = LMDataset(str(raw), from_dataset_partition=False)
    assert len(ds) == 3 and [ds[i] for i in range(3)] == ["HELLO WORLD", "IT'S 9 O'CLOCK", "LAST LINE"]
    paths = []
    for i, s in enumerate(("first {sample}\nsecond line is ignored\n", "another one\n")):
        p = tmp_path / f"s{i}.txt"
        p.write_text(s)
        paths.append(str(p))
    split = tmp_path / "split.csv"
    split.write_text("video_path,audio_path,transcription_path\n" + "".join(f"v{i}.mp4,a{i}.wav,{p}\n" for i, p in enumerate(paths)))
    ds = LMDataset(str(split), from_dataset_partition=True)
    assert len(ds) == 2 and [ds[0], ds[1]] == ["FIRST SAMPLE", "ANOTHER ONE"]


def _tok():
    from tavsr.lm_main import get_tokenizer_converter
    return get_tokenizer_converter("char", None, list(TOKENS_EN))


@pytest.mark.parametrize("ignore_id", [-1, 0])
def test_lm_data_processing_pads_with_the_ignore_id(ignore_id):
    from tavsr.utils.lm_dataloader import lm_data_processing
    tokenizer, converter = _tok()
    data = ["AB C", "Z", "IT'S 42"]
    x, ilens, refs = lm_data_processing(data, tokenizer, converter, ignore_id)
    ids = {t: i for i, t in enumerate(TOKENS_EN)}
    want = [[ids["A"], ids["B"], ids["<space>"], ids["C"]], [ids["Z"]],
            [ids["I"], ids["T"], ids["'"], ids["S"], ids["<space>"], ids["4"], ids["2"]]]
    assert x.dtype == torch.int64 and ilens.dtype == torch.int64 and x.shape == (3, 7)
    assert ilens.tolist() == [4, 1, 7] and refs == data
    for row, w in zip(x.tolist(), want):
        assert row == w + [ignore_id] * (7 - len(w))
    assert converter.tokens2ids(tokenizer.text2tokens("a")) == [ids["<unk>"]]


def test_get_lm_dataloader_takes_its_settings_from_the_recipe(tmp_path):
    from tavsr.utils.lm_dataloader import get_lm_dataloader
    raw = tmp_path / "train.txt"
    raw.write_text("\n".join(["AB", "C", "DEF", "GH", "I"]))
    conf = argparse.Namespace(training_settings=dict(batch_size=2, num_workers=0), model_conf=dict(ignore_id=-1))
    tokenizer, converter = _tok()
    train = get_lm_dataloader(conf, str(raw), tokenizer, converter, is_training=True)
    assert train.batch_size == 2 and len(train) == 3 and train.dataset.from_dataset_partition is False
    val = get_lm_dataloader(conf, str(raw), tokenizer, converter, is_training=False)
    batches = list(val)
    assert val.batch_size == 1 and len(batches) == 5 and batches[2][2] == ["DEF"] and batches[2][1].tolist() == [3]
    assert isinstance(batches[0], tuple) and len(batches[0]) == 3


@pytest.mark.parametrize("name,tokens,init", [("lm_english", "char/english", None), ("lm_spanish", "char/spanish", "chainer")])
def test_lm_recipes_keep_their_keys_and_gain_the_training_ones(name, tokens, init):
    conf = yaml.safe_load(open(os.path.join(LM_DIR, name + ".yaml")))
    assert conf["lm"] == "transformer" and conf["init"] == init and conf["token_list"] == tokens
    assert conf["lm_conf"] == dict(att_unit=512, dropout_rate=0.0, embed_unit=128, head=8, layer=16, pos_enc=None, unit=2048)
    assert conf["model_conf"] == {"ignore_id": -1} and conf["token_type"] == "char" and conf["bpemodel"] is None
    ts = conf["training_settings"]
    assert ts["batch_size"] >= 1 and ts["num_workers"] >= 0 and ts["optimizer"] in ("adam", "adamw")
    assert ts["scheduler"] in ("noam", "onecycle") and ts["learning_rate"] > 0
    assert conf["epochs"] >= 1 and conf["accum_grad"] >= 1 and 1 <= conf["average_epochs"] <= conf["epochs"]
    assert ts["epochs"] == conf["epochs"] and ts["accum_grad"] == conf["accum_grad"]      # what set_optimizer reads


class _StubLM(torch.nn.Module):
    """loss = w * (sum of the batch's lengths): ``w.grad`` counts what a window accumulated"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(1.0))
        self.modes = []

    def forward(self, xs, ilens):
        self.modes.append(self.training)
        loss = self.w * ilens.sum().float()
        return loss, {"loss": loss.detach()}, ilens.sum()


class _StubOpt:
    def __init__(self, p):
        self.p, self.seen, self.zeroed = p, [], 0

    def zero_grad(self):
        self.p.grad = None
        self.zeroed += 1

    def step(self):
        self.seen.append(float(self.p.grad))


class _StubSched:
    n = 0

    def step(self):
        self.n += 1


def _batches(lens):
    return [(torch.zeros(1, l, dtype=torch.int64), torch.tensor([l]), ["x"]) for l in lens]


def test_lm_training_steps_at_the_accumulation_boundaries_and_after_the_last_batch():
    from tavsr.train import lm_training
    lm, sched = _StubLM(), _StubSched()
    opt = _StubOpt(lm.w)
    out = lm_training(lm, _batches([1, 2, 3, 4, 5, 6, 7]), opt, sched, 3, device="cpu")
    assert opt.seen == pytest.approx([(1 + 2 + 3) / 3, (4 + 5 + 6) / 3, 7 / 3])      # two full windows and the partial last one
    assert sched.n == 3 and opt.zeroed == 4 and lm.w.grad is None and all(lm.modes)
    assert out == pytest.approx((28 / 3) / (7 / 3))
    opt2 = _StubOpt(lm.w)
    lm_training(lm, _batches([1, 2, 3, 4]), opt2, None, 2, device="cpu")                # no scheduler, no partial window
    assert opt2.seen == pytest.approx([1.5, 3.5])


def test_lm_validation_rounds_the_mean_loss_to_three_decimals():
    from tavsr.train import lm_validation
    lm = _StubLM()
    with torch.no_grad():
        lm.w.fill_(0.33333)
    out = lm_validation(lm, _batches([1, 2, 4]), device="cpu")
    assert out == round(0.33333 * 7 / 3, 3) == 0.778 and not any(lm.modes) and lm.w.grad is None
