"""``python -m tavsr.lm_main`` - trains and evaluates the language model of a recipe (lm_main.py:59-152 with the pieces it reads
but never defines filled in: the optional checkpoint comes from ``--load-lm``, the training keys from the recipe's
``training_settings`` / ``epochs`` / ``accum_grad`` / ``average_epochs``).  Per epoch: train, validate, test, save; at the end
the ``average_epochs`` checkpoints with the lowest validation loss are averaged and saved as ``model_average.pth``."""
from __future__ import annotations

import argparse
import os

import torch

from .tasks.lm import LMTask
from .train import lm_training, lm_validation, set_optimizer
from .utils.config import load_config
from .utils.lm_dataloader import get_lm_dataloader
from .utils.model_checkpoint import average_model, save_model, save_val_stats
from .utils.tokens import load_token_list


class CharTokenizer:
    """espnet2 CharTokenizer with ``space_symbol="<space>"``: one token per character"""

    def text2tokens(self, text):
        return ["<space>" if c == " " else c for c in text]


class TokenIDConverter:
    """espnet2 TokenIDConverter: ids of a token list, ``<unk>`` for everything else"""

    def __init__(self, token_list):
        self.token2id = {t: i for i, t in enumerate(token_list)}
        self.unk = self.token2id["<unk>"]

    def tokens2ids(self, tokens):
        return [self.token2id.get(t, self.unk) for t in tokens]


def get_tokenizer_converter(token_type, bpemodel, token_list):
    if token_type != "char":
        raise ValueError(f"the shipped LM recipes are character models (token_type: char): {token_type}")
    return CharTokenizer(), TokenIDConverter(load_token_list(token_list))


def build_parser():
    parser = argparse.ArgumentParser(description="Language Model based on an End-to-End architecture",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--training-dataset", default="", type=str, help="Path to where the training dataset split is")
    parser.add_argument("--validation-dataset", default="", type=str, help="Path to where the validation dataset split is")
    parser.add_argument("--test-dataset", default="", type=str, help="Path to where the test dataset split is")
    parser.add_argument("--mode", default="both", type=str, help="Choose: 'training', 'evaluation' or 'both'")
    parser.add_argument("--lm-config-file", default="", type=str, help="Path to a config file that specifies the LM architecture")
    parser.add_argument("--load-lm", default="", type=str, help="Path to load a pre-trained LM")
    parser.add_argument("--yaml-overrides", metavar="CONF:KEY:VALUE", nargs="*",
                        help="Set a number of conf-key-value pairs for modifying the yaml config file on the fly.")
    parser.add_argument("--output-dir", required=True, type=str, help="Path to save the language model")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    conf = load_config(args.lm_config_file, args.yaml_overrides)
    device = getattr(conf, "device", "cuda")
    tokenizer, converter = get_tokenizer_converter(conf.token_type, conf.bpemodel, conf.token_list)
    lm = LMTask.build_model(conf).to(dtype=getattr(torch, getattr(conf, "dtype", "float32")), device=device)
    if args.load_lm:
        print(f"Loading the entire LM system from {args.load_lm}")
        lm.load_state_dict(torch.load(args.load_lm, map_location=device))
    loader = lambda path, train=False: get_lm_dataloader(conf, dataset_path=path, tokenizer=tokenizer, converter=converter,
                                                         is_training=train)
    val_loader, test_loader = loader(args.validation_dataset), loader(args.test_dataset)
    if args.mode in ("training", "both"):
        train_loader = loader(args.training_dataset, True)
        conf.training_settings.setdefault("epochs", conf.epochs)
        conf.training_settings.setdefault("accum_grad", conf.accum_grad)
        optimizer, scheduler = set_optimizer(conf, lm, train_loader)
        print("\nTRAINING PHASE\n")
        os.makedirs(args.output_dir, exist_ok=True)
        val_stats = []
        grad_clip = float(conf.training_settings.get("grad_clip", -1.0))
        grad_clip_type = float(conf.training_settings.get("grad_clip_type", 2.0))
        for epoch in range(1, conf.epochs + 1):
            train_loss = lm_training(lm, train_loader, optimizer, scheduler, conf.accum_grad, device, grad_clip=grad_clip,
                                     grad_clip_type=grad_clip_type)
            val_loss, test_loss = lm_validation(lm, val_loader, device), lm_validation(lm, test_loader, device)
            print(f"Epoch {epoch}: TRAIN LOSS={train_loss} || VAL LOSS={val_loss} || TEST LOSS={test_loss}")
            if grad_clip > 0 and hasattr(optimizer, "clip_stats"):
                st = optimizer.clip_stats()
                print(f"Epoch {epoch}: GRAD CLIP={grad_clip} || STEPS={st['steps']} || SKIPPED={st['skipped']} || "
                      f"CLIPPED={st['clipped']} || LAST NORM={st['last_norm']}")
            val_stats.append((save_model(args.output_dir, lm, str(epoch).zfill(3)), val_loss))
        save_val_stats(args.output_dir, val_stats)
        best = [path for path, _ in sorted(val_stats, key=lambda s: s[1])[: conf.average_epochs]]
        average_model(lm, best)
        save_model(args.output_dir, lm, "average")
    if args.mode in ("evaluation", "both"):
        print(f"VAL LOSS={lm_validation(lm, val_loader, device)} || TEST LOSS={lm_validation(lm, test_loader, device)}")


if __name__ == "__main__":
    main()
