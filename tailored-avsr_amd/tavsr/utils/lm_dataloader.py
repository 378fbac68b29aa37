"""Text batches of the language model (src/utils/lm_dataloader.py): ``lm_data_processing`` pads the token ids of a list of
sentences with ``ignore_id`` (the model delimits rows by the lengths, so the pad value is free), ``get_lm_dataloader`` wraps an
``LMDataset`` - with the keyword the reference misspells (``from_dataset_partiton``) spelt as the dataset declares it."""
from __future__ import annotations

import torch
import torch.utils.data as data

from ..datasets.lm_dataset import LMDataset


def lm_data_processing(batch, tokenizer, converter, ignore_id):
    """-> (x_tokens [B, Lmax] int64 padded with ``ignore_id``, x_ilens [B] int64, refs: the sentences)"""
    x_tokens, x_ilens, refs = [], [], []
    for text in batch:
        ids = torch.tensor(list(converter.tokens2ids(tokenizer.text2tokens(text))), dtype=torch.int64)
        x_tokens.append(ids)
        x_ilens.append(ids.shape[0])
        refs.append(text)
    x_tokens = torch.nn.utils.rnn.pad_sequence(x_tokens, padding_value=ignore_id, batch_first=True).to(torch.int64)
    return x_tokens, torch.tensor(x_ilens, dtype=torch.int64), refs


class _Collate:
    """(a class, not a lambda: worker processes pickle the collate function)"""

    def __init__(self, tokenizer, converter, ignore_id):
        self.tokenizer, self.converter, self.ignore_id = tokenizer, converter, ignore_id

    def __call__(self, batch):
        return lm_data_processing(batch, self.tokenizer, self.converter, self.ignore_id)


def get_lm_dataloader(config, dataset_path, tokenizer, converter, is_training=True):
    dataset = LMDataset(dataset_path=dataset_path, from_dataset_partition=".csv" in dataset_path)
    return data.DataLoader(
        dataset=dataset,
        batch_size=config.training_settings["batch_size"] if is_training else 1,
        shuffle=is_training,
        collate_fn=_Collate(tokenizer, converter, config.model_conf["ignore_id"]),
        num_workers=config.training_settings["num_workers"],
        pin_memory=True,
    )
