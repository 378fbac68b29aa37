"""``LMDataset`` - the text a language model is trained on (src/datasets/lm_dataset.py): a raw text file with one sentence per
line, or a split CSV of an audio-visual dataset whose ``transcription_path`` column names one text file per sample (its first
line is the sentence).  Sentences are upper-cased and ``{`` / ``}`` are removed, as the reference does."""
from __future__ import annotations

import csv

from torch.utils.data import Dataset


class LMDataset(Dataset):
    def __init__(self, dataset_path, from_dataset_partition=True):
        self.dataset_path = dataset_path
        self.from_dataset_partition = from_dataset_partition
        if from_dataset_partition:
            with open(dataset_path, "r", encoding="utf-8", newline="") as f:
                self.samples = [row["transcription_path"] for row in csv.DictReader(f, delimiter=",")]
        else:
            with open(dataset_path, "r", encoding="utf-8") as f:
                self.samples = [line.strip() for line in f.readlines()]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        if self.from_dataset_partition:
            with open(self.samples[index], "r") as f:
                text = f.readlines()[0].strip()
        else:
            text = self.samples[index]
        return text.upper().replace("{", "").replace("}", "")
