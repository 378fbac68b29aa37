from .lm_dataset import LMDataset  # noqa: F401
