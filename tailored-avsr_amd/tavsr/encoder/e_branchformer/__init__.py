from .encoder import EBranchformerEncoder  # noqa: F401
from .encoder_layer import EBranchformerEncoderLayer  # noqa: F401
