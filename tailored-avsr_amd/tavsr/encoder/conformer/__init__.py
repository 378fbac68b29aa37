from .convolution import ConvolutionModule  # noqa: F401
from .encoder import ConformerEncoder  # noqa: F401
from .encoder_layer import EncoderLayer  # noqa: F401
