from .beam_search import Speech2Text
from .maskctc import Speech2TextMaskCTC

__all__ = ["Speech2Text", "Speech2TextMaskCTC"]
