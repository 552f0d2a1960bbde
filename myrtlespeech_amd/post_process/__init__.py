"""Decoders: CTC greedy / prefix beam search, RNN-T greedy / beam; the n-gram language model the CTC beam search takes."""
from myrtlespeech_amd.language_model import NGramLanguageModel  # noqa: F401
