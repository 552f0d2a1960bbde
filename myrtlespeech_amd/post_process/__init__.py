"""Decoders: CTC greedy / prefix beam search (and its scored n-best), RNN-T greedy / beam; the n-gram language model the CTC beam search takes;
CTC and transducer forced alignment of a known transcript; the chunk-by-chunk RNN-T greedy decoder; the batched edit distance of the word error rate."""
from myrtlespeech_amd.language_model import NGramLanguageModel  # noqa: F401
from myrtlespeech_amd.post_process.ctc_beam_decoder import BeamHypothesis  # noqa: F401
from myrtlespeech_amd.post_process.ctc_aligner import Alignment, CTCForcedAligner, TokenSpan, WordSpan, words  # noqa: F401
from myrtlespeech_amd.post_process.edit_distance import EditCounts, edit_distance  # noqa: F401
from myrtlespeech_amd.post_process.rnnt_aligner import RNNTAlignment, RNNTForcedAligner  # noqa: F401
from myrtlespeech_amd.post_process.rnnt_streaming import StreamingRNNTGreedyDecoder  # noqa: F401
