from myrtlespeech_amd.run.callbacks.callback import Callback, CallbackHandler, ModelCallback  # noqa: F401
from myrtlespeech_amd.run.callbacks.clip_grad_norm import ClipGradNorm  # noqa: F401
from myrtlespeech_amd.run.callbacks.report_ctc_decoder import ReportCTCDecoder  # noqa: F401
from myrtlespeech_amd.run.callbacks.report_mean_batch_loss import ReportMeanBatchLoss  # noqa: F401
from myrtlespeech_amd.run.callbacks.stop_epoch_after import StopEpochAfter  # noqa: F401
