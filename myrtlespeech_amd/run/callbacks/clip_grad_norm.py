from typing import Union

from myrtlespeech_amd import optim
from myrtlespeech_amd.run.callbacks.callback import ModelCallback


class ClipGradNorm(ModelCallback):
    """Clips the global gradient norm of the parameters that ``seq_to_seq.optim`` holds, after the backward and before the step
    (``on_backward_end``), with this project's ``optim.clip_grad_norm_`` on the device.  It REWRITES the gradients in place, as
    ``torch.nn.utils.clip_grad_norm_`` does, and so works with any optimizer; the project's own optimizers can clip in
    registers instead (``max_grad_norm``), which leaves ``.grad`` unclipped.  ``last_norm`` is the device tensor
    ``[norm, non-finite flag]`` of the latest call."""

    def __init__(self, seq_to_seq, max_norm: Union[float, int], norm_type: Union[float, int] = 2):
        super().__init__(seq_to_seq)
        if float(norm_type) != 2.0:
            raise ValueError(f"ClipGradNorm serves norm_type 2 only, not {norm_type}")
        self.max_norm = max_norm
        self.norm_type = norm_type
        self.last_norm = None

    def on_backward_end(self, **kwargs):
        params = [p for group in self.model.optim.param_groups for p in group["params"]]
        self.last_norm = optim.clip_grad_norm_(params, self.max_norm, self.norm_type)
