"""CTC loss (``loss.ctc_loss.CTCLoss``), transducer loss on logits (``loss.rnnt_loss.RNNTLoss``) and the fused transducer loss
on the joint network's inputs (``RNNTJointLoss`` / ``rnnt_joint_loss``, re-exported here)."""
from myrtlespeech_amd.loss.rnnt_loss import RNNTJointLoss, rnnt_joint_loss  # noqa: F401
