"""CTC loss (``loss.ctc_loss.CTCLoss``) and transducer loss (``loss.rnnt_loss.RNNTLoss``)."""
