"""The training loop of the reference's ``run`` package, restated: ``train.fit`` and the callback protocol."""
