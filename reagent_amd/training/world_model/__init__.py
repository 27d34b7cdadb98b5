from .mdnrnn_trainer import MDNRNNTrainer  # noqa: F401
