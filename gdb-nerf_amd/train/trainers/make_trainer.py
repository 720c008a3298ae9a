"""Plugin factory for the loss surface, the wrapper half of the reference's train/trainers/make_trainer.py:5-9: load the module at
`cfg.loss_path` under the name `cfg.loss_module` and return its `NetworkWrapper(network, cfg)`.  The reference's `Trainer` (its
loop, optimiser, scheduler, recorder and data loaders) is not part of this package: a training script wraps the returned module
in its own."""
from ...networks.make_network import load_source


def make_wrapper(cfg, network):
    return load_source(cfg.loss_module, cfg.loss_path).NetworkWrapper(network, cfg)
