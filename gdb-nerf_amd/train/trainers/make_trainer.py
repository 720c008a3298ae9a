"""Plugin factory for the loss surface and the trainer, the reference's train/trainers/make_trainer.py:5-14: `make_wrapper` loads the
module at `cfg.loss_path` under the name `cfg.loss_module` and returns its `NetworkWrapper(network, cfg)`; `make_trainer` wraps the
network that way and returns the `Trainer` (trainer.py) that runs the epoch loop over it."""
from ...networks.make_network import load_source


def make_wrapper(cfg, network):
    return load_source(cfg.loss_module, cfg.loss_path).NetworkWrapper(network, cfg)


def make_trainer(cfg, network, device=None):
    from .trainer import Trainer
    return Trainer(make_wrapper(cfg, network), cfg, device=device)
