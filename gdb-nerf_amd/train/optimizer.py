"""`make_optimizer(cfg, net)`, same contract as the reference's train/optimizer.py:13-29: ONE param group per trainable parameter,
each with `cfg.train.lr / weight_decay / eps`, for `cfg.train.optim` in adam, adamw, sgd (momentum 0.9).

`train.hip_optimizer: true` (default false) takes adam / adamw from `optim.HipAdam`: the whole step - the trainer's clip at
CLIP_VALUE included - as one library call instead of a few launches per group.  It is an error with any other optimiser.  `radam` (a
file of the reference's own, utils/optimizer/radam.py) is not part of this package and raises NotImplementedError."""
import torch

from ..optim import HipAdam

CLIP_VALUE = 40.0   # the trainer's clip_grad_value_ (trainer.py:64 of the reference)


def make_optimizer(cfg, net):
    lr, weight_decay, eps = cfg.train.lr, cfg.train.weight_decay, cfg.train.eps
    name = cfg.train.optim
    hip = bool(getattr(cfg.train, "hip_optimizer", False))
    if name == "radam":
        raise NotImplementedError("train.optim: radam is not implemented in this package (adam, adamw and sgd are)")
    if name not in ("adam", "adamw", "sgd"):
        raise ValueError(f"train.optim: unknown optimiser {name!r} (adam, adamw, sgd)")
    if hip and name == "sgd":
        raise ValueError("train.hip_optimizer: true implements adam and adamw only, not train.optim: sgd")
    params = [{"params": [value], "lr": lr, "weight_decay": weight_decay, "eps": eps}
              for _, value in net.named_parameters() if value.requires_grad]
    if name == "sgd":
        return torch.optim.SGD(params, lr, momentum=0.9)
    if hip:
        return HipAdam(params, lr, weight_decay=weight_decay, eps=eps, decoupled=name == "adamw", clip_value=CLIP_VALUE)
    return (torch.optim.AdamW if name == "adamw" else torch.optim.Adam)(params, lr, weight_decay=weight_decay, eps=eps)
