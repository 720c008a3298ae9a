"""`train(cfg, network, train_loader, val_loader=None)`: the epoch loop of the reference's train_net.py:26-77 - trainer, optimiser,
scheduler, recorder, evaluator; resume from `cfg.trained_model_dir`; per epoch the trainer's pass, `scheduler.step()`, then the
numbered checkpoint every `save_ep`, `latest.pth` every `save_latest_ep` and a validation pass every `eval_ep` epochs unless
`skip_eval`.  The data loaders are arguments (this package has no data-set readers), CUDA_LAUNCH_BLOCKING is not set, and the process
is not killed at the end.

    python -m gdb_nerf_amd.train_net [--cfg configs/dtu_pretrain.yaml] [--frames 4] [--size 64 96] [key value ...]

runs it on `train.data.SyntheticFrames` - a smoke run of the loop, not training: those frames are not multi-view consistent."""
import argparse
import os
import random

import numpy as np
import torch

from .evaluators.make_evaluator import make_evaluator
from .train import make_lr_scheduler, make_optimizer, make_recorder, make_trainer, set_lr_scheduler
from .utils.net_utils import load_model, load_pretrain, save_model


def train(cfg, network, train_loader, val_loader=None, device=None):
    if cfg.fix_random:
        random.seed(0)
        np.random.seed(0)
        torch.manual_seed(0)
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
    trainer = make_trainer(cfg, network, device=device)
    optimizer = make_optimizer(cfg, network)
    scheduler = make_lr_scheduler(cfg, optimizer)
    recorder = make_recorder(cfg)
    evaluate = not cfg.skip_eval and val_loader is not None
    evaluator = make_evaluator(cfg) if evaluate else None

    begin_epoch = load_model(network, optimizer, scheduler, recorder, cfg.trained_model_dir, resume=cfg.resume)
    if begin_epoch == 0 and cfg.train.pretrain != "":
        load_pretrain(network, cfg.train.pretrain, os.path.dirname(cfg.trained_model_dir))   # <workspace>/trained_model/<task>
    set_lr_scheduler(cfg, scheduler)

    for epoch in range(begin_epoch, cfg.train.epoch):
        recorder.epoch = epoch
        if hasattr(train_loader, "dataset"):
            train_loader.dataset.epoch = epoch
        trainer.train(epoch, train_loader, optimizer, recorder)
        scheduler.step()
        if (epoch + 1) % cfg.save_ep == 0:
            save_model(network, optimizer, scheduler, recorder, cfg.trained_model_dir, epoch)
        if (epoch + 1) % cfg.save_latest_ep == 0:
            save_model(network, optimizer, scheduler, recorder, cfg.trained_model_dir, epoch, last=True)
        if evaluate and (epoch + 1) % cfg.eval_ep == 0:
            trainer.val(epoch, val_loader, evaluator, recorder)
    return network


def main(argv=None):
    from .configs import make_cfg
    from .networks import make_network
    from .train.data import SyntheticFrames
    ap = argparse.ArgumentParser(description="smoke run of the training loop on synthetic frames")
    ap.add_argument("--cfg", default="configs/dtu_pretrain.yaml")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(64, 96))
    ap.add_argument("opts", nargs="*")
    args = ap.parse_args(argv)
    base = ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "train.photometric_weights", "[1.0, 0.1, 0.0]", "train.epoch", "1",
            "skip_eval", "True"]
    cfg = make_cfg(args.cfg, base + list(args.opts))
    loader = SyntheticFrames(cfg, args.frames, *args.size)
    train(cfg, make_network(cfg), loader)
    print("done: checkpoints in", cfg.trained_model_dir)


if __name__ == "__main__":
    main()
