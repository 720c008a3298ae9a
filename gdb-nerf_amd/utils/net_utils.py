"""Checkpoints, the contract of the reference's utils/net_utils.py: a checkpoint is the dictionary {net, optim, scheduler, recorder,
epoch} of state_dicts in `<model_dir>/<epoch>.pth` or `<model_dir>/latest.pth`; `load_model` resumes at `epoch + 1`.

Differences: every `torch.load` passes `map_location` (CPU: `load_state_dict` copies to wherever the module and the optimiser
live) and `weights_only=True` (a checkpoint holds tensors, numbers and containers only); directories are made and files removed with
`os`, nothing shells out, and `resume=False` starts at epoch 0 without deleting what is there; `load_pretrain` takes the directory of
trained models as an argument instead of a global config."""
import os

import torch

KEEP = 100   # numbered checkpoints kept in a directory; the oldest goes first


def _numbered(model_dir):
    return [int(f.split(".")[0]) for f in os.listdir(model_dir) if f != "latest.pth" and f.endswith(".pth") and f.split(".")[0].isdigit()]


def _pick(model_dir, epoch=-1):
    """Path of the checkpoint to load from a directory - `latest.pth` before the highest number - or None."""
    if not os.path.isdir(model_dir):
        return None
    pths, latest = _numbered(model_dir), os.path.exists(os.path.join(model_dir, "latest.pth"))
    if not pths and not latest:
        return None
    name = epoch if epoch != -1 else ("latest" if latest else max(pths))
    return os.path.join(model_dir, f"{name}.pth")


def _load(path):
    print(f"load model: {path}")
    return torch.load(path, map_location="cpu", weights_only=True)


def load_model(net, optim, scheduler, recorder, model_dir, resume=True, epoch=-1):
    path = _pick(model_dir, epoch) if resume else None
    if path is None:
        return 0
    ckpt = _load(path)
    net.load_state_dict(ckpt["net"])
    if "optim" not in ckpt:
        return 0
    optim.load_state_dict(ckpt["optim"])
    scheduler.load_state_dict(ckpt["scheduler"])
    recorder.load_state_dict(ckpt["recorder"])
    return ckpt["epoch"] + 1


def save_model(net, optim, scheduler, recorder, model_dir, epoch, last=False):
    os.makedirs(model_dir, exist_ok=True)
    model = {"net": net.state_dict(), "optim": optim.state_dict(), "scheduler": scheduler.state_dict(),
             "recorder": recorder.state_dict(), "epoch": epoch}
    torch.save(model, os.path.join(model_dir, "latest.pth" if last else f"{epoch}.pth"))
    pths = _numbered(model_dir)
    if len(pths) > KEEP:
        os.remove(os.path.join(model_dir, f"{min(pths)}.pth"))


def load_network(net, model_dir, resume=True, epoch=-1, strict=True):
    if not resume:
        return 0
    if not os.path.exists(model_dir):
        print(f"pretrained model does not exist: {model_dir}")
        return 0
    path = _pick(model_dir, epoch) if os.path.isdir(model_dir) else model_dir
    if path is None:
        return 0
    ckpt = _load(path)
    net.load_state_dict(ckpt["net"], strict=strict)
    return ckpt["epoch"] + 1 if "epoch" in ckpt else 0


def load_pretrain(net, model_dir, trained_model_root=""):
    """The network's weights alone from `<trained_model_root>/<model_dir>`: 0 when loaded, 1 when there is nothing to load."""
    path = _pick(os.path.join(trained_model_root, model_dir))
    if path is None:
        return 1
    net.load_state_dict(_load(path)["net"])
    return 0
