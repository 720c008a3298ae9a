"""`make_lr_scheduler` / `set_lr_scheduler`, same contract as the reference's train/scheduler.py and the two schedules of its
utils/optimizer/lr_scheduler.py it builds, stepped once per epoch:

  exponential: lr = base_lr * gamma ** (epoch / decay_epochs)
  multi_step:  lr *= gamma ** (times `epoch` occurs among the milestones), the milestones kept as a Counter

Both subclass torch's scheduler base, so `state_dict()` / `load_state_dict()` are torch's; `set_lr_scheduler` re-applies the
config's schedule after a checkpoint has been loaded (a resumed run follows the current config, as in the reference)."""
from collections import Counter

from torch.optim.lr_scheduler import LRScheduler


class MultiStepLR(LRScheduler):
    def __init__(self, optimizer, milestones, gamma=0.1, last_epoch=-1):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        groups = self.optimizer.param_groups
        if self.last_epoch not in self.milestones:
            return [g["lr"] for g in groups]
        return [g["lr"] * self.gamma ** self.milestones[self.last_epoch] for g in groups]


class ExponentialLR(LRScheduler):
    def __init__(self, optimizer, decay_epochs, gamma=0.1, last_epoch=-1):
        self.decay_epochs = decay_epochs
        self.gamma = gamma
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [base_lr * self.gamma ** (self.last_epoch / self.decay_epochs) for base_lr in self.base_lrs]


def make_lr_scheduler(cfg, optimizer):
    sch = cfg.train.scheduler
    if sch.type == "multi_step":
        return MultiStepLR(optimizer, milestones=sch.milestones, gamma=sch.gamma)
    if sch.type == "exponential":
        return ExponentialLR(optimizer, decay_epochs=sch.decay_epochs, gamma=sch.gamma)
    raise ValueError(f"train.scheduler.type: unknown schedule {sch.type!r} (multi_step, exponential)")


def set_lr_scheduler(cfg, scheduler):
    sch = cfg.train.scheduler
    if sch.type == "multi_step":
        scheduler.milestones = Counter(sch.milestones)
    elif sch.type == "exponential":
        scheduler.decay_epochs = sch.decay_epochs
    scheduler.gamma = sch.gamma
