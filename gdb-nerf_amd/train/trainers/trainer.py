"""`Trainer(network, cfg)`: the epoch loop of the reference's train/trainers/trainer.py.  `network` is the wrapped module
(`make_wrapper`: forward(batch) -> (output, loss, scalar_stats, image_stats)).

`train` keeps the reference's order per iteration: forward -> loss.mean() -> zero_grad -> backward -> clip at 40 -> step; then
recorder.step, the statistics, the timers and global_step.  Where it differs:

* With an `optim.HipAdam` the clip is part of the optimiser's one library call (`clip_value` = 40); with any other optimiser it is
  `torch.nn.utils.clip_grad_value_`.
* Statistics stay on the device between log points: the recorder copies them, stacked, when it prints or records - at
  `cfg.log_interval` and at the last iteration (the reference's second condition names the iteration before the last).  Nothing
  here sets CUDA_LAUNCH_BLOCKING.
* `cfg.distributed` raises: DistributedDataParallel / SyncBatchNorm are not part of this package.
* The config is an argument, not a module global."""
import datetime
import time

import torch

from ...optim import HipAdam
from ..optimizer import CLIP_VALUE


def to_device(batch, device):
    if isinstance(batch, (tuple, list)):
        return [to_device(b, device) for b in batch]
    if isinstance(batch, dict):
        return {k: to_device(v, device) for k, v in batch.items()}
    if isinstance(batch, torch.Tensor):
        return batch.to(device, non_blocking=True)
    return batch


class Trainer(object):
    def __init__(self, network, cfg, device=None):
        if getattr(cfg, "distributed", False):
            raise NotImplementedError("cfg.distributed: DistributedDataParallel / SyncBatchNorm training is not implemented in this package")
        self.cfg = cfg
        self.local_rank = getattr(cfg, "local_rank", 0)
        self.device = torch.device(device if device is not None else "cuda:{}".format(self.local_rank))
        self.network = network.to(self.device)
        self.global_step = 0

    def reduce_loss_stats(self, loss_stats):
        return {k: torch.mean(v) if isinstance(v, torch.Tensor) else v for k, v in loss_stats.items()}

    def train(self, epoch, data_loader, optimizer, recorder):
        cfg = self.cfg
        max_iter = len(data_loader)
        self.network.train()
        hip = isinstance(optimizer, HipAdam)
        if hip:
            if optimizer.clip_value is None:
                optimizer.clip_value = CLIP_VALUE
            elif optimizer.clip_value != CLIP_VALUE:
                raise ValueError(f"Trainer clips gradients at {CLIP_VALUE}; the HipAdam it was given clips at {optimizer.clip_value}")
        params = [p for p in self.network.parameters()]
        end = time.time()
        if self.global_step == 0:
            self.global_step = cfg.ep_iter * epoch
        for iteration, batch in enumerate(data_loader):
            data_time = time.time() - end
            iteration = iteration + 1

            batch = to_device(batch, self.device)
            batch["step"] = 0

            output, loss, loss_stats, image_stats = self.network(batch)
            loss = loss.mean()
            optimizer.zero_grad()
            loss.backward()
            if not hip:
                torch.nn.utils.clip_grad_value_(params, CLIP_VALUE)
            optimizer.step()

            if self.local_rank > 0:
                continue

            recorder.step += 1
            recorder.update_loss_stats(self.reduce_loss_stats(loss_stats))

            batch_time = time.time() - end
            end = time.time()
            recorder.batch_time.update(batch_time)
            recorder.data_time.update(data_time)

            self.global_step += 1
            if iteration % cfg.log_interval == 0 or iteration == max_iter:
                eta_seconds = recorder.batch_time.global_avg * (max_iter - iteration)
                eta_string = str(datetime.timedelta(seconds=int(eta_seconds)))
                lr = optimizer.param_groups[0]["lr"]
                memory = torch.cuda.max_memory_allocated() / 1024.0 / 1024.0 if self.device.type == "cuda" else 0.0
                print("  ".join(["eta: {}", "{}", "lr: {:.6f}", "max_mem: {:.0f}"]).format(eta_string, str(recorder), lr, memory))
                recorder.update_image_stats(image_stats)
                recorder.record("train")

    def val(self, epoch, data_loader, evaluator=None, recorder=None):
        self.network.eval()
        if self.device.type == "cuda":
            torch.cuda.empty_cache()
        val_loss_stats = {}
        image_stats = {}
        data_size = len(data_loader)
        for batch in data_loader:
            batch = to_device(batch, self.device)
            batch["step"] = recorder.step if recorder else 0
            with torch.no_grad():
                output, loss, loss_stats, _ = self.network(batch)
                if evaluator is not None:
                    image_stats_ = evaluator.evaluate(output, batch)
                    if image_stats_ is not None:
                        image_stats.update(image_stats_)
            for k, v in self.reduce_loss_stats(loss_stats).items():
                val_loss_stats[k] = val_loss_stats.get(k, 0) + v

        if val_loss_stats:   # one stacked copy for the whole validation set
            keys = [k for k, v in val_loss_stats.items() if isinstance(v, torch.Tensor)]
            host = torch.stack([val_loss_stats[k].reshape(()).float() for k in keys]).tolist() if keys else []
            val_loss_stats.update(zip(keys, host))
            val_loss_stats = {k: float(v) / data_size for k, v in val_loss_stats.items()}
        print(["{}: {:.4f}".format(k, v) for k, v in val_loss_stats.items()])

        if evaluator is not None:
            val_loss_stats.update(evaluator.summarize())

        if recorder:
            recorder.record("val", epoch, val_loss_stats, image_stats)
        return val_loss_stats
