"""`Recorder`, `SmoothedValue`, `make_recorder`: the methods of the reference's train/recorder.py, with two differences.

* No tensorboard package is required: `record()` appends ONE JSON line to `<cfg.record_dir>/record.jsonl` -
  {"prefix", "step", "epoch", "scalars": {...}} - and image statistics are not written.  A fresh run (`cfg.resume` false) truncates
  that file; no directory is ever removed and nothing shells out.
* `update_loss_stats` keeps the values as detached 0-dim tensors on their device and copies nothing.  When numbers are needed -
  `record()` or `str()` - everything pending goes to the host as ONE stacked transfer and into the `SmoothedValue`s.  The reference
  calls `.cpu()` on every statistic of every step, i.e. waits for the device once per statistic per step."""
import json
import os
import statistics
from collections import defaultdict, deque

import torch


class SmoothedValue(object):
    """A series of values: median / mean over a window, and the mean of the whole series."""

    def __init__(self, window_size=20):
        self.deque = deque(maxlen=window_size)
        self.total = 0.0
        self.count = 0

    def update(self, value):
        self.deque.append(value)
        self.count += 1
        self.total += value

    @property
    def median(self):   # torch.median's convention: the lower of the two middle values
        return float(statistics.median_low(self.deque))

    @property
    def avg(self):
        return float(sum(self.deque) / len(self.deque))

    @property
    def global_avg(self):
        return self.total / self.count


class Recorder(object):
    def __init__(self, cfg):
        self.local_rank = getattr(cfg, "local_rank", 0)
        if self.local_rank > 0:
            return
        self.log_dir = cfg.record_dir
        os.makedirs(self.log_dir, exist_ok=True)
        self.path = os.path.join(self.log_dir, "record.jsonl")
        if not cfg.resume:
            open(self.path, "w").close()
        self.epoch = 0
        self.step = 0
        self.loss_stats = defaultdict(SmoothedValue)
        self.batch_time = SmoothedValue()
        self.data_time = SmoothedValue()
        self.image_stats = defaultdict(object)
        self.processor = None   # the reference looks up process_<task>; it has none for gdb_nerf
        self._pending = []      # [(keys, detached 0-dim tensors)] not yet copied to the host

    def update_loss_stats(self, loss_dict):
        if self.local_rank > 0:
            return
        keys = list(loss_dict)
        self._pending.append((keys, [v.detach() if isinstance(v, torch.Tensor) else v for v in (loss_dict[k] for k in keys)]))

    def _flush(self):
        """Everything pending -> the SmoothedValues, in arrival order, with one device-to-host copy."""
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        flat = [v for _, vals in pending for v in vals]
        tensors = [v for v in flat if isinstance(v, torch.Tensor)]
        host = iter(torch.stack([t.reshape(()).float() for t in tensors]).tolist() if tensors else ())
        for keys, vals in pending:
            for k, v in zip(keys, vals):
                self.loss_stats[k].update(next(host) if isinstance(v, torch.Tensor) else float(v))

    def update_image_stats(self, image_stats):
        if self.local_rank > 0 or self.processor is None:
            return
        for k, v in self.processor(image_stats).items():
            self.image_stats[k] = v.detach().cpu()

    def record(self, prefix, step=-1, loss_stats=None, image_stats=None):
        if self.local_rank > 0:
            return
        self._flush()
        step = step if step >= 0 else self.step
        loss_stats = loss_stats if loss_stats else self.loss_stats
        scalars = {}
        for k, v in loss_stats.items():
            scalars[k] = v.median if isinstance(v, SmoothedValue) else float(v)
        with open(self.path, "a") as f:
            f.write(json.dumps({"prefix": prefix, "step": int(step), "epoch": int(self.epoch), "scalars": scalars}) + "\n")

    def state_dict(self):
        if self.local_rank > 0:
            return
        return {"step": self.step}

    def load_state_dict(self, scalar_dict):
        if self.local_rank > 0:
            return
        self.step = scalar_dict["step"]

    def __str__(self):
        if self.local_rank > 0:
            return ""
        self._flush()
        loss_state = "  ".join("{}: {:.4f}".format(k, v.avg) for k, v in self.loss_stats.items())
        avg = lambda s: s.avg if s.count else 0.0
        return "  ".join(["epoch: {}", "step: {}", "{}", "data: {:.4f}", "batch: {:.4f}"]).format(
            self.epoch, self.step, loss_state, avg(self.data_time), avg(self.batch_time))


def make_recorder(cfg):
    return Recorder(cfg)
