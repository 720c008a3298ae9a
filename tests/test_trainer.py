"""The training loop: `Trainer`, `make_optimizer`'s recipe, the schedules, the recorder, checkpoints, `SyntheticFrames` and
`train_net.train` on a four-parameter stand-in that honours the wrapper contract - no GPU - and, on the GPU, K iterations of
`Trainer.train` over the real dtu_pretrain network with `train.hip_optimizer` on and off.

The GPU half writes both loss curves to profiles/optimizer/trainer_curves.json; their difference is recorded, not asserted (the
PyTorch convolution backwards of the step are not run-to-run deterministic)."""
import json
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn as nn

from gdb_nerf_amd import train_net
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.optim import HipAdam
from gdb_nerf_amd.train import make_lr_scheduler, make_optimizer, make_recorder, make_trainer, set_lr_scheduler
from gdb_nerf_amd.train.data import SyntheticFrames
from gdb_nerf_amd.train.recorder import Recorder, SmoothedValue
from gdb_nerf_amd.train.trainers.trainer import Trainer
from gdb_nerf_amd.utils import net_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = os.path.join(ROOT, "profiles", "optimizer", "trainer_curves.json")
K_ITER = 20


class StandIn(nn.Module):
    """Four parameters; forward(batch) -> (output, loss, stats, image_stats).  `log` receives the order of what happens to it."""

    def __init__(self, log=None, big=False):
        super().__init__()
        self.a, self.b = nn.Parameter(torch.tensor([1.0, -2.0, 0.5])), nn.Parameter(torch.tensor(0.25))
        self.lin = nn.Linear(3, 1)
        self.log = [] if log is None else log
        self.big = big

    def forward(self, batch):
        self.log.append("forward")
        y = self.lin(batch["x"] * self.a).squeeze(-1) + self.b
        loss = ((y - batch["y"]) ** 2).mean() * (1e6 if self.big else 1.0)
        return {"y": y}, loss.reshape(1), {"loss": loss.detach(), "mse": loss.detach() * 2}, {}


class LoggedAdam(torch.optim.Adam):
    def __init__(self, params, log, **kw):
        super().__init__(params, **kw)
        self.log, self.seen = log, []

    def zero_grad(self, set_to_none=True):
        self.log.append("zero_grad")
        super().zero_grad(set_to_none)

    def step(self, closure=None):
        self.log.append("step")
        self.seen.append(max(float(p.grad.abs().max()) for g in self.param_groups for p in g["params"]))
        return super().step(closure)


def _cfg(tmp_path, *opts):
    return make_cfg("configs/dtu_pretrain.yaml", ["log_interval", "2", "resume", "False", *opts], workspace=str(tmp_path))


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(5, 3, generator=g), "y": torch.randn(5, generator=g)} for _ in range(n)]


def test_call_order_clip_and_step_counters(tmp_path):
    cfg = _cfg(tmp_path, "ep_iter", "5")
    log = []
    net = StandIn(log, big=True)
    orig = torch.Tensor.backward

    trainer = Trainer(net, cfg, device="cpu")
    opt = LoggedAdam(net.parameters(), log, lr=1e-3)
    rec = make_recorder(cfg)
    try:
        torch.Tensor.backward = lambda self, *a, **k: (log.append("backward"), orig(self, *a, **k))[1]
        trainer.train(3, _batches(5), opt, rec)
    finally:
        torch.Tensor.backward = orig
    assert log == ["forward", "zero_grad", "backward", "step"] * 5
    assert net.training
    assert max(opt.seen) == 40.0                     # the loss is scaled so that the raw gradients are far beyond the clip
    assert trainer.global_step == 5 * 3 + 5 and rec.step == 5
    trainer.train(4, _batches(5), opt, rec)          # a running trainer keeps counting: global_step is seeded once
    assert trainer.global_step == 5 * 3 + 10 and rec.step == 10


def test_hip_adam_takes_the_clip_from_the_trainer(tmp_path):
    cfg = _cfg(tmp_path)
    net = StandIn()
    trainer = Trainer(net, cfg, device="cpu")
    opt = HipAdam(net.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="CUDA"):    # CPU parameters: refused by the optimiser, after the trainer has set the clip
        trainer.train(0, _batches(1), opt, make_recorder(cfg))
    assert opt.clip_value == 40.0
    with pytest.raises(ValueError, match="clips"):
        trainer.train(0, _batches(1), HipAdam(net.parameters(), lr=1e-3, clip_value=1.0), make_recorder(cfg))
    hip = make_optimizer(_cfg(tmp_path, "train.hip_optimizer", "True"), net)
    assert isinstance(hip, HipAdam) and hip.clip_value == 40.0


def test_exponential_schedule_of_dtu_pretrain(tmp_path):
    cfg = _cfg(tmp_path)
    assert cfg.train.scheduler.type == "exponential"
    net = StandIn()
    opt = make_optimizer(cfg, net)
    sch = make_lr_scheduler(cfg, opt)
    assert isinstance(sch, torch.optim.lr_scheduler.LRScheduler)
    lrs = {}
    for e in range(51):
        lrs[e] = [g["lr"] for g in opt.param_groups]
        opt.step()
        sch.step()
    lrs[51] = [g["lr"] for g in opt.param_groups]
    for e in (0, 1, 50):
        assert lrs[e] == [5e-4 * 0.5 ** (e / 50)] * 4, e
    assert lrs[50][0] == pytest.approx(2.5e-4, rel=1e-12)


def test_multi_step_schedule_and_set_lr_scheduler(tmp_path):
    cfg = _cfg(tmp_path, "train.scheduler", "{'type': 'multi_step', 'milestones': [2, 4, 4], 'gamma': 0.5}")
    opt = make_optimizer(cfg, StandIn())
    sch = make_lr_scheduler(cfg, opt)
    assert isinstance(sch, torch.optim.lr_scheduler.LRScheduler) and sch.milestones == Counter([2, 4, 4])
    seen = []
    for _ in range(6):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert seen == [5e-4, 5e-4, 2.5e-4, 2.5e-4, 6.25e-5, 6.25e-5]     # a milestone listed twice halves twice
    cfg.train.scheduler.milestones, cfg.train.scheduler.gamma = [7], 0.1
    set_lr_scheduler(cfg, sch)
    assert sch.milestones == Counter([7]) and sch.gamma == 0.1


class Counting(torch.Tensor):
    """A statistic that counts every conversion to a host number."""
    reads = 0

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in ("item", "cpu", "tolist", "__float__", "numpy", "__int__", "__bool__"):
            Counting.reads += 1
        return super().__torch_function__(func, types, args, kwargs or {})


def test_recorder_json_lines_and_no_host_read_between_log_points(tmp_path):
    cfg = _cfg(tmp_path)
    rec = make_recorder(cfg)
    assert isinstance(rec, Recorder) and isinstance(rec.batch_time, SmoothedValue)
    Counting.reads = 0
    for i in range(3):
        rec.step += 1
        rec.update_loss_stats({"loss": torch.tensor(float(i + 1)).as_subclass(Counting), "psnr": torch.tensor(10.0 * (i + 1)).as_subclass(Counting)})
    assert Counting.reads == 0 and len(rec.loss_stats) == 0            # nothing has been read on the host yet
    rec.record("train")
    assert Counting.reads >= 1
    assert rec.loss_stats["loss"].count == 3 and rec.loss_stats["loss"].median == 2.0 and rec.loss_stats["psnr"].global_avg == 20.0
    text = str(rec)
    assert "epoch: 0" in text and "step: 3" in text and "loss: 2.0000" in text
    rec.record("val", 7, {"psnr": torch.tensor(31.5), "n": 2})
    lines = [json.loads(l) for l in open(os.path.join(cfg.record_dir, "record.jsonl"))]
    assert lines == [{"prefix": "train", "step": 3, "epoch": 0, "scalars": {"loss": 2.0, "psnr": 20.0}},
                     {"prefix": "val", "step": 7, "epoch": 0, "scalars": {"psnr": 31.5, "n": 2.0}}]
    assert rec.state_dict() == {"step": 3}
    # a resumed recorder appends; a fresh one starts the file again and removes nothing else from the directory
    keep = os.path.join(cfg.record_dir, "other.txt")
    open(keep, "w").write("x")
    cfg.resume = True
    make_recorder(cfg).record("train", 9, {"loss": 1.0})
    assert len(open(os.path.join(cfg.record_dir, "record.jsonl")).readlines()) == 3
    cfg.resume = False
    make_recorder(cfg)
    assert open(os.path.join(cfg.record_dir, "record.jsonl")).read() == "" and os.path.exists(keep)


def test_trainer_reads_statistics_only_at_log_points(tmp_path, monkeypatch):
    cfg = _cfg(tmp_path, "log_interval", "3")
    net = StandIn()
    trainer = Trainer(net, cfg, device="cpu")
    rec = make_recorder(cfg)
    flushed = []
    orig = Recorder._flush
    monkeypatch.setattr(Recorder, "_flush", lambda self: (flushed.append((self.step, len(self._pending))), orig(self))[1])
    trainer.train(0, _batches(7), make_optimizer(cfg, net), rec)
    with_work = [f for f in flushed if f[1]]
    assert with_work == [(3, 3), (6, 3), (7, 1)]          # iterations 3 and 6 (log_interval) and 7 (the last): one stacked copy each
    lines = [json.loads(l) for l in open(os.path.join(cfg.record_dir, "record.jsonl"))]
    assert [l["step"] for l in lines] == [3, 6, 7] and set(lines[0]["scalars"]) == {"loss", "mse"}


RESUME = """
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_trainer import StandIn, _cfg
from gdb_nerf_amd.train import make_lr_scheduler, make_optimizer, make_recorder
from gdb_nerf_amd.utils import net_utils
cfg = _cfg(sys.argv[2], "resume", "True")
net = StandIn()
with torch.no_grad():
    for p in net.parameters():
        p.fill_(9.0)
opt = make_optimizer(cfg, net); sch = make_lr_scheduler(cfg, opt); rec = make_recorder(cfg)
begin = net_utils.load_model(net, opt, sch, rec, cfg.trained_model_dir, resume=True)
torch.save({"begin": begin, "net": net.state_dict(), "optim": opt.state_dict(), "sched": sch.state_dict(), "rec": rec.state_dict()}, sys.argv[3])
"""


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


PLUGIN = """
import torch.nn as nn
class NetworkWrapper(nn.Module):   # the stand-in already returns (output, loss, stats, image_stats)
    def __init__(self, net, cfg):
        super().__init__()
        self.net = net
    def forward(self, batch):
        return self.net(batch)
"""


def _plugin(cfg, tmp_path):
    path = tmp_path / "standin_loss.py"
    path.write_text(PLUGIN)
    cfg.loss_module, cfg.loss_path = "standin_loss", str(path)
    return cfg


def test_checkpoint_resumes_in_a_new_process(tmp_path):
    cfg = _plugin(_cfg(tmp_path, "train.epoch", "3"), tmp_path)
    net = StandIn()
    train_net.train(cfg, net, _batches(4), device="cpu")
    files = sorted(os.listdir(cfg.trained_model_dir))
    assert files == ["0.pth", "1.pth", "2.pth", "latest.pth"]
    ckpt = torch.load(os.path.join(cfg.trained_model_dir, "latest.pth"), map_location="cpu", weights_only=True)
    assert set(ckpt) == {"net", "optim", "scheduler", "recorder", "epoch"} and ckpt["epoch"] == 2 and ckpt["recorder"] == {"step": 12}
    out = str(tmp_path / "resumed.pt")
    r = subprocess.run([sys.executable, "-c", RESUME, ROOT, str(tmp_path), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = torch.load(out, map_location="cpu", weights_only=True)
    assert got["begin"] == 3
    assert _same(got["net"], dict(net.state_dict()))
    assert _same(got["optim"]["state"], ckpt["optim"]["state"]) and len(got["optim"]["state"]) == 4
    assert [g["lr"] for g in got["optim"]["param_groups"]] == [5e-4 * 0.5 ** (3 / 50)] * 4
    assert got["sched"]["last_epoch"] == 3 and got["rec"] == {"step": 12}
    # train() itself picks the run up where it stopped: epochs 3 and 4 only
    cfg2 = _plugin(_cfg(tmp_path, "train.epoch", "5", "resume", "True"), tmp_path)
    train_net.train(cfg2, net, _batches(4), device="cpu")
    assert sorted(os.listdir(cfg.trained_model_dir)) == ["0.pth", "1.pth", "2.pth", "3.pth", "4.pth", "latest.pth"]
    assert [json.loads(l)["step"] for l in open(os.path.join(cfg.record_dir, "record.jsonl"))][-1] == 20
    assert net_utils.load_network(StandIn(), cfg.trained_model_dir) == 5
    assert net_utils.load_network(StandIn(), cfg.trained_model_dir, epoch=1) == 2
    assert net_utils.load_pretrain(StandIn(), "dtu_pretrain", os.path.dirname(cfg.trained_model_dir)) == 0
    assert net_utils.load_pretrain(StandIn(), "absent", os.path.dirname(cfg.trained_model_dir)) == 1


def test_synthetic_frames_layout():
    cfg = make_cfg("configs/dtu_pretrain.yaml")
    assert list(cfg.mvs.vol_scales) == [0.125, 0.5]
    data = SyntheticFrames(cfg, 3, 64, 96, V=3, seed=5)
    assert len(data) == 3
    batches = list(data)
    assert len(batches) == 3
    b = batches[0]
    assert set(b) == {"src_views", "tar_views", "near_far", "tar_gt_ms"}
    assert b["src_views"]["rgb"].shape == (1, 3, 3, 64, 96) and b["src_views"]["extrinsics"].shape == (1, 3, 4, 4)
    assert b["src_views"]["intrinsics"].shape == (1, 3, 3, 3)
    assert b["tar_views"]["rgb"].shape == (1, 64, 96, 3) and b["tar_views"]["extrinsics"].shape == (1, 4, 4) and b["tar_views"]["intrinsics"].shape == (1, 3, 3)
    assert b["near_far"].shape == (1, 2)
    assert [tuple(t.shape) for t in b["tar_gt_ms"]["rgb"]] == [(1, 8, 12, 3), (1, 32, 48, 3)]
    tar = b["tar_views"]["rgb"].double()
    for t, k in zip(b["tar_gt_ms"]["rgb"], (8, 2)):     # the area average of the target image
        ref = tar.reshape(1, 64 // k, k, 96 // k, k, 3).mean(dim=(2, 4))
        assert t.dtype == torch.float32 and (t.double() - ref).abs().max() < 1e-6
    assert all(v.dtype == torch.float32 for v in (b["near_far"], b["src_views"]["rgb"], b["tar_views"]["rgb"]))
    again = list(SyntheticFrames(cfg, 3, 64, 96, V=3, seed=5))
    assert torch.equal(again[1]["tar_views"]["rgb"], batches[1]["tar_views"]["rgb"]) and not torch.equal(batches[0]["tar_views"]["rgb"], batches[1]["tar_views"]["rgb"])
    with pytest.raises(ValueError, match="divide"):
        SyntheticFrames(cfg, 1, 60, 96)
    assert "TESTS AND SMOKE" in sys.modules[SyntheticFrames.__module__].__doc__


def test_distributed_raises_and_nothing_sets_launch_blocking(tmp_path):
    cfg = _cfg(tmp_path, "distributed", "True", "train.photometric_weights", "[1.0, 0.1, 0.0]")
    with pytest.raises(NotImplementedError, match="distributed"):
        Trainer(StandIn(), cfg, device="cpu")
    with pytest.raises(NotImplementedError, match="distributed"):
        make_trainer(cfg, StandIn())
    pkg = os.path.join(ROOT, "gdb-nerf_amd")
    for rel in ("train_net.py", "train/trainers/trainer.py", "train/recorder.py", "utils/net_utils.py", "optim.py"):
        src = open(os.path.join(pkg, rel)).read()
        assert "os.environ[" not in src and "os.system" not in src and "kill" not in src.replace("killed", ""), rel


# ---- GPU: the real network ------------------------------------------------------------------------------------------------------------
def _run(hip, K, ws):
    from gdb_nerf_amd.networks import make_network
    cfg = make_cfg("configs/dtu_pretrain.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "train.photometric_weights", "[1.0, 0.1, 0.0]",
                                                 "train.hip_optimizer", str(hip), "log_interval", "1000", "resume", "False"],
                   workspace=str(ws))
    torch.manual_seed(109)
    net = make_network(cfg)
    trainer = make_trainer(cfg, net)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt = make_optimizer(cfg, net)
    assert isinstance(opt, HipAdam) == hip and len(opt.param_groups) == sum(p.requires_grad for p in net.parameters())
    rec = make_recorder(cfg)
    batch = SyntheticFrames(cfg, 1, 64, 96, V=3, seed=11).batch(0)
    had_grad, nonzero = {}, {}
    orig = opt.step

    def step(*a, **k):   # which parameters the backward reached, seen where the optimiser sees it
        for n, p in net.named_parameters():
            had_grad[n] = had_grad.get(n, False) or p.grad is not None
            nonzero[n] = nonzero.get(n, False) or (p.grad is not None and bool(p.grad.count_nonzero()))
        return orig(*a, **k)
    opt.step = step
    kept, update = [], rec.update_loss_stats
    rec.update_loss_stats = lambda stats: (kept.append(stats["loss"].detach()), update(stats))[1]
    trainer.train(0, [batch] * K, opt, rec)
    return net, before, (had_grad, nonzero), torch.stack(kept).tolist(), rec


@pytest.mark.gpu
def test_trainer_on_the_dtu_pretrain_network(tmp_path):
    K = K_ITER
    net, before, (had_grad, nonzero), losses, rec = _run(True, K, tmp_path / "hip")
    assert rec.step == K and len(losses) == K
    print("HipAdam loss curve:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)), losses
    moved = {n: not torch.equal(p.detach(), before[n]) for n, p in net.named_parameters()}
    # "received a gradient" is a gradient with a non-zero element in some iteration: from an identically zero one Adam's update is
    # 0 / (0 + eps), and the parameter keeps its bits under torch.optim.Adam as well (the stage NeRF's agg_w_fc is such a tensor)
    zero_only = sorted(n for n in had_grad if had_grad[n] and not nonzero[n])
    print("gradient tensors that were identically zero in every iteration:", zero_only)
    assert sum(nonzero.values()) > len(nonzero) // 2
    for n in moved:
        assert moved[n] == nonzero[n], (n, "moved" if moved[n] else "did not move", "gradient" if had_grad[n] else "no gradient",
                                        "non-zero" if nonzero[n] else "all zero")
    _, _, _, ref, _ = _run(False, K, tmp_path / "torch")
    print("torch Adam loss curve:", " ".join(f"{v:.5f}" for v in ref))
    try:
        os.makedirs(os.path.dirname(CURVES), exist_ok=True)
        with open(CURVES, "w") as f:
            json.dump({"iterations": K, "frame": "64x96, V=3, one fixed batch", "hip_adam_loss": losses, "torch_adam_loss": ref,
                       "max_abs_difference": float(np.max(np.abs(np.array(losses) - np.array(ref)))),
                       "parameters_with_gradient": sum(had_grad.values()), "parameters_without": sum(not v for v in had_grad.values()),
                       "gradients_identically_zero": zero_only}, f, indent=1)
    except OSError:
        pass
    assert losses[-1] < losses[0], (losses[0], losses[-1])
