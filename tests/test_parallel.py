"""Row-strip sharding of one frame over ranks and the all-gather of rendered strips
(gdb-nerf_amd/parallel.py), exercised with world_size-2/3 gloo process groups on the CPU."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gdb_nerf_amd.parallel import all_strips, gather_strips, row_strip


@pytest.mark.parametrize("H,world", [(256, 8), (256, 1), (10, 4), (3, 8), (37, 5), (1, 2)])
def test_row_strips_partition_rows(H, world):
    strips = all_strips(H, world)
    assert strips[0][0] == 0 and strips[-1][1] == H
    for (a0, a1), (b0, b1) in zip(strips, strips[1:]):
        assert a1 == b0 and a0 <= a1
    sizes = [b - a for a, b in strips]
    assert max(sizes) - min(sizes) <= 1 and sorted(sizes, reverse=True) == sizes
    with pytest.raises(ValueError):
        row_strip(H, world, world)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, B, H, W, C, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        full = torch.arange(B * H * W * C, dtype=torch.float32).view(B * H * W, C)  # what a full render would hold
        mine = torch.full_like(full, float("nan"))                                   # this rank renders only its strip
        r0, r1 = row_strip(H, rank, world)
        mine.view(B, H, W, C)[:, r0:r1] = full.view(B, H, W, C)[:, r0:r1]
        out = gather_strips(mine, H, world, dist, B=B)
        ok = bool(torch.equal(out, full))
        depth = torch.full((B * H * W,), -1.0)
        depth.view(B, H, W)[:, r0:r1] = full[:, 0].view(B, H, W)[:, r0:r1]
        ok = ok and bool(torch.equal(gather_strips(depth, H, world, dist, B=B), full[:, 0].contiguous()))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,B,H,W,C", [(2, 1, 8, 5, 39), (2, 2, 7, 4, 3), (3, 1, 4, 6, 2)])
def test_gather_strips_gloo(world, B, H, W, C):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, B, H, W, C, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, True) for r in range(world)]


class _FakeEngine:
    """Stands in for HotPathEngine.render_packed on the CPU: writes the rows it is asked for, and only those."""

    def __init__(self, truth):
        self.truth = truth

    def render_packed(self, r0, r1, precision, out):
        H = self.truth.shape[0]
        out.view(H, -1)[r0:r1] = self.truth[r0:r1]
        return out


def _packed_worker(rank, world, port, H, W, C, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gdb_nerf_amd.parallel import StripGather
        truth = torch.arange(H * W * C, dtype=torch.float32).view(H, W * C)
        g = StripGather(H, W, C, world, rank, "cpu", dist)
        g.full.fill_(float("nan"))
        ok = True
        for rep in range(2):  # the buffers are reused call after call, exactly as bench.py's rows mode does
            _FakeEngine(truth + rep).render_packed(*g.strip, None, g.full)
            ok = ok and bool(torch.equal(g.gather().view(H, W * C), truth + rep))
        ok = ok and g.even == (H % world == 0) and g.nbytes == (world - 1) * (-(-H // world)) * W * C * 4
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,H,W,C", [(2, 8, 5, 41), (2, 7, 4, 41), (3, 6, 3, 41), (3, 4, 6, 2)])
def test_packed_strip_gather_gloo(world, H, W, C):
    """bench.py's N > 1 step (render_packed of the rank's strip into StripGather.full, then ONE all_gather_into_tensor):
    in place when the rows divide evenly, through the padded buffer otherwise."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_packed_worker, args=(r, world, port, H, W, C, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, True) for r in range(world)]


class _FakeHotPath:
    """Stands in for HotPathEngine inside Network._render_packed on the CPU: writes the rows it is asked for, and only those."""

    def __init__(self, truth, B, H):
        self.truth, self.B, self.H, self.Q, self.device = truth, B, H, truth.shape[1] - 2, torch.device("cpu")
        self.calls = []
        self.fused_supported = True   # (bundle_size 2: what HotPathEngine answers from gdb_render_info)

    def render_packed(self, r0=0, r1=None, precision=None, out=None):
        r1 = self.H if r1 is None else r1
        self.calls.append((r0, r1))
        if out is None:
            out = torch.zeros_like(self.truth)
        v, t = out.view(self.B, self.H, -1), self.truth.view(self.B, self.H, -1)
        v[:, r0:r1] = t[:, r0:r1]
        return out


def _network_worker(rank, world, port, B, H, W, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gdb_nerf_amd.configs import make_cfg
        from gdb_nerf_amd.networks import make_network
        net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.shard", "rows"])).eval()
        ok = net.shard == "rows"
        for rep in range(2):   # the gather buffers are cached per shape and reused frame after frame
            truth = torch.arange(B * H * W * 41, dtype=torch.float32).view(B * H * W, 41) + 1000.0 * rep
            eng = _FakeHotPath(truth, B, H)
            packed = net._render_packed(eng, B, H, W)
            ok = ok and bool(torch.equal(packed, truth)) and eng.calls == [row_strip(H, rank, world)]
        plain = make_network(make_cfg("configs/dtu_eval.yaml")).eval()   # nerf.shard defaults to none: whole frames on every rank
        eng = _FakeHotPath(truth, B, H)
        ok = ok and bool(torch.equal(plain._render_packed(eng, B, H, W), truth)) and eng.calls == [(0, H)]
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,B,H,W", [(2, 1, 8, 5), (2, 1, 7, 4), (2, 2, 5, 3)])
def test_network_forward_shards_rows_over_ranks(world, B, H, W):
    """`nerf.shard: rows` (north_star: rays shard across the GPUs of a node): with torch.distributed initialised,
    Network.forward's hot-path section renders this rank's strip of bundle-map rows and ONE all-gather leaves the whole packed
    bundle map on every rank (even and uneven H, batch > 1); without the key every rank renders whole frames.
    Reference call site: network.py:145-169, driven once per frame by run.py:54-66."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_network_worker, args=(r, world, port, B, H, W, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, True) for r in range(world)]


def test_strip_gather_collective_at_world_1_gloo():
    """`gather(always_collective=True)` takes the real all_gather_into_tensor branch on a ONE-rank group too - in place (the send
    view aliases the receive buffer: send == recv + rank * count) and through the padded buffer - and leaves the rows as they were."""
    from gdb_nerf_amd.parallel import StripGather
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        H, W, C = 6, 5, 41
        truth = torch.arange(H * W * C, dtype=torch.float32).view(H * W, C)
        for padded in (False, True):
            g = StripGather(H, W, C, 1, 0, "cpu", dist, force_padded=padded)
            assert g.even == (not padded) and g.strip == (0, H)
            g.full.copy_(truth)
            out = g.gather(always_collective=True)
            assert out is g.full and torch.equal(out, truth)
            if padded:
                assert torch.equal(g._recv[0].reshape(H * W, C), truth)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_strip_gather_through_one_rank_rccl():
    """The first thing a multi-GPU run does that no one-GPU run did in three rounds: hand RCCL the all-gather of a packed render.
    A ONE-rank "nccl" communicator (RCCL on ROCm) on the box's GPU takes StripGather through the real all_gather_into_tensor call,
    in place (send view aliasing the receive buffer) and padded, on an actual render_packed result: bit-identical rows afterwards.
    Reference: the only process-group bootstrap the reference has is train_net.py:106-111 (DDP init); the all-gather of rendered
    strips is north_star's."""
    from gdb_nerf_amd import synthetic
    from gdb_nerf_amd.engine import HotPathEngine
    from gdb_nerf_amd.parallel import StripGather
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        fr = synthetic.make_frame(64, 80, V=3, seed=0)
        eng = HotPathEngine(max_num_samples=3, is_adaptive=True, device=dev)
        eng.load_weights(synthetic.make_nerf_weights(seed=0))
        eng.prepare({k: torch.from_numpy(v).to(dev) for k, v in fr.items()})
        H, W, C = 32, 40, eng.Q + 2
        want = eng.render_packed(0, H).clone()
        for padded in (False, True):
            g = StripGather(H, W, C, 1, 0, dev, dist, force_padded=padded)
            for rep in range(2):   # buffers reused call after call
                g.full.fill_(float("nan"))
                eng.render_packed(*g.strip, None, g.full)
                out = g.gather(always_collective=True)
                torch.cuda.synchronize()
                assert out is g.full and torch.equal(out, want), (padded, rep)
                if padded:
                    assert torch.equal(g._recv[0].reshape(H * W, C), want)
        # the collective the bench times on N ranks, once: a barrier and a MAX all-reduce of the step time on the device
        dist.barrier()
        t = torch.tensor([1.25], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        assert float(t.item()) == 1.25
    finally:
        dist.destroy_process_group()


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment - the command form the driver uses - starts its own two ranks
    under torch.distributed.run and relays rank 0's ONE JSON line and the exit code (as written it exited at the
    WORLD_SIZE check).  This host has no GPU, so under GDB_BENCH_REHEARSE=1 the ranks rehearse the plumbing alone (gloo rendezvous
    from the launcher's environment, barrier + max-over-ranks timing, the strip all-gather, the per-rank report) and say so."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GDB_BENCH_REHEARSE="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["world_size"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["plumbing_only"] is True and rec["gathered_equals_full_render"] is True
    assert sorted(r["rank"] for r in rec["per_rank"]) == [0, 1]
    # the N > 1 headline is north_star's partitioning: one frame, row strips, ONE all-gather (strong scaling); the line says so
    assert rec["scaling"] == "strong" and rec["config"]["shard"] == "rows" and rec["mode"].startswith("rows:") and "gloo" in rec["collective"]
    assert all(set(r) >= {"rank", "rows", "prepare_ms", "kernel_ms", "allgather_ms", "bus_GBps"} for r in rec["per_rank"])
    assert sorted(tuple(r["rows"]) for r in rec["per_rank"]) == [(0, 16), (16, 32)]
    # a failing rank is not swallowed: the launcher's exit code comes back
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         env={k: v for k, v in env.items() if k != "GDB_BENCH_REHEARSE"}, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "needs a GPU" in bad.stderr


@pytest.mark.gpu
def test_bench_two_ranks_self_launched_on_one_gpu():
    """The same command form on the GPU box: `python bench.py --gpus 2` starts two ranks that share the one card (GDB_BENCH_REHEARSE=1:
    gloo, the all-gather staged through host memory - a rehearsal of the product path, never a measurement).  The line must carry
    what an N > 1 record is graded on.  Headline = north_star's partitioning: ONE frame, row strips, one
    all-gather, strong scaling - with the gathered strips equal to the full render, every rank's prepare / kernel / all-gather time and
    bus GB/s, the same protocol on c4 (`rows_c4`; c5 is left out of this test for its size), the independent-frames record beside it,
    and rank 0's CPU baseline."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GDB_BENCH_REHEARSE="1")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--prewarm-ms", "50", "--rows-extra", "c4", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["world_size"] == 2 and rec["scaling"] == "strong" and rec["value"] > 0 and rec["config"]["shard"] == "rows"
    assert rec["mode"].startswith("rows:") and rec["gathered_equals_full_render"] is True and "gloo" in rec["collective"]
    assert rec["allgather_bytes_per_rank"] > 0 and rec["allgather_ms"] > 0 and rec["bus_GBps"] > 0 and rec["prepare_ms"] > 0
    rr = rec["rows_per_rank"]
    assert sorted(r["rank"] for r in rr) == [0, 1] and rr[0]["rows"] == [0, 128] and rr[1]["rows"] == [128, 256]
    assert all(r["kernel_ms"] > 0 and r["prepare_ms"] > 0 and r["allgather_ms"] > 0 and r["gathered_equals_full_render"] is True for r in rr)
    assert all(r["kernel_ms"] > 0 and 0 < r["roofline_frac"] < 1 for r in rec["per_rank"])
    c4 = rec["rows_c4"]
    assert c4["gathered_equals_full_render"] is True and c4["scaling"] == "strong" and c4["value"] > 0 and c4["kernel"] == "k_render_dense"
    assert [r["rows"] for r in c4["per_rank"]] == [[0, 200], [200, 400]]
    fr = rec["independent_frames"]
    assert fr["scaling"] == "weak" and fr["value"] > 0
    assert rec["cpu_baseline"]["cores"] == 8 and rec["cpu_baseline"]["value"] > 0
    # ... and `--shard frames` puts the weak-scaling record on top
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--prewarm-ms", "50", "--shard", "frames", "--full", "--no-cpu-baseline", "--rows-extra", ""],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    rec2 = json.loads([l for l in p.stdout.splitlines() if l.strip()][0])
    assert rec2["scaling"] == "weak" and rec2["gathered_equals_full_render"] is True and rec2["single_frame_rows"]["scaling"] == "strong"
