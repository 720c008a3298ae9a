"""bench.py --dump-outputs: what the timed path returned in its last step, written as float32 .npy files so that two builds can be
compared output for output on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


def test_dump_outputs_keeps_a_fixed_sample_under_the_budget(tmp_path):
    """Outputs above the budget are cut to one seeded sample of rows, the same rows for every array of that row count, and the
    files stay under 64 MB in all; outputs within it are written whole."""
    nb, Q = 1200 * 1600 // 4, 39   # c5's bundle map: 75 MB of bundle_feat
    arrays = {"bundle_feat": torch.arange(nb, dtype=torch.float32)[:, None] + torch.arange(Q) / Q, "bundle_depth": torch.arange(nb, dtype=torch.float32),
              "bundle_opacity": -torch.arange(nb, dtype=torch.float32)}
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), arrays)
        assert rec["row_sample"] != "all rows" and rec["dtype"] == "float32"
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert all(a.dtype == np.float32 for a in got.values())
    rows = got["bundle_depth"].astype(np.int64)
    assert len(rows) == rec["arrays"]["bundle_depth"]["shape"][0] and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["bundle_opacity"], -got["bundle_depth"]) and np.array_equal(got["bundle_feat"], arrays["bundle_feat"].numpy()[rows])
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))
    small = {n: t[:1000] for n, t in arrays.items()}
    rec = bench.dump_outputs(str(tmp_path / "c"), small)
    assert rec["row_sample"] == "all rows"
    assert np.array_equal(np.load(tmp_path / "c" / "bundle_feat.npy"), small["bundle_feat"].numpy())


def _bench(args, out_dir, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--steps", "3", "--warmup", "1", "--prewarm-ms", "0",
                        "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(out_dir), *args],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_bench_dumps_the_last_step_of_its_timed_path(tmp_path, path):
    """N = 1: the dumped arrays are the render of the benched frame (synthetic seed 0) that the same path returns when called
    directly, and `--steps` is the number of timed steps the line reports."""
    from gdb_nerf_amd import synthetic
    from gdb_nerf_amd.engine import HotPathEngine
    rec = _bench(["--path", path], tmp_path)
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["dumped_outputs"]["row_sample"] == "all rows"
    wl = bench.WORKLOADS["c1"]
    frame = synthetic.make_frame(wl["Ho"], wl["Wo"], V=wl["V"], scene=wl["scene"], seed=0)
    eng = HotPathEngine(max_num_samples=wl["S"], is_adaptive=wl["adaptive"], device="cuda:0")
    eng.load_weights(synthetic.make_nerf_weights(seed=0))
    eng.prepare(bench.to_dev(frame, "cuda:0"))
    want = eng.render() if path == "fused" else eng.render_unfused()
    for name, w in zip(("bundle_feat", "bundle_depth", "bundle_opacity"), want):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(w.shape), name
        np.testing.assert_allclose(got, w.cpu().numpy(), rtol=0, atol=1e-5, err_msg=name)


@pytest.mark.gpu
def test_bench_dump_of_the_gathered_row_strips_equals_one_gpu(tmp_path):
    """N = 2 (two ranks sharing the card, GDB_BENCH_REHEARSE=1): rank 0 dumps the all-gathered strips of the last timed step, which
    are the whole frame's render of N = 1."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GDB_BENCH_REHEARSE="1")
    _bench([], tmp_path / "one")
    rec = _bench(["--gpus", "2", "--rows-extra", "", "--full"], tmp_path / "two", env)
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["gathered_equals_full_render"] is True
    for name in ("bundle_feat", "bundle_depth", "bundle_opacity"):
        np.testing.assert_allclose(np.load(tmp_path / "two" / f"{name}.npy"), np.load(tmp_path / "one" / f"{name}.npy"), rtol=0, atol=1e-5,
                                   err_msg=name)


@pytest.mark.gpu
def test_plain_run_carries_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """A plain run times its steps and prints the headline, none of what `--full` measures after them; `--full` (trimmed by
    --no-extras / --no-cpu-baseline) adds the roofline of the dominant kernel, timed in runs of its own."""
    plain = _bench([], tmp_path / "plain")
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "rays/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f32" and plain["steps"] == 3 and plain["warmup"] == 1
    assert not set(plain) & {"roofline", "hbm_frac", "mfma_frac", "secondary", "psnr_delta_db", "peaks_measured", "t_frame_ms", "cpu_baseline"}
    full = _bench(["--full"], tmp_path / "full")
    assert full["dtype"] == plain["dtype"] and full["roofline"]["kernel_ms"] > 0 and 0 < full["mfma_frac"] < 1
    for name in ("bundle_feat", "bundle_depth", "bundle_opacity"):
        np.testing.assert_allclose(np.load(tmp_path / "full" / f"{name}.npy"), np.load(tmp_path / "plain" / f"{name}.npy"), rtol=0, atol=1e-5,
                                   err_msg=name)


@pytest.mark.gpu
def test_plain_two_rank_run_times_its_shard_mode_alone(tmp_path):
    """N = 2 (two ranks sharing the card, GDB_BENCH_REHEARSE=1) without --full: only the --shard mode is timed, none of the other
    mode, the --rows-extra workloads or the per-rank figures; what each mode dumps is still the N = 1 render (rank 0's frame)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GDB_BENCH_REHEARSE="1")
    _bench([], tmp_path / "one")
    only_full = {"independent_frames", "single_frame_rows", "rows_c4", "rows_c5", "rows_per_rank", "per_rank", "gathered_equals_full_render",
                 "value_strong_rows", "value_weak_frames", "roofline", "cpu_baseline"}
    for shard, scaling in (("rows", "strong"), ("frames", "weak")):
        rec = _bench(["--gpus", "2", "--shard", shard], tmp_path / shard, env)
        assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == scaling and rec["value"] > 0 and rec["ms_per_step"] > 0, shard
        assert not set(rec) & only_full, (shard, set(rec) & only_full)
        for name in ("bundle_feat", "bundle_depth", "bundle_opacity"):
            np.testing.assert_allclose(np.load(tmp_path / shard / f"{name}.npy"), np.load(tmp_path / "one" / f"{name}.npy"), rtol=0, atol=1e-5,
                                       err_msg=f"{shard} {name}")
