"""`nerf.shard: tiles`: the decoder and the merge sharded by bundle-map row strips, one all-gather of the decoder's
squeeze-excitation sums per dense block and ONE all-gather of the finished image tiles (gdb_decode_rows,
gdb_merge_packed_rows, gdb_upsample_maps; parallel.decode_window / PartialsGather / TileGather; Network._forward_tiles).
CPU: the window arithmetic, the C ABI's host-side checks, both gathers over gloo and the network's call sequence on a fake
engine.  GPU: emulated ranks bit-identical to the whole-frame decode and merge, and two gloo ranks on one card."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_golden
from gdb_nerf_amd import _lib
from gdb_nerf_amd.parallel import (PartialsGather, TileGather, all_strips, decode_window, decoder_halo, row_strip,
                                   se_partial_pitch)
from test_parallel import _free_port


# ---- window arithmetic ---------------------------------------------------------------------------------------------------------
def test_decoder_halo():
    assert decoder_halo(2, 3) == 11 and decoder_halo(4, 3) == 12
    assert decoder_halo(2, 1) == 5 and decoder_halo(4, 16) == 51
    for b, L in ((1, 3), (8, 3), (2, 0), (2, 17)):
        with pytest.raises(ValueError):
            decoder_halo(b, L)


@pytest.mark.parametrize("H,world", [(256, 8), (600, 8), (37, 5), (37, 3), (10, 4), (3, 8), (1, 2), (64, 1), (150, 7)])
@pytest.mark.parametrize("b,L", [(2, 3), (4, 3), (2, 1), (4, 5)])
def test_windows_cover_the_frame_and_strips_are_disjoint(H, world, b, L):
    halo = decoder_halo(b, L)
    strips = all_strips(H, world)
    covered = np.zeros(H, dtype=int)
    owned = np.zeros(H, dtype=int)
    for rank, (r0, r1) in enumerate(strips):
        w0, w1 = decode_window(H, rank, world, halo)
        owned[r0:r1] += 1
        if r0 == r1:
            assert (w0, w1) == (r0, r0)
            continue
        assert w0 % 4 == 0 and 0 <= w0 <= r0 and r1 <= w1 <= H
        assert w0 == 0 or r0 - w0 >= halo
        assert w1 == H or w1 - r1 == halo
        covered[w0:w1] += 1
    assert (owned == 1).all()                      # the strips partition the rows
    assert (covered >= 1).all()                    # the windows cover the frame


# ---- C ABI: host-side checks, no launch --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gdb_nerf_amd import build
    build.build()
    return _lib.load()


def _cfg(b=2):
    return _lib.GdbConfig(b, 3, 1, 0, 64, 3, 16, 8, 64, 1)


def _shape(B=1, H=64, W=80, b=2):
    return _lib.GdbFrame(B, 3, H * b, W * b, H, W, 8, *([None] * 10))


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("B,H,W,L", [(1, 64, 80, 3), (2, 37, 45, 1), (1, 300, 400, 5)])
def test_rows_workspace_and_layout(lib, b, B, H, W, L):
    cfg, sh = _cfg(b), _shape(B, H, W, b)
    whole, n = C.c_size_t(), C.c_size_t()
    _lib.check(lib.gdb_decoder_workspace_bytes(C.byref(cfg), C.byref(sh), C.byref(whole)))
    _lib.check(lib.gdb_decoder_rows_workspace_bytes(C.byref(cfg), C.byref(sh), 0, H, L, C.byref(n)))
    assert n.value == whole.value                  # the whole frame as one window: gdb_decode's workspace
    for world in (2, 3, 8):
        for rank in range(world):
            r0, r1 = row_strip(H, rank, world)
            if r0 == r1:
                continue
            off, pitch, w0, w1 = C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_int32()
            _lib.check(lib.gdb_decoder_rows_workspace_bytes(C.byref(cfg), C.byref(sh), r0, r1, L, C.byref(n)))
            _lib.check(lib.gdb_decoder_rows_layout(C.byref(cfg), C.byref(sh), r0, r1, L, C.byref(off), C.byref(pitch), C.byref(w0), C.byref(w1)))
            assert (w0.value, w1.value) == decode_window(H, rank, world, decoder_halo(b, L))
            assert pitch.value == 4 * se_partial_pitch(W)
            assert off.value % 256 == 0 and off.value + B * H * pitch.value <= n.value
            assert n.value <= whole.value


def test_rows_entries_refuse_bad_arguments_on_the_host(lib):
    cfg, sh = _cfg(), _shape()
    n = C.c_size_t()
    fake = 256   # never dereferenced: every call below fails its host-side checks first

    def rows(r0, r1, phase, cfg=cfg, prec=1, L=3, ptr=fake):
        return lib.gdb_decode_rows(C.byref(cfg), C.byref(sh), ptr, 41, ptr, L, prec, r0, r1, phase, ptr, 1 << 40, ptr, None)

    for phase in (-1, 4, 100):
        assert rows(0, 16, phase) == _lib.GDB_E_BADARG
    assert rows(16, 16, 0) == _lib.GDB_E_BADARG and rows(20, 10, 1) == _lib.GDB_E_BADARG
    assert rows(-1, 10, 0) == _lib.GDB_E_SHAPE and rows(10, 65, 0) == _lib.GDB_E_SHAPE
    assert rows(0, 16, 0, cfg=_cfg(1)) == _lib.GDB_E_BADARG                      # b = 1: no HIP decoder
    assert rows(0, 16, 0, prec=0) == _lib.GDB_E_BADARG
    assert rows(0, 16, 0, L=17) == _lib.GDB_E_BADARG
    assert rows(0, 16, 1, ptr=None) == _lib.GDB_E_BADARG
    assert lib.gdb_decode_rows(C.byref(cfg), C.byref(sh), fake, 41, fake, 3, 1, 0, 16, 0, fake, 1024, fake, None) == _lib.GDB_E_WORKSPACE
    assert lib.gdb_decoder_rows_workspace_bytes(C.byref(_cfg(1)), C.byref(sh), 0, 16, 3, C.byref(n)) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_rows_workspace_bytes(C.byref(cfg), C.byref(sh), 8, 8, 3, C.byref(n)) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_rows_workspace_bytes(C.byref(cfg), C.byref(sh), 0, 65, 3, C.byref(n)) == _lib.GDB_E_SHAPE
    assert lib.gdb_decoder_rows_layout(C.byref(cfg), C.byref(sh), 0, 16, 0, None, None, None, None) == _lib.GDB_E_BADARG
    assert lib.gdb_merge_packed_rows(C.byref(cfg), C.byref(sh), fake, None, 0, 5, 5, 8, fake, None) == _lib.GDB_E_BADARG
    assert lib.gdb_merge_packed_rows(C.byref(cfg), C.byref(sh), fake, None, 0, 0, 16, 8, fake, None) == _lib.GDB_E_SHAPE
    assert lib.gdb_upsample_maps(C.byref(cfg), C.byref(sh), fake, 1, fake, fake, None) == _lib.GDB_E_BADARG


# ---- the two gathers over gloo -----------------------------------------------------------------------------------------------------
def _gather_worker(rank, world, port, B, H, W, b, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ok = True
        r0, r1 = row_strip(H, rank, world)
        P = se_partial_pitch(W)
        truth = torch.arange(B * H * P, dtype=torch.float32).view(B, H, P)
        for padded in (False, True):
            part = torch.full((B, H, P), float("nan"))
            g = PartialsGather(part, world, rank, dist, force_padded=padded)
            for rep in range(2):     # buffers reused phase after phase
                part.fill_(float("nan"))
                part[:, r0:r1] = truth[:, r0:r1] + rep
                ok = ok and g.gather() is part and bool(torch.equal(part, truth + rep))
            ok = ok and g.even == (not padded and (world == 1 or (B == 1 and H % world == 0)))
            ok = ok and g.nbytes == (world - 1) * B * (-(-H // world)) * P * 4
        img = torch.arange(B * 3 * H * b * W * b, dtype=torch.float32).view(B, 3, H * b, W * b)
        maps = -torch.arange(B * H * W * 2, dtype=torch.float32).view(B, H, W, 2)
        t = TileGather(B, H, W, b, world, rank, "cpu", dist)
        for rep in range(2):
            t.slots.fill_(float("nan"))
            t.tile[:, :, : (r1 - r0) * b] = img[:, :, r0 * b: r1 * b] + rep
            t.maps[:, : r1 - r0] = maps[:, r0:r1] + rep
            got_img, got_maps = t.gather()
            ok = ok and bool(torch.equal(got_img, img + rep)) and bool(torch.equal(got_maps, (maps + rep).view(B * H * W, 2)))
        ok = ok and t.nbytes == (world - 1) * B * (-(-H // world)) * W * (3 * b * b + 2) * 4
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args, timeout=180):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=timeout) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,B,H,W,b", [(2, 1, 8, 5, 2), (2, 1, 7, 40, 2), (3, 2, 6, 33, 4), (3, 1, 7, 3, 2), (2, 2, 9, 4, 2), (3, 1, 2, 6, 2)])
def test_partials_and_tile_gathers_gloo(world, B, H, W, b):
    """Even and uneven H, B = 1 and 2, a world larger than H: both gathers leave every rank with the full buffers."""
    assert _spawn(_gather_worker, world, B, H, W, b) == [(r, True) for r in range(world)]


# ---- Network._forward_tiles on a fake engine ---------------------------------------------------------------------------------------
class _FakeDecodeRows:
    """Stands in for engine.DecodeRows: writes its strip's rows of `part` per phase and checks, at every phase after the first, that
    the exchange left every rank's rows of the previous phase in `part`."""

    def __init__(self, eng, r0, r1):
        self.eng, self.r0, self.r1 = eng, r0, r1
        B, H, W, b, L = eng.B, eng.H, eng.W, eng.b, eng.L
        h = decoder_halo(b, L)
        self.window = (max(0, r0 - h) // 4 * 4, min(H, r1 + h))
        self.phases = L + 1
        self.part = torch.full((B, H, se_partial_pitch(W)), float("nan"))
        self.rgb_c = torch.full((B, 3, H * b, W * b), float("nan"))

    def expect(self, p):
        return torch.arange(self.part.numel(), dtype=torch.float32).view(self.part.shape) + 1000.0 * p

    def run_phase(self, packed, p):
        eng = self.eng
        eng.calls.append(("phase", p))
        w0, w1 = self.window
        v = packed.view(eng.B, eng.H, -1)
        eng.ok &= bool(torch.equal(v[:, w0:w1], eng.truth.view(eng.B, eng.H, -1)[:, w0:w1]))   # the window was rendered
        if p > 0:
            eng.ok &= bool(torch.equal(self.part, self.expect(p - 1)))
        if p < eng.L:
            self.part[:, self.r0:self.r1] = self.expect(p)[:, self.r0:self.r1]
            return None
        b = eng.b
        self.rgb_c[:, :, self.r0 * b: self.r1 * b] = eng.rgb_c_full[:, :, self.r0 * b: self.r1 * b]
        return self.rgb_c


class _FakeTilesEngine:
    def __init__(self, truth, B, H, W, b, L):
        self.truth, self.B, self.H, self.W, self.b, self.L = truth, B, H, W, b, L
        self.Q, self.device, self.fused_supported = truth.shape[1] - 2, torch.device("cpu"), True
        self.calls, self.ok = [], True
        self.rgb_c_full = torch.randn(B, 3, H * b, W * b, generator=torch.Generator().manual_seed(1))

    def render_packed(self, r0, r1, precision, out):
        self.calls.append(("render", r0, r1))
        out.view(self.B, self.H, -1)[:, r0:r1] = self.truth.view(self.B, self.H, -1)[:, r0:r1]
        return out

    def decoder_rows(self, r0, r1):
        return _FakeDecodeRows(self, r0, r1)

    def merge_packed_rows(self, packed, rgb_c, reweighting, r0, r1, tile):
        self.calls.append(("merge", r0, r1))
        b = self.b
        tile[:, :, : (r1 - r0) * b] = rgb_c[:, :, r0 * b: r1 * b] + 1.0
        return tile

    def upsample_maps(self, maps):
        self.calls.append(("upsample",))
        up = lambda m: m.view(self.B, self.H, self.W).repeat_interleave(self.b, 1).repeat_interleave(self.b, 2)
        return up(maps[:, 0].contiguous()), up(maps[:, 1].contiguous())


def _network_worker(rank, world, port, B, H, W, b, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gdb_nerf_amd.parallel as par
        from gdb_nerf_amd.configs import make_cfg
        from gdb_nerf_amd.networks import make_network
        counts = {"partials": 0, "tiles": 0}
        pg, tg = par.PartialsGather.gather, par.TileGather.gather
        par.PartialsGather.gather = lambda self: (counts.__setitem__("partials", counts["partials"] + 1), pg(self))[1]
        par.TileGather.gather = lambda self, *a: (counts.__setitem__("tiles", counts["tiles"] + 1), tg(self, *a))[1]
        net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.shard", "tiles", "nerf.bundle_size", str(b)])).eval()
        L = int(net.dec_layers)
        ok = net.shard == "tiles" and net._dist() is dist
        r0, r1 = row_strip(H, rank, world)
        w0, w1 = decode_window(H, rank, world, decoder_halo(b, L))
        Q = 3 * b * b + 27
        for rep in range(2):   # buffers cached per shape and reused frame after frame
            truth = torch.arange(B * H * W * (Q + 2), dtype=torch.float32).view(B * H * W, Q + 2) + 1000.0 * rep
            eng = _FakeTilesEngine(truth, B, H, W, b, L)
            counts.update(partials=0, tiles=0)
            img, dep, opa = net._forward_tiles(eng, B, H, W, dist)
            want_calls = ([("render", w0, w1)] + [("phase", p) for p in range(L + 1)] + [("merge", r0, r1)]) if r1 > r0 else []
            ok = ok and eng.ok and eng.calls == want_calls + [("upsample",)]
            ok = ok and counts == {"partials": L, "tiles": 1}
            ok = ok and bool(torch.equal(img, eng.rgb_c_full + 1.0))
            up = lambda m: m.view(B, H, W).repeat_interleave(b, 1).repeat_interleave(b, 2)
            ok = ok and bool(torch.equal(dep, up(truth[:, Q]))) and bool(torch.equal(opa, up(truth[:, Q + 1])))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,B,H,W,b", [(2, 1, 40, 5, 2), (2, 2, 27, 4, 2), (3, 1, 50, 3, 4), (3, 1, 2, 4, 2)])
def test_network_tiles_sequence_on_a_fake_engine(world, B, H, W, b):
    """Each rank renders its window, runs num_layers + 1 decode phases with one partial-sums exchange between each, merges its strip,
    and ONE tile gather leaves the whole frame (image, upsampled depth and opacity) on every rank; a rank with an empty strip (H < world)
    only takes part in the collectives."""
    assert _spawn(_network_worker, world, B, H, W, b) == [(r, True) for r in range(world)]


def test_tiles_config_is_refused_without_the_hip_decoder():
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    net = lambda *o: make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.shard", "tiles", *o]))
    assert net().shard == "tiles" and net("nerf.bundle_size", "4").shard == "tiles"
    for opts in (("nerf.hip_decoder", "False"), ("nerf.bundle_size", "1"), ("nerf.dec_layers", "17")):
        with pytest.raises(ValueError, match="tiles.*hip_decoder"):
            net(*opts)
    with pytest.raises(ValueError, match="tiles.*fused"):
        net("nerf.hot_path", "mirrors")
    with pytest.raises(ValueError, match="tiles"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.shard", "tile"]))
    assert net()._dist() is None     # no process group: tiles renders whole frames, as rows does


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def _decoder_engine(b, L, B, H, W):
    from gdb_nerf_amd import synthetic
    from gdb_nerf_amd.engine import HotPathEngine
    from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder
    key = (b, L, B, H, W)
    if key not in _ENGINES:
        torch.manual_seed(3 + L)
        dec = Decoder(27, 3, num_feats=64, num_layers=L, upscale_factor=b).eval()
        with torch.no_grad():
            for p in dec.parameters():      # biases and gates that matter
                p.mul_(1.5)
        frame = synthetic.make_frame(b * H, b * W, V=2, B=B, bundle_size=b, seed=1)
        eng = HotPathEngine(bundle_size=b)
        eng.prepare({k: torch.from_numpy(v).cuda() for k, v in frame.items()})
        eng.load_decoder_weights({k: v.detach() for k, v in dec.state_dict().items()}, L)
        _ENGINES.clear()
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("b,L,B,H,W", [(2, 3, 1, 64, 40), (2, 1, 2, 37, 45), (2, 5, 1, 90, 33), (2, 3, 2, 21, 70),
                                       (4, 3, 1, 48, 20), (4, 1, 2, 29, 24), (4, 5, 1, 70, 16)])
def test_emulated_ranks_decode_bit_identical_to_the_whole_frame(b, L, B, H, W):
    """G ranks in one process, G in {1, 2, 3, 4, 8}, both precisions: each rank's decode sees only its window of the bundle rows
    (NaN elsewhere) and a NaN-filled workspace; between phases the owned rows of `part` are copied between the G workspaces (the
    all-gather).  The stitched rgb_c must equal gdb_decode on the whole frame bit for bit; the strip merge and the map upsampling
    must equal gdb_merge_packed bit for bit."""
    eng = _decoder_engine(b, L, B, H, W)
    Q = eng.Q
    torch.manual_seed(11)
    packed = torch.randn(B * H * W, Q + 2, device="cuda")
    packed[:, Q:] = torch.rand(B * H * W, 2, device="cuda") * 4.0
    for prec in (1, 2):
        want = eng.decode(packed, precision=prec).clone()
        want_img, want_dep, want_opa = (t.clone() for t in eng.merge_packed(packed, want, reweighting=False))
        for G in (1, 2, 3, 4, 8):
            decs, inputs = [], []
            for g in range(G):
                r0, r1 = row_strip(H, g, G)
                if r0 == r1:
                    continue
                d = eng.decoder_rows(r0, r1)
                assert d.window == decode_window(H, g, G, decoder_halo(b, L)) and d.phases == L + 1
                d.ws.view(torch.float32).fill_(float("nan"))
                d.rgb_c.fill_(float("nan"))
                mine = torch.full_like(packed, float("nan"))
                w0, w1 = d.window
                mine.view(B, H, W, -1)[:, w0:w1] = packed.view(B, H, W, -1)[:, w0:w1]
                decs.append(d)
                inputs.append(mine)
            for p in range(L + 1):
                if p:
                    for d in decs:
                        for e in decs:
                            if e is not d:
                                d.part[:, e.r0:e.r1] = e.part[:, e.r0:e.r1]
                for d, mine in zip(decs, inputs):
                    out = d.run_phase(mine, p, precision=prec)
                    assert (out is None) == (p < L)
            got = torch.full_like(want, float("nan"))
            img = torch.full_like(want_img, float("nan"))
            rows = -(-H // G)
            for d, mine in zip(decs, inputs):
                got[:, :, d.r0 * b: d.r1 * b] = d.rgb_c[:, :, d.r0 * b: d.r1 * b]
                tile = torch.full((B, 3, rows * b, W * b), float("nan"), device="cuda")
                eng.merge_packed_rows(mine, d.rgb_c, False, d.r0, d.r1, tile)
                img[:, :, d.r0 * b: d.r1 * b] = tile[:, :, : (d.r1 - d.r0) * b]
            torch.cuda.synchronize()
            assert torch.equal(got, want), (prec, G, float((got - want).abs().nan_to_num(1e30).max()))
            assert torch.equal(img, want_img), (prec, G)
        dep, opa = eng.upsample_maps(packed[:, Q:].contiguous())
        assert torch.equal(dep, want_dep) and torch.equal(opa, want_opa)


def _batch(fx, dev):
    t = lambda k: torch.from_numpy(fx[k].astype(np.float32) if fx[k].dtype == np.float16 else fx[k]).to(dev)
    return {"src_views": {"rgb": t("src_images"), "extrinsics": t("src_exts"), "intrinsics": t("src_ints")},
            "tar_views": {"extrinsics": t("tar_ext"), "intrinsics": t("tar_int")}, "near_far": t("near_far")}


def _net(fx, shard, precision):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    opts = [str(x) for x in fx["opts"]] if "opts" in fx else []
    net = make_network(make_cfg("configs/dtu_eval.yaml", opts + ["nerf.shard", shard, "nerf.precision", precision])).eval()
    sd = {k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in fx.items() if k.startswith("sd.")}
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def _tiles_worker(rank, world, port, fixture, precision, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fx = load_golden(fixture)
        net = _net(fx, "tiles", precision)
        with torch.no_grad():
            for _ in range(2):     # buffers reused frame after frame
                out = net(_batch(fx, "cuda"))[0]
        st = net._tiles_state
        q.put((rank, {k: v.cpu().numpy() for k, v in out.items()}, st["partials"].nbytes, st["tiles"].nbytes, st["partials"].P,
               tuple(st["dec"].window)))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,precision", [("F7_network", "f32"), ("F7_network", "f32x"), ("F7d_network_bundle4", "f32")])
def test_network_tiles_two_ranks_on_one_gpu_equal_shard_none(fixture, precision):
    """Network.forward with `nerf.shard: tiles` on two gloo ranks spawned on the one card: rgb, nerf_depth and opacity equal
    `shard: none` on the same inputs and weights bit for bit, mvs_depth is unchanged, and each rank receives 3 b^2 + 2 floats per
    bundle of the other rank's tile plus the squeeze-excitation sums of its rows once per dense block."""
    fx = load_golden(fixture)
    ref = _net(fx, "none", precision)
    with torch.no_grad():
        want = {k: v.cpu().numpy() for k, v in ref(_batch(fx, "cuda"))[0].items()}
    B, _, Ho, Wo = want["rgb"].shape
    b = ref.b_size
    H, W, L = Ho // b, Wo // b, int(ref.dec_layers)
    res = _spawn(_tiles_worker, 2, fixture, precision, timeout=600)
    for rank, out, part_bytes, tile_bytes, P, window in res:
        assert window == decode_window(H, rank, 2, decoder_halo(b, L))
        for k in want:
            assert np.array_equal(out[k], want[k]), (rank, k)
        rows = -(-H // 2)
        assert tile_bytes == rows * W * B * (3 * b * b + 2) * 4
        assert P == se_partial_pitch(W) and part_bytes == B * rows * P * 4
