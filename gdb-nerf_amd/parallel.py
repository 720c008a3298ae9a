"""Multi-GPU sharding of the hot path.  Bundles are independent end to end,
so the only exchange is the all-gather of rendered row strips when ONE frame is split over
the ranks.  One process per GPU; `dist` is torch.distributed (backend "nccl" = RCCL over xGMI
on the GPU box, "gloo" in the CPU tests).

The exchange unit is the PACKED render (`HotPathEngine.render_packed`): one (n_bundles, Q + 2)
tensor whose row is [bundle_feat | depth | opacity], so a rank's strip of rows is one contiguous
block and the whole exchange is ONE `all_gather_into_tensor` — in place when the rows divide
evenly (every BASELINE config does for 1/2/4/8 ranks), through one preallocated padded buffer
otherwise.  No zero-fill, no per-strip copies, depth and opacity included.

`nerf.shard: tiles` shards the decoder and the merge as well: each rank renders its strip plus a halo
(`decode_window`), decodes its strip by row windows (gdb_decode_rows) with one all-gather of the
squeeze-excitation channel sums per dense block (`PartialsGather`), merges its strip and ONE all-gather of
the finished image tiles plus the bundle-resolution depth and opacity (`TileGather`) leaves the frame on
every rank.
"""
from __future__ import annotations

from typing import List, Tuple

import torch


def row_strip(H: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous strip [r0, r1) of bundle-map rows owned by `rank`; sizes differ by at most one
    row, earlier ranks take the longer strips; ranks beyond H get an empty strip."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    base, rem = divmod(H, world)
    r0 = rank * base + min(rank, rem)
    return r0, r0 + base + (1 if rank < rem else 0)


def all_strips(H: int, world: int) -> List[Tuple[int, int]]:
    return [row_strip(H, r, world) for r in range(world)]


class StripGather:
    """All-gather of the row strips of one packed render, with every buffer allocated once.

        g = StripGather(H, W, C, world, rank, device, dist)      # C = Q + 2 floats per bundle
        eng.render_packed(*g.strip, out=g.full)                  # this rank writes rows [r0, r1) of g.full
        g.gather()                                               # afterwards g.full holds all rows on every rank

    H % world == 0 (B == 1): in place — the send buffer is this rank's slice of `full`, the receive buffer is `full`
    itself (the all-gather's own in-place form: send == recv + rank * count).  Otherwise the strip goes through
    one padded (world, rows, W*C) buffer.  `nbytes` is what one rank receives per call (the bus-bandwidth numerator)."""

    def __init__(self, H: int, W: int, C: int, world: int, rank: int, device, dist, dtype=torch.float32, stage_cpu: bool = False,
                 force_padded: bool = False):
        self.H, self.W, self.C, self.world, self.rank, self.dist = H, W, C, world, rank, dist
        # stage_cpu: the collective runs on host copies (gloo cannot move device tensors: the one-GPU rehearsal of bench.py)
        self.stage_cpu = stage_cpu and torch.device(device).type != "cpu"
        self.strip = row_strip(H, rank, world)
        self.full = torch.zeros((H * W, C), dtype=dtype, device=device)
        # force_padded: take the padded form although the rows divide evenly (tests: both collective forms on one rank count)
        self.even = (world == 1 or H % world == 0) and not force_padded
        self.rows = -(-H // world)
        self._rowview = self.full.view(H, W * C)
        if not self.even:
            self._recv = torch.empty((world, self.rows, W * C), dtype=dtype, device=device)
            self._send = torch.zeros((self.rows, W * C), dtype=dtype, device=device)  # pad rows zeroed once, never re-written
        self.nbytes = (world - 1) * self.rows * W * C * self.full.element_size()

    def gather(self, always_collective: bool = False) -> torch.Tensor:
        """always_collective: run the collective at world size 1 as well (a one-rank RCCL communicator then sees exactly the call
        an N-rank job makes, in-place aliasing included: tests/test_parallel.py::test_strip_gather_through_one_rank_rccl)."""
        if self.world == 1 and not always_collective:
            return self.full
        r0, r1 = self.strip
        if self.stage_cpu:
            host = gather_strips(self.full.cpu(), self.H, self.world, self.dist)
            self.full.copy_(host)
            return self.full
        if self.even:
            self.dist.all_gather_into_tensor(self.full.view(-1), self._rowview[r0:r1].reshape(-1))
            return self.full
        self._send[: r1 - r0].copy_(self._rowview[r0:r1])
        self.dist.all_gather_into_tensor(self._recv.view(-1), self._send.view(-1))
        for r, (a, b) in enumerate(all_strips(self.H, self.world)):
            if r != self.rank and b > a:
                self._rowview[a:b].copy_(self._recv[r, : b - a])
        return self.full


def gather_strips(full: torch.Tensor, H: int, world: int, dist, B: int = 1) -> torch.Tensor:
    """General form for any per-bundle tensor `full` ((B*H*W, C) or (B*H*W,)) and batch B: on entry each rank has
    written only its own strip of every batch item; on return every rank holds all rows.  Allocates its padded
    buffers per call — the engine path uses StripGather."""
    if world == 1:
        return full
    rank = dist.get_rank()
    v = full.view(B, H, -1)  # (B, H, W*C)
    rows = -(-H // world)
    r0, r1 = row_strip(H, rank, world)
    send = torch.zeros((B, rows, v.shape[2]), dtype=full.dtype, device=full.device)
    send[:, : r1 - r0] = v[:, r0:r1]
    recv = torch.empty((world,) + tuple(send.shape), dtype=full.dtype, device=full.device)
    dist.all_gather_into_tensor(recv.view(-1), send.view(-1))
    for r, (a, b) in enumerate(all_strips(H, world)):
        if r != rank and b > a:
            v[:, a:b] = recv[r][:, : b - a]
    return full


# ---- nerf.shard: tiles ------------------------------------------------------------------------------------------------------------
WINDOW_ALIGN = 4   # the decoder's window starts on a multiple of every workgroup tile height (gdb_decoder.hip DEC_WIN_ALIGN)
SE_FEATS = 64      # channels of the decoder's squeeze-excitation sums


def decoder_halo(b: int, num_layers: int) -> int:
    """Bundle rows a strip's decode window reaches beyond the strip: one per 3x3 convolution (in_conv, three per dense block, the
    up stage; at b = 4 the last convolution runs at 2H and rounds up to a whole bundle row) - gdb_decoder.hip dec_halo."""
    if b not in (2, 4):
        raise ValueError(f"the HIP decoder serves bundle sizes 2 and 4, got {b}")
    if not 1 <= num_layers <= 16:
        raise ValueError(f"decoder layers {num_layers} outside 1..16")
    return 1 + 3 * num_layers + (b.bit_length() - 1)


def decode_window(H: int, rank: int, world: int, halo: int, align: int = WINDOW_ALIGN) -> Tuple[int, int]:
    """Bundle-map rows [w0, w1) that `rank` renders and decodes for its strip: the strip plus `halo` rows each side, clipped to the
    frame, the start rounded down to `align` (what gdb_decoder_rows_layout reports).  An empty strip has an empty window."""
    r0, r1 = row_strip(H, rank, world)
    if r0 == r1:
        return r0, r0
    return max(0, r0 - halo) // align * align, min(H, r1 + halo)


def se_partial_pitch(W: int) -> int:
    """Floats per bundle row of the decoder's channel-sum buffer: 64 per 32-pixel segment."""
    return SE_FEATS * (-(-W // 32))


class PartialsGather:
    """All-gather of the decoder's squeeze-excitation channel sums between the phases of a row-window decode.

        g = PartialsGather(dec.part, world, rank, dist)   # dec.part: (B, H, P) floats inside the rank's decode workspace
        dec.run_phase(packed, p)                          # writes the rank's rows [r0, r1) of every batch item
        g.gather()                                        # afterwards every row is there, on every rank

    B == 1 and H % world == 0: in place (the send buffer is the rank's rows of `part`).  Otherwise through one padded
    (world, B, rows, P) buffer.  `nbytes` is what one rank receives per call."""

    def __init__(self, part: torch.Tensor, world: int, rank: int, dist, stage_cpu: bool = False, force_padded: bool = False):
        self.part, self.world, self.rank, self.dist = part, world, rank, dist
        self.B, self.H, self.P = part.shape
        self.stage_cpu = stage_cpu and part.device.type != "cpu"
        self.strip = row_strip(self.H, rank, world)
        self.even = (world == 1 or (self.B == 1 and self.H % world == 0)) and not force_padded
        self.rows = -(-self.H // world)
        if not self.even:
            self._send = torch.zeros((self.B, self.rows, self.P), dtype=part.dtype, device=part.device)
            self._recv = torch.empty((world, self.B, self.rows, self.P), dtype=part.dtype, device=part.device)
        self.nbytes = (world - 1) * self.B * self.rows * self.P * part.element_size()

    def gather(self) -> torch.Tensor:
        if self.world == 1:
            return self.part
        r0, r1 = self.strip
        if self.stage_cpu:
            self.part.copy_(gather_strips(self.part.cpu(), self.H, self.world, self.dist, B=self.B))
        elif self.even:
            self.dist.all_gather_into_tensor(self.part.view(-1), self.part[0, r0:r1].reshape(-1))
        else:
            self._send[:, : r1 - r0].copy_(self.part[:, r0:r1])
            self.dist.all_gather_into_tensor(self._recv.view(-1), self._send.view(-1))
            for r, (a, e) in enumerate(all_strips(self.H, self.world)):
                if r != self.rank and e > a:
                    self.part[:, a:e] = self._recv[r, :, : e - a]
        return self.part


class TileGather:
    """The one exchange of finished work: every rank's image tile (B, 3, rows b, W b) and its bundle-resolution depth and opacity
    (B, rows, W, 2) - 3 b^2 + 2 floats per bundle - in one slot per rank of a (world, slot) buffer.  The rank writes its slot
    (`tile`, `maps`); `gather()` all-gathers the slots in place (send = the rank's slot of the receive buffer) and assembles the
    frame's image (B, 3, H b, W b) and maps (B H W, 2).  Slots hold ceil(H / world) rows: exact when the rows divide evenly,
    padded otherwise.  `nbytes` is what one rank receives."""

    def __init__(self, B: int, H: int, W: int, b: int, world: int, rank: int, device, dist, stage_cpu: bool = False):
        self.B, self.H, self.W, self.b, self.world, self.rank, self.dist = B, H, W, b, world, rank, dist
        self.stage_cpu = stage_cpu and torch.device(device).type != "cpu"
        self.strip = row_strip(H, rank, world)
        self.rows = -(-H // world)
        self.n_img, self.n_maps = B * 3 * self.rows * b * W * b, B * self.rows * W * 2
        self.slots = torch.zeros((world, self.n_img + self.n_maps), dtype=torch.float32, device=device)
        self.tile = self._tile(rank)
        self.maps = self._maps(rank)
        self.nbytes = (world - 1) * (self.n_img + self.n_maps) * self.slots.element_size()

    def _tile(self, r: int) -> torch.Tensor:
        return self.slots[r, : self.n_img].view(self.B, 3, self.rows * self.b, self.W * self.b)

    def _maps(self, r: int) -> torch.Tensor:
        return self.slots[r, self.n_img:].view(self.B, self.rows, self.W, 2)

    def gather(self, img: torch.Tensor = None):
        B, H, W, b = self.B, self.H, self.W, self.b
        if self.world > 1:
            if self.stage_cpu:   # gloo moves host tensors (its own send buffer: no aliasing assumed of it)
                host = self.slots.cpu()
                self.dist.all_gather_into_tensor(host.view(-1), host[self.rank].clone())
                self.slots.copy_(host)
            else:
                self.dist.all_gather_into_tensor(self.slots.view(-1), self.slots[self.rank])
        if img is None:
            img = torch.empty((B, 3, H * b, W * b), dtype=torch.float32, device=self.slots.device)
        maps = torch.empty((B, H, W, 2), dtype=torch.float32, device=self.slots.device)
        for r, (a, e) in enumerate(all_strips(H, self.world)):
            if e > a:
                img[:, :, a * b: e * b] = self._tile(r)[:, :, : (e - a) * b]
                maps[:, a:e] = self._maps(r)[:, : e - a]
        return img, maps.view(B * H * W, 2)
