"""`nerf.shard: tiles` against `nerf.shard: rows`: the per-rank compute of one frame split over G ranks, every rank's share run in
turn on ONE GPU (no collective is timed), plus the bytes each rank would exchange.

    python tools/bench_shard_tiles.py [--workloads c2,c5] [--precisions f32,f32x] [--ranks 1,2,4,8] [--reps 5] [--out FILE]

Per rank, timed with HIP events (median of --reps after two warm-up runs):
  tiles: prepare(rows = strip + decoder halo), render_packed(window), the num_layers + 1 decode phases (gdb_decode_rows), the strip
         merge (gdb_merge_packed_rows), and the upsampling of the gathered depth / opacity (every rank runs it on the full maps);
  rows:  prepare(rows = strip), render_packed(strip), then the whole-frame decode and merge every rank runs after the exchange.
The record carries the max over ranks of each, and the bytes one rank sends / receives per collective of either mode.
Random decoder weights (Decoder(27, 3, 64, 3 blocks, x2)); synthetic frames as bench.py's workloads."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdb_nerf_amd import _lib, synthetic  # noqa: E402
from gdb_nerf_amd.engine import HotPathEngine  # noqa: E402
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder  # noqa: E402
from gdb_nerf_amd.parallel import decode_window, decoder_halo, row_strip, se_partial_pitch  # noqa: E402

WORKLOADS = {"c2": dict(Ho=512, Wo=640, V=3, S=3, adaptive=True, scene="dtu"),
             "c5": dict(Ho=1200, Wo=1600, V=5, S=6, adaptive=False, scene="dtu")}
PREC = {"f32": _lib.PREC_F32, "f32x": _lib.PREC_F32X}


def timed(fn, reps):
    """Median ms of fn() over reps runs after two warm-up runs; fn returns a list of (name, start, end) event pairs."""
    out = {}
    for i in range(reps + 2):
        ev = fn()
        torch.cuda.synchronize()
        if i >= 2:
            for name, a, b in ev:
                out.setdefault(name, []).append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in out.items()}


def ev():
    return torch.cuda.Event(enable_timing=True)


def bench(name, prec, G, reps, L=3, b=2):
    wl = WORKLOADS[name]
    Ho, Wo = wl["Ho"], wl["Wo"]
    H, W = Ho // b, Wo // b
    frame = {k: torch.from_numpy(v).cuda() for k, v in synthetic.make_frame(Ho, Wo, V=wl["V"], scene=wl["scene"], seed=0).items()}
    eng = HotPathEngine(max_num_samples=wl["S"], is_adaptive=wl["adaptive"], device="cuda")
    eng.load_weights(synthetic.make_nerf_weights(seed=0))
    torch.manual_seed(0)
    dec = Decoder(27, 3, num_feats=64, num_layers=L, upscale_factor=b).eval()
    eng.load_decoder_weights({k: v.detach() for k, v in dec.state_dict().items()}, L)
    eng.precision = PREC[prec]
    Q = eng.Q
    halo = decoder_halo(b, L)
    packed = torch.zeros((H * W, Q + 2), device="cuda")
    ranks = []
    for g in range(G):
        r0, r1 = row_strip(H, g, G)
        w0, w1 = decode_window(H, g, G, halo)
        rows_tile = -(-H // G)
        tile = torch.empty((1, 3, rows_tile * b, Wo), device="cuda")
        maps = torch.empty((H * W, 2), device="cuda")
        eng.prepare(frame, rows=(w0, w1))
        d = eng.decoder_rows(r0, r1)

        def tiles_step():
            e = [ev() for _ in range(2 * (L + 5))]
            e[0].record(); eng.prepare(frame, rows=(w0, w1)); e[1].record()
            e[2].record(); eng.render_packed(w0, w1, None, packed); e[3].record()
            rgb_c = None
            for p in range(L + 1):
                e[4 + 2 * p].record(); rgb_c = d.run_phase(packed, p); e[5 + 2 * p].record()
            k = 4 + 2 * (L + 1)
            e[k].record(); eng.merge_packed_rows(packed, rgb_c, False, r0, r1, tile); e[k + 1].record()
            e[k + 2].record(); eng.upsample_maps(maps); e[k + 3].record()
            return ([("prepare", e[0], e[1]), ("render", e[2], e[3])] + [(f"decode_phase_{p}", e[4 + 2 * p], e[5 + 2 * p]) for p in range(L + 1)]
                    + [("merge_strip", e[k], e[k + 1]), ("upsample_maps", e[k + 2], e[k + 3])])

        def rows_step():
            e = [ev() for _ in range(8)]
            e[0].record(); eng.prepare(frame, rows=(r0, r1)); e[1].record()
            e[2].record(); eng.render_packed(r0, r1, None, packed); e[3].record()
            e[4].record(); rgb_c = eng.decode(packed); e[5].record()
            e[6].record(); eng.merge_packed(packed, rgb_c, False); e[7].record()
            return [("prepare", e[0], e[1]), ("render", e[2], e[3]), ("decode", e[4], e[5]), ("merge", e[6], e[7])]

        t = timed(tiles_step, reps)
        t["decode"] = sum(t[f"decode_phase_{p}"] for p in range(L + 1))
        t["total"] = t["prepare"] + t["render"] + t["decode"] + t["merge_strip"] + t["upsample_maps"]
        eng.prepare(frame, rows=(r0, r1))
        r = timed(rows_step, reps)
        r["total"] = sum(r.values())
        ranks.append({"rank": g, "strip": [r0, r1], "window": [w0, w1], "tiles_ms": t, "rows_ms": r})
        del d
    rows = -(-H // G)
    P = se_partial_pitch(W)
    f4 = 4
    exchange = {
        "tiles": {"se_partials_allgather": {"calls_per_frame": L, "send_bytes": rows * P * f4, "recv_bytes": (G - 1) * rows * P * f4},
                  "tile_allgather": {"calls_per_frame": 1, "floats_per_bundle": 3 * b * b + 2, "send_bytes": rows * W * (3 * b * b + 2) * f4,
                                     "recv_bytes": (G - 1) * rows * W * (3 * b * b + 2) * f4}},
        "rows": {"packed_allgather": {"calls_per_frame": 1, "floats_per_bundle": Q + 2, "send_bytes": rows * W * (Q + 2) * f4,
                                      "recv_bytes": (G - 1) * rows * W * (Q + 2) * f4}},
    }
    exchange["tiles"]["recv_bytes_per_frame"] = L * exchange["tiles"]["se_partials_allgather"]["recv_bytes"] + exchange["tiles"]["tile_allgather"]["recv_bytes"]
    exchange["rows"]["recv_bytes_per_frame"] = exchange["rows"]["packed_allgather"]["recv_bytes"]
    mx = lambda mode, key: max(rk[mode][key] for rk in ranks)
    tkeys = ["prepare", "render"] + [f"decode_phase_{p}" for p in range(L + 1)] + ["decode", "merge_strip", "upsample_maps", "total"]
    return {"workload": name, "Ho": Ho, "Wo": Wo, "H": H, "W": W, "bundle_size": b, "dec_layers": L, "halo_rows": halo, "precision": prec,
            "ranks": G, "max_over_ranks_ms": {"tiles": {k: mx("tiles_ms", k) for k in tkeys},
                                               "rows": {k: mx("rows_ms", k) for k in ("prepare", "render", "decode", "merge", "total")}},
            "exchange_per_rank": exchange, "per_rank": ranks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c5")
    ap.add_argument("--precisions", default="f32,f32x")
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_shard_tiles.py needs a GPU")
    recs = []
    for name in a.workloads.split(","):
        for prec in a.precisions.split(","):
            for G in [int(x) for x in a.ranks.split(",")]:
                rec = bench(name, prec, G, a.reps)
                recs.append(rec)
                m = rec["max_over_ranks_ms"]
                print(f"{name} {prec} G={G}: tiles {m['tiles']['total']:.3f} ms (decode {m['tiles']['decode']:.3f}) vs rows "
                      f"{m['rows']['total']:.3f} ms (decode {m['rows']['decode']:.3f}) per rank", file=sys.stderr)
    out = {"what": "per-rank compute of nerf.shard tiles vs rows, every rank's share run in turn on ONE GPU; no collective was timed "
                   "(exchange_per_rank gives the bytes each collective would move); not a multi-GPU measurement",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "statistic": "median of reps per step, then max over ranks",
           "records": recs}
    s = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(json.dumps({"what": out["what"], "summary": [{k: r[k] for k in ("workload", "precision", "ranks")} | {
        "tiles_ms": round(r["max_over_ranks_ms"]["tiles"]["total"], 3), "rows_ms": round(r["max_over_ranks_ms"]["rows"]["total"], 3)} for r in recs]}))


if __name__ == "__main__":
    main()
