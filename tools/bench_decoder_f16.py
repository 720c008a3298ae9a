"""The decoder's three forms - fp32 MFMA, split-f16 and plain f16 (gdb_decode_f16) - on the c2 bundle map (256x320, 3 blocks, output
512x640), alternating in one process: 9 rounds of 40 decodes per side, each round ending in one device synchronise; median with
min .. max per side.  `--once SIDE` runs a few decodes of one side only (for a kernel trace or a counter pass of its own).

    python tools/bench_decoder_f16.py [--out profiles/r11/bench_decoder_f16.json] [--once f16|f32x|f32]"""
import json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import gdb_nerf_amd  # noqa
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import HotPathEngine
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder
H, W, ROUNDS, N = 256, 320, 9, 40
argv = sys.argv[1:]
torch.manual_seed(0)
dec = Decoder(27, 3, num_feats=64, num_layers=3, upscale_factor=2).cuda().eval()
frame = synthetic.make_frame(2 * H, 2 * W, V=2, seed=1)
eng = HotPathEngine(); eng.reuse_outputs = True
eng.prepare({k: torch.from_numpy(v).cuda() for k, v in frame.items()})
eng.load_decoder_weights({k: v.detach() for k, v in dec.state_dict().items()}, 3)
x = torch.randn(1, 27, H, W, device="cuda")
bf = torch.zeros((H * W, 41), device="cuda"); bf[:, 12:39] = x.permute(0, 2, 3, 1).reshape(H * W, 27)
sides = {"f32": lambda: eng.decode(bf, precision=1), "f32x": lambda: eng.decode(bf, precision=2), "f16": lambda: eng.decode_f16(bf)}
if "--once" in argv:
    fn = sides[argv[argv.index("--once") + 1]]
    for _ in range(5): fn()
    torch.cuda.synchronize(); sys.exit(0)
for fn in sides.values():
    for _ in range(10): fn()
torch.cuda.synchronize()
ms = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(N): fn()
        torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / N * 1e3)
with torch.no_grad():
    want = dec(x)
res = {"shape": [1, H, W], "blocks": 3, "rounds": ROUNDS, "decodes_per_round": N,
       "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
       "max_abs_err_vs_torch_fp32": {k: float((fn() - want).abs().max()) for k, fn in sides.items()}, "output_scale": float(want.abs().max())}
spread = max(res["ms"][k]["max"] - res["ms"][k]["min"] for k in ("f32x", "f16"))
res["f16_below_split_f16_by_ms"] = res["ms"]["f32x"]["median"] - res["ms"]["f16"]["median"]
res["wider_spread_ms"] = spread
res["done"] = res["f16_below_split_f16_by_ms"] > spread
print(json.dumps(res))
if "--out" in argv:
    out = argv[argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
