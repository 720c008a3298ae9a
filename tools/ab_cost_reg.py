"""Bitwise A/B of two builds of the library on the cost-regularisation U-Nets: volume, prob and the whole workspace.
usage: ab_cost_reg.py dump <lib.so> <out.npz>   |   ab_cost_reg.py cmp <a.npz> <b.npz>"""
import sys, os, ctypes as C, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
if sys.argv[1] == "cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    ok = sorted(a.files) == sorted(b.files)
    for k in a.files:
        same = k in b.files and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
        ok &= same
        print(k, a[k].shape, "bit-identical" if same else "DIFFERENT")
    sys.exit(0 if ok else 1)
import torch
from gdb_nerf_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[2])
from gdb_nerf_amd import costvol
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d
out = {}
# (depth, cin, c, cout, B, D, H, W): the two c2 stage shapes, and base_channels 24 / 16 for the kernels those do not launch
cases = [(2, 32, 8, 8, 1, 64, 64, 80), (3, 16, 8, 8, 1, 8, 256, 320), (2, 24, 24, 15, 2, 8, 8, 36), (3, 40, 16, 4, 1, 8, 16, 72)]
lib = _lib.load()
for i, (depth, cin, c, cout, B, D, H, W) in enumerate(cases):
    torch.manual_seed(70 + i)
    m = _UNet3d(cin, cout, c, depth).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.weight.uniform_(0.5, 1.5); mod.bias.uniform_(-0.2, 0.2); mod.running_mean.uniform_(-0.1, 0.1); mod.running_var.uniform_(0.8, 1.2)
    cost = (torch.rand(B, cin, D, H, W) * 2.0 - 0.5).cuda()
    packed = costvol.CostReg(m).pack(cost.device)
    n = C.c_size_t()
    _lib.check(lib.gdb_cost_reg_workspace_bytes(depth, cin, c, cout, B, D, H, W, C.byref(n)))
    ws = torch.zeros(n.value // 4, device="cuda")
    vol, prob = torch.zeros(B, cout, D, H, W, device="cuda"), torch.zeros(B, D, H, W, device="cuda")
    _lib.check(lib.gdb_cost_reg(depth, cin, c, cout, cost.data_ptr(), B, D, H, W, packed.data_ptr(), ws.data_ptr(), n.value, vol.data_ptr(),
                                prob.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out[f"case{i}_volume"], out[f"case{i}_prob"], out[f"case{i}_workspace"] = vol.cpu().numpy(), prob.cpu().numpy(), ws.cpu().numpy()
np.savez(sys.argv[3], **out)
print("dumped", sys.argv[3])
