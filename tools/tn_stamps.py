#!/usr/bin/env python3
"""Cycle breakdown of a stage of the 128x384 weight-gradient kernel from in-kernel s_memtime stamps.
Needs the diagnostic build:  make -C vit-gan_amd/csrc var SRC=gemm_tn NAME=tnst DEFS=-DVG_TN_STAMPS  (the product carries none)."""
import ctypes as C
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vit_gan_amd  # noqa: F401,E402
from vit_gan_amd import _lib  # noqa: E402

M, N, K, SPL = 33280, int(os.environ.get("N", "1152")), 384, int(os.environ.get("WG_SPLITS", "10"))
nwg = (N // 128) * (K // 384) * SPL
stamps = torch.zeros(nwg * 8 * 8, dtype=torch.int64, device="cuda")
os.environ["VG_STAMP_PTR"] = hex(stamps.data_ptr())
L = _lib.bind(C.CDLL(os.path.join(root, "vit-gan_amd", "libvitgan_hip_tnst.so")), ["vg_linear_wgrad"])
P = _lib.ptr
BF = torch.bfloat16
dy = torch.randn(M, N, device="cuda").to(BF); x = torch.randn(M, K, device="cuda").to(BF)
dw = torch.empty(N, K, device="cuda"); slab = torch.empty(SPL * N * K, device="cuda")
st = _lib.stream()
for _ in range(5):
    L.vg_linear_wgrad(P(dy), P(x), P(dw), P(slab), slab.numel(), M, N, K, SPL, 0, st)
torch.cuda.synchronize()
t = stamps.cpu().numpy().reshape(nwg, 8, 8).astype(np.float64)
steps = t[:, :, 5]
per = t[:, :, :5] / steps[:, :, None]
print(f"N {N}: {nwg} workgroups, {int(steps[0,0])} stages each; cycles per stage (mean over waves): "
      f"vmcnt+barrier {per[:,:,0].mean():.0f} | before MFMA {per[:,:,1].mean():.0f} | MFMA {per[:,:,2].mean():.0f} | "
      f"MFMA {per[:,:,3].mean():.0f} | total {per[:,:,4].mean():.0f}")
for w in range(8):
    print(f"  wave {w}: " + " ".join(f"{per[:, w, i].mean():7.0f}" for i in range(5)))
