"""Times the 81..256-token paths (csrc/attention_long.hip and the networks built on it) and prints one JSON line per measurement.

  python tools/long_seq_bench.py [--iters N] [--out FILE]

Attention launches are reported against two floors: HBM (bytes in + out at 6.3 TB/s, the achievable copy rate) and MFMA (the
algorithm's products at 2.5 PF/s bf16 dense: 4 B H S^2 HE FLOPs forward, 10 B H S^2 HE backward - the kernels recompute P and dP
in a second orientation, 14 B H S^2 HE issued).  The whole-network rows are plain wall times per call (events around N calls)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_gan_amd  # noqa: E402,F401
from vit_gan_amd import _lib  # noqa: E402

HBM = 6.3e12
MFMA = 2.5e15


def _time(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def attention_rows(iters):
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for (S, H, HE) in ((197, 12, 64), (145, 4, 96)):
        for B in (256, 512):
            E, scale = H * HE, HE ** -0.5
            qkv = (torch.randn(B * S, 3 * E, device="cuda") * 1.5).to(torch.bfloat16)
            o = torch.empty(B * S, E, dtype=torch.bfloat16, device="cuda")
            lse = torch.empty(B, H, S, device="cuda")
            do = torch.randn(B * S, E, device="cuda").to(torch.bfloat16)
            dqkv = torch.empty_like(qkv)

            def fwd():
                _lib.check(lib.vg_attention_fwd(p(qkv), p(o), p(lse), B, H, S, HE, scale, st), "vg_attention_fwd")

            def bwd():
                _lib.check(lib.vg_attention_bwd(p(qkv), p(o), p(do), p(lse), p(dqkv), B, H, S, HE, scale, st), "vg_attention_bwd")
            fwd()
            tf, tb = _time(fwd, iters), _time(bwd, iters)
            fb = B * S * 3 * E * 2 + B * S * E * 2 + B * H * S * 4
            bb = B * S * 3 * E * 2 + 2 * B * S * E * 2 + B * H * S * 4 + B * S * 3 * E * 2
            ff, bf = 4.0 * B * H * S * S * HE, 10.0 * B * H * S * S * HE
            for name, t, by, fl in (("attn_fwd", tf, fb, ff), ("attn_bwd", tb, bb, bf)):
                hf, mf = by / HBM * 1e6, fl / MFMA * 1e6
                rows.append(dict(what=name, B=B, H=H, S=S, HE=HE, us=round(t, 2), hbm_floor_us=round(hf, 2), mfma_floor_us=round(mf, 2),
                                 x_hbm_floor=round(t / hf, 2), x_max_floor=round(t / max(hf, mf), 2)))
    return rows


def network_rows(iters):
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    rows = []
    torch.manual_seed(0)
    B = 64
    D = ViTDiscriminator(Config(image_size=224, patch_size=16, embeddings_dimension=768, attention_heads_count=12,
                                transformer_blocks_count=6, dropout_rate=0.0, classes_count=1)).cuda()
    x = torch.rand(B, 3, 224, 224, device="cuda") * 2 - 1

    def d_fb():
        D(x).sum().backward()
    rows.append(dict(what="D_fwd_bwd_224_16_E768_L6", B=B, S=197, us=round(_time(d_fb, max(2, iters // 10)), 1)))
    del D
    Bs = 128
    Dg = ViTDiscriminator(Config(image_size=48, patch_size=4, embeddings_dimension=384, attention_heads_count=4,
                                 transformer_blocks_count=6, dropout_rate=0.1, classes_count=1, batch_size=Bs))
    G = SirenGenerator(latent=1024, image_size=48, channels=3, embed=384, heads=4, layers=4, siren_hidden=768, dropout=0.2, patch_size=4)
    eng = GanEngine(Dg.cuda(), G.cuda(), batch=Bs, use_graph=True)
    real = torch.rand(Bs, 3, 48, 48, device="cuda") * 2 - 1
    rows.append(dict(what="GanEngine_step_48_4_E384_L6_graph", B=Bs, S=145, T=144, us=round(_time(lambda: eng.step(real), max(2, iters // 5)), 1)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = attention_rows(a.iters) + network_rows(a.iters)
    lines = [json.dumps(dict(r, device=torch.cuda.get_device_name(0))) for r in rows]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
