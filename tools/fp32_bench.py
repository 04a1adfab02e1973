"""Time the fp32 mode of the discriminator (vg_vit_forward_f32 + vg_vit_backward_f32 with weight gradients) at C2 geometry.

    python tools/fp32_bench.py [--batch 256] [--iters 20] [--warmup 3] [--dropout 0.1]

Prints one JSON line: ms per forward + backward (device events around `iters` calls), and the GEMM FLOPs of one pass.  For the
TF/s of a single kernel run it under `rocprofv3 --kernel-trace --stats` and divide that kernel's FLOPs by its time.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gemm_flops(B, C_, IH, P, E, H, L, R, Kc):
    NP = (IH // P) ** 2
    S, M = NP + 1, B * (NP + 1)
    per_block = 2 * M * E * (3 * E + E + 2 * R * E)      # qkv, out-projection, fc1, fc2
    fwd = L * per_block + 2 * B * NP * C_ * P * P * E + 2 * B * E * (E + Kc)
    attn = L * B * H * 2 * 2 * S * S * (E // H)         # scores and P.V
    return 3 * fwd, 3 * attn                            # forward + input gradient + weight gradient


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib, flat

    if not torch.cuda.is_available():
        raise SystemExit("fp32_bench needs the GPU")
    d = flat.vit_dims_struct(3, 32, 4, 384, 4, 6, 2, 1)
    lay = flat.vit_layout(d)
    g = torch.Generator(device="cuda").manual_seed(0)
    Pm = torch.randn(lay.total, device="cuda", generator=g) * 0.02
    G = torch.zeros_like(Pm)
    net = _lib.VgVitNet(d, Pm.data_ptr(), None, G.data_ptr(), a.dropout, 1234, None, None, 0, 0)
    B = a.batch
    lib = _lib.lib()
    ws = torch.empty(lib.vg_vit_ws_bytes_f32(C.byref(d), B), dtype=torch.uint8, device="cuda")
    x = torch.rand(B, 3, 32, 32, device="cuda", generator=g) * 2 - 1
    dl = torch.randn(B, 1, device="cuda", generator=g)
    logits = torch.empty(B, 1, device="cuda")
    dimg = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step():
        _lib.check(lib.vg_vit_forward_f32(C.byref(net), B, x.data_ptr(), ws.data_ptr(), logits.data_ptr(), st), "forward_f32")
        _lib.check(lib.vg_vit_backward_f32(C.byref(net), B, ws.data_ptr(), dl.data_ptr(), dimg.data_ptr(), 1, st), "backward_f32")

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    fl, fa = gemm_flops(B, 3, 32, 4, 384, 4, 6, 2, 1)
    print(json.dumps({"what": "fp32 D forward+backward (C2 geometry)", "batch": B, "dropout": a.dropout, "ms": round(ms, 3),
                      "gemm_tflop": round(fl / 1e12, 4), "attention_tflop": round(fa / 1e12, 4),
                      "gemm_tf_per_s_if_all_time": round(fl / (ms * 1e-3) / 1e12, 2), "finite": bool(torch.isfinite(G).all())}))


if __name__ == "__main__":
    main()
