"""Time the fp32 mode of the discriminator (vg_vit_forward_f32 + vg_vit_backward_f32 with weight gradients) at C2 geometry, and of
the generator (vg_gen_forward_f32 + vg_gen_backward_f32) at the reference's default geometry g1 next to its bf16 engine.

    python tools/fp32_bench.py [--batch 256] [--iters 20] [--warmup 3] [--dropout 0.1] [--net d|g|both]

Prints one JSON line per network: ms per forward + backward (device events around `iters` calls), and the GEMM FLOPs of one pass.  For
the TF/s of a single kernel run it under `rocprofv3 --kernel-trace --stats` and divide that kernel's FLOPs by its time.  The generator
line (kept in profiles/gen_fp32_bench.txt) carries no threshold: its fp32 mode is a parity instrument.
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


def _time(step, warmup, iters):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def generator_line(a):
    """forward + backward of the g1 generator (32 row tokens, E 384, 4 blocks, SIREN 768) in both modes, on the same weights"""
    import torch
    from vit_gan_amd import _lib
    from vit_gan_amd.generator import SirenGenerator
    B, lib = a.batch, _lib.lib()
    torch.manual_seed(0)
    mod = SirenGenerator().cuda()  # the reference's defaults and init distributions
    d = mod._dims
    Pm = mod._flat.flat
    Pb, G = Pm.to(torch.bfloat16), torch.zeros_like(Pm)
    net = _lib.VgGenNet(d, Pm.data_ptr(), Pb.data_ptr(), G.data_ptr(), a.dropout, 1234, None, None)
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn(B, 1024, device="cuda", generator=g)
    dimg = torch.randn(B, 3, 32, 32, device="cuda", generator=g)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws32 = torch.empty(lib.vg_gen_ws_bytes_f32(C.byref(d), B), dtype=torch.uint8, device="cuda")
    img32 = torch.empty(B, 3, 32, 32, device="cuda")
    ws16 = torch.empty(lib.vg_gen_ws_bytes(C.byref(d), B), dtype=torch.uint8, device="cuda")
    img16, dimg16 = torch.empty(B, 3, 32, 32, device="cuda", dtype=torch.bfloat16), dimg.to(torch.bfloat16)

    def step32():
        _lib.check(lib.vg_gen_forward_f32(C.byref(net), B, z.data_ptr(), ws32.data_ptr(), img32.data_ptr(), None, st), "vg_gen_forward_f32")
        _lib.check(lib.vg_gen_backward_f32(C.byref(net), B, ws32.data_ptr(), dimg.data_ptr(), None, st), "vg_gen_backward_f32")

    def step16():
        _lib.check(lib.vg_gen_forward(C.byref(net), B, z.data_ptr(), ws16.data_ptr(), img16.data_ptr(), st), "vg_gen_forward")
        _lib.check(lib.vg_gen_backward(C.byref(net), B, ws16.data_ptr(), dimg16.data_ptr(), st), "vg_gen_backward")

    ms16 = _time(step16, a.warmup, a.iters)
    ms32 = _time(step32, a.warmup, a.iters)
    Z, T, E, O, CW, L = d.Z, d.T, d.E, d.O, d.CW, d.L
    per_image = 2 * Z * T * E + L * (2 * T * E * 3 * E + 4 * T * T * E + 4 * T * E * E) + 2 * T * E * O + 2 * T * O * CW  # 243.79 MFLOP
    fl = 3 * B * per_image
    return {"what": "G forward+backward (g1 geometry)", "batch": B, "dropout": a.dropout, "ms_fp32": round(ms32, 3), "ms_bf16": round(ms16, 3),
            "matmul_tflop": round(fl / 1e12, 4), "fp32_tf_per_s_if_all_time": round(fl / (ms32 * 1e-3) / 1e12, 2),
            "fp32_workspace_mib": round(ws32.numel() / 2 ** 20, 1), "image_max_distance": round(float((img32 - img16.float()).abs().max()), 4),
            "finite": bool(torch.isfinite(G).all() and torch.isfinite(img32).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--net", choices=("d", "g", "both"), default="both")
    a = ap.parse_args()
    import torch
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib, flat

    if not torch.cuda.is_available():
        raise SystemExit("fp32_bench needs the GPU")
    if a.net != "d":
        print(json.dumps(generator_line(a)))
    if a.net == "g":
        return
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

    ms = _time(step, a.warmup, a.iters)
    fl, fa = gemm_flops(B, 3, 32, 4, 384, 4, 6, 2, 1)
    print(json.dumps({"what": "fp32 D forward+backward (C2 geometry)", "batch": B, "dropout": a.dropout, "ms": round(ms, 3),
                      "gemm_tflop": round(fl / 1e12, 4), "attention_tflop": round(fa / 1e12, 4),
                      "gemm_tf_per_s_if_all_time": round(fl / (ms * 1e-3) / 1e12, 2), "finite": bool(torch.isfinite(G).all())}))


if __name__ == "__main__":
    main()
