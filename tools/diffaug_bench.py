"""Cost of the differentiable augmentation (csrc/augment.hip) at the C2 shape, two measurements in one process on one box:

  python tools/diffaug_bench.py [--batch 256] [--out profiles/diffaug_bench.txt]

1. single application: the three launches of an augmented step (T_1 on [2B, 3, 32, 32], T_2 and its adjoint on [B, 3, 32, 32]) against
   the same augmentation written with torch ops on the same bf16 buffers - what a caller could do without the kernels.  Device events
   around 200 repetitions, five alternating rounds; launches of the torch form counted with the profiler (one repetition).
2. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) with diffaug="color,translation,cutout" against the same step
   without it - launch for launch the step of an engine built without the argument - alternating, five rounds of 40 steps."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_gan_amd  # noqa: E402,F401
from vit_gan_amd import ops  # noqa: E402
from vit_gan_amd.config import Config  # noqa: E402
from vit_gan_amd.engine import GanEngine  # noqa: E402
from vit_gan_amd.generator import SirenGenerator  # noqa: E402
from vit_gan_amd.modules import ViTDiscriminator  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


def torch_params(n, IH, dev):
    """per-image parameters drawn with torch's generator: four launches, counted with the augmentation they belong to"""
    u = torch.rand(n, 3, device=dev)
    r = IH // 8
    t = torch.randint(-r, r + 1, (n, 2), device=dev)
    c = torch.randint(0, IH + 1, (n, 2), device=dev)
    return u[:, 0] - 0.5, 2 * u[:, 1], u[:, 2] + 0.5, t[:, 0], t[:, 1], c[:, 0], c[:, 1]


def torch_augment(x, IH, ar):
    """T on bf16 [n, 3, IH, IH] with torch ops, fp32 arithmetic, bf16 out"""
    n = x.shape[0]
    b, s, k, tx, ty, cx, cy = torch_params(n, IH, x.device)
    v = x.float() + b.view(-1, 1, 1, 1)
    m = v.mean(1, keepdim=True)
    v = m + s.view(-1, 1, 1, 1) * (v - m)
    M = v.mean((1, 2, 3), keepdim=True)
    v = M + k.view(-1, 1, 1, 1) * (v - M)
    si, sj = ar[None, :] - ty[:, None], ar[None, :] - tx[:, None]
    ok = ((si >= 0) & (si < IH))[:, :, None] & ((sj >= 0) & (sj < IH))[:, None, :]
    v = v[torch.arange(n, device=x.device)[:, None, None], :, si.clamp(0, IH - 1)[:, :, None], sj.clamp(0, IH - 1)[:, None, :]].permute(0, 3, 1, 2)
    r0, c0 = cy - IH // 4, cx - IH // 4
    cut = (((ar[None, :] >= r0[:, None]) & (ar[None, :] < (r0 + IH // 2)[:, None]))[:, :, None]
           & ((ar[None, :] >= c0[:, None]) & (ar[None, :] < (c0 + IH // 2)[:, None]))[:, None, :])
    return (v * (ok & ~cut)[:, None]).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, B, IH = torch.device("cuda:0"), args.batch, 32
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- 1. single application
    pair = (torch.rand(2 * B, 3, IH, IH, device=dev) * 2 - 1).to(torch.bfloat16)
    fake, dlog = pair[B:], (torch.randn(B, 3, IH, IH, device=dev) * 1e-3).to(torch.bfloat16)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    ar = torch.arange(IH, device=dev)
    L = ops._lib.lib()
    o2, o1, o0 = torch.empty_like(pair), torch.empty_like(fake), torch.empty_like(fake)
    p = ops._p
    st = ops._st()

    def hip_three():
        L.vg_diffaug_fwd(p(pair), p(o2), None, 2 * B, 3, IH, 7, 1, 0, p(step), st)
        L.vg_diffaug_fwd(p(fake), p(o1), None, B, 3, IH, 7, 1, 1, p(step), st)
        L.vg_diffaug_bwd(p(dlog), p(o0), 0, B, 3, IH, 7, 1, 1, p(step), st)

    def torch_three():  # the adjoint through autograd, as a caller without the kernels would have it
        torch_augment(pair, IH, ar)
        f = fake.detach().requires_grad_(True)
        torch_augment(f, IH, ar).backward(dlog)

    for fn in (hip_three, torch_three):
        timed(fn, 20)
    hip_t, tor_t = [], []
    for _ in range(5):
        hip_t.append(timed(hip_three, 200))
        tor_t.append(timed(torch_three, 200))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_three()
            torch.cuda.synchronize()
        n_torch = sum(e.count for e in prof.key_averages() if e.device_type is not None and "cuda" in str(e.device_type).lower())
    except Exception as exc:  # the count is an extra; the times above do not depend on it
        n_torch = f"not counted ({type(exc).__name__})"
    say(f"single application, 2B = {2 * B} images 3x{IH}x{IH} bf16: T_1([real; fake]) + T_2(fake) + T_2^T(dy)")
    say(f"  HIP kernels   3 launches   {statistics.median(hip_t):8.1f} us  (rounds {[round(v, 1) for v in hip_t]})")
    say(f"  torch ops     {n_torch} launches   {statistics.median(tor_t):8.1f} us  (rounds {[round(v, 1) for v in tor_t]})")
    one = [timed(lambda: L.vg_diffaug_fwd(p(pair), p(o2), None, 2 * B, 3, IH, 7, 1, 0, p(step), st), 500) for _ in range(3)]
    say(f"  T_1 alone, back to back in the stream: {statistics.median(one):.2f} us per launch "
        f"({2 * pair.numel() * 2 / statistics.median(one) / 1e6:.2f} TB/s of in + out bytes)")

    # ---- 2. engine step
    def make(diffaug):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, diffaug=diffaug)

    engines = {"plain": make(""), "diffaug": make("color,translation,cutout")}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    res = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a, b = statistics.median(res["plain"]), statistics.median(res["diffaug"])
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  without diffaug                  {a:.4f}  (rounds {[round(v, 4) for v in res['plain']]})")
    say(f"  color,translation,cutout         {b:.4f}  (rounds {[round(v, 4) for v in res['diffaug']]})")
    say(f"  difference {1e3 * (b - a):+.1f} us per step ({100 * (b - a) / a:+.2f} %), 3 launches more")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
