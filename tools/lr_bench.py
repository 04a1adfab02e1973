"""Cost of the device-side learning-rate schedule at the C2 shape, measured in one process on one box:

  python tools/lr_bench.py [--batch 256] [--out profiles/lr_bench.txt]

1. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) twice - plain (host-float rates) and with
   lr_schedule="cosine", lr_warmup=100, lr_total=100000, lr_final=0.1 (one vg_lr_schedule launch more, both AdamW launches in their
   _dlr form) - alternating, five rounds of 40 steps, device events around each round.
2. the two new kernels alone, back to back in the stream: vg_lr_schedule, and vg_adamw_step_dlr against vg_adamw_step on a buffer of
   the discriminator's size."""
import argparse
import ctypes as C
import os
import platform
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vit_gan_amd  # noqa: E402,F401
from vit_gan_amd import ops  # noqa: E402
from vit_gan_amd.config import Config  # noqa: E402
from vit_gan_amd.engine import GanEngine  # noqa: E402
from vit_gan_amd.generator import SirenGenerator  # noqa: E402
from vit_gan_amd.modules import ViTDiscriminator  # noqa: E402

SCHEDULE = dict(lr_schedule="cosine", lr_warmup=100, lr_total=100000, lr_final=0.1)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


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

    say(f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}")

    # ---- 1. engine step
    def make(**kw):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, **kw)

    engines = {"plain": make(), "sched": make(**SCHEDULE)}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    res = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a, b = statistics.median(res["plain"]), statistics.median(res["sched"])
    for e in engines.values():
        assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all())
    spread = max(max(v) - min(v) for v in res.values())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  host-float rates (plain)                        {a:.4f}  (rounds {[round(v, 4) for v in res['plain']]})")
    say(f"  cosine, warm-up 100, total 100000, final 0.1    {b:.4f}  (rounds {[round(v, 4) for v in res['sched']]})")
    say(f"  difference {(b - a) * 1e3:+.1f} us per step ({100 * (b - a) / a:+.2f} %), 1 launch more (vg_lr_schedule) and the two AdamW launches "
        f"in their _dlr form; round-to-round spread {spread * 1e3:.1f} us")
    say(f"  rates in force after {engines['sched'].steps} steps: {engines['sched'].lr}; losses plain {[round(v, 4) for v in engines['plain'].losses.tolist()]}, "
        f"scheduled {[round(v, 4) for v in engines['sched'].losses.tolist()]}")

    # ---- 2. the kernels alone
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    counter = torch.full((1,), 500, dtype=torch.int32, device=dev)
    scale, rates = torch.ones(2, device=dev), torch.zeros(2, device=dev)
    sched = (5e-4, "cosine", 100, 100000, 0.1)
    n = engines["plain"].vit._flat.total
    P, G_, M, V = (torch.randn(n, device=dev) * 0.02 for _ in range(4))
    V.abs_()
    SH = torch.empty(n, dtype=torch.bfloat16, device=dev)
    hyp = (0.9, 0.999, 1e-8, 1e-3, 0, p(counter), 1.0)
    sd, sg = C.byref(ops.lr_sched_struct(*sched)), C.byref(ops.lr_sched_struct(*sched))  # (built once: the loop times the launch, not ctypes)
    jobs = (("vg_lr_schedule", lambda: L.vg_lr_schedule(sd, sg, p(counter), p(scale), p(rates), st)),
            ("vg_adamw_step", lambda: L.vg_adamw_step(p(P), p(G_), p(M), p(V), p(SH), n, 5e-4, *hyp, st)),
            ("vg_adamw_step_dlr", lambda: L.vg_adamw_step_dlr(p(P), p(G_), p(M), p(V), p(SH), n, p(rates[0:1]), *hyp, st)))
    say(f"the kernels alone, back to back in the stream, us per launch (median of three rounds of 500); AdamW on the discriminator's {n} parameters")
    for name, fn in jobs:
        assert not fn()
        timed(fn, 50)
        t = [timed(fn, 500) for _ in range(3)]
        say(f"  {name:18s} {statistics.median(t):7.2f} us   (rounds {[round(v, 2) for v in t]})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
