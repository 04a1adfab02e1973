"""Cost of class conditioning at the C2 shape, measured in one process on one box:

  python tools/cond_bench.py [--batch 256] [--classes 10] [--out profiles/cond_bench.txt]

1. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) on a discriminator with a K = 10 head, twice - unconditioned
   (n_classes=0: the B K logits are B K samples, today's treatment of such a head) and n_classes=10 (label-selected logit, class
   table in the generator, fake labels drawn on the device) - alternating, five rounds of 40 steps, device events around each round.
2. the three new launches alone at the step's sizes, back to back in the stream: vg_draw_labels, vg_class_add, vg_class_grad."""
import argparse
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
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, B, K, IH = torch.device("cuda:0"), args.batch, args.classes, 32
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}")

    # ---- 1. engine step
    def make(n_classes):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=K, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2, n_classes=n_classes).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, n_classes=n_classes)

    engines = {"plain": make(0), "cond": make(K)}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    y = torch.randint(0, K, (B,), device=dev)
    step = {"plain": lambda: engines["plain"].step(real), "cond": lambda: engines["cond"].step(real, labels=y)}
    res = {k: [] for k in engines}
    for k in engines:
        for _ in range(10):
            step[k]()
    for _ in range(5):
        for k in engines:
            res[k].append(timed(step[k], 40) / 1e3)
    a, b = statistics.median(res["plain"]), statistics.median(res["cond"])
    for e in engines.values():
        assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all())
    spread = max(max(v) - min(v) for v in res.values())
    say(f"engine step, C2 with a K = {K} head (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  n_classes=0 (B K = {B * K} samples per half)      {a:.4f}  (rounds {[round(v, 4) for v in res['plain']]})")
    say(f"  n_classes={K} (label-selected, class table)     {b:.4f}  (rounds {[round(v, 4) for v in res['cond']]})")
    say(f"  difference {(b - a) * 1e3:+.1f} us per step ({100 * (b - a) / a:+.2f} %), 3 launches more (labels, table add, table gradient) and "
        f"{K * 32 * 384} parameters more under AdamW; round-to-round spread {spread * 1e3:.1f} us")
    say(f"  losses after the run: n_classes=0 {[round(v, 4) for v in engines['plain'].losses.tolist()]}, n_classes={K} "
        f"{[round(v, 4) for v in engines['cond'].losses.tolist()]}; fake labels of the last step {engines['cond'].fake_labels[:8].tolist()} ...")

    # ---- 2. the launches alone
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    N = 32 * 384
    lab = torch.empty(B, dtype=torch.int32, device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    w = torch.randn(B, N, device=dev).to(torch.bfloat16)
    table = torch.randn(K, N, device=dev).to(torch.bfloat16)
    dw, dt = torch.randn(B, N, device=dev), torch.zeros(K, N, device=dev)
    jobs = (("vg_draw_labels", lambda: L.vg_draw_labels(p(lab), B, K, 1, 3, p(counter), st), 4 * B),
            ("vg_class_add", lambda: L.vg_class_add(p(w), p(table), p(lab), B, N, K, st), 6 * B * N),
            ("vg_class_grad", lambda: L.vg_class_grad(p(dw), p(lab), p(dt), B, N, K, 1, st), 4 * B * N + 8 * K * N))
    say(f"the new launches alone, B = {B}, N = T E = {N}, K = {K}, back to back in the stream, us per launch (median of three rounds of 500)")
    for name, fn, nbytes in jobs:
        assert fn() == 0
        timed(fn, 50)
        t = [timed(fn, 500) for _ in range(3)]
        say(f"  {name:16s} {statistics.median(t):7.2f} us   {nbytes / statistics.median(t) / 1e6:6.2f} TB/s of the {nbytes / 1e6:.2f} MB it must move "
            f"(rounds {[round(v, 2) for v in t]})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
