"""Cost of the generator's weight EMA (csrc/elementwise.hip: vg_adamw_ema_kernel) at the C2 shape, two measurements in one process on one box:

  python tools/ema_bench.py [--batch 256] [--out profiles/ema_bench.txt]

1. optimizer pass on buffers of the C2 generator's size: plain AdamW (vg_adamw_step, 30 B per parameter), the fused form
   (vg_adamw_ema_step, 38 B) and the two-launch form (vg_adamw_step + vg_ema_update, 42 B: the second launch reads the weights again).
   Device events around 200 repetitions, five alternating rounds; the step counter sits past the warm-up, so the average is read and
   blended as in a running step.  The buffers of one form (64 MB x 6) fit the 256 MiB Infinity Cache only in part and the forms take
   turns, so the rates are those of a step that streams other data in between, not of a resident working set.
2. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) with ema_decay=0.999 against the same step without it - launch
   for launch the step of an engine built without the argument - alternating, five rounds of 40 steps."""
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

HYP = (5e-4, 0.9, 0.999, 1e-8, 1e-3)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


def spread(v):
    return max(v) - min(v)


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

    # ---- 1. optimizer pass
    n = SirenGenerator(dropout=0.2)._flat.total  # the C2 generator's flat master
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    step = torch.full((1,), 1000, dtype=torch.int32, device=dev)

    def bufs():
        torch.manual_seed(1)  # the three forms start from the same state: their results are compared below
        P = torch.randn(n, device=dev) * 0.05
        return dict(P=P, G=torch.randn(n, device=dev) * 1e-3, M=torch.zeros(n, device=dev), V=torch.full((n,), 1e-6, device=dev),
                    SH=torch.empty(n, dtype=torch.bfloat16, device=dev), E=P.clone())

    a, f, t = bufs(), bufs(), bufs()

    def plain():
        L.vg_adamw_step(p(a["P"]), p(a["G"]), p(a["M"]), p(a["V"]), p(a["SH"]), n, *HYP, 0, p(step), 1.0, st)

    def fused():
        L.vg_adamw_ema_step(p(f["P"]), p(f["G"]), p(f["M"]), p(f["V"]), p(f["SH"]), p(f["E"]), n, *HYP, 0, p(step), 1.0, 0.999, 0, st)

    def two():
        L.vg_adamw_step(p(t["P"]), p(t["G"]), p(t["M"]), p(t["V"]), p(t["SH"]), n, *HYP, 0, p(step), 1.0, st)
        L.vg_ema_update(p(t["E"]), p(t["P"]), n, 0.999, 0, 0, p(step), st)

    forms = (("vg_adamw_step (no average)", plain, 30), ("vg_adamw_ema_step (fused)", fused, 38), ("vg_adamw_step + vg_ema_update", two, 42))
    for _, fn, _ in forms:
        timed(fn, 20)
    res = {name: [] for name, _, _ in forms}
    for _ in range(5):
        for name, fn, _ in forms:
            res[name].append(timed(fn, 200))
    torch.cuda.synchronize()
    assert torch.equal(f["P"], t["P"]) and torch.equal(f["E"], t["E"]) and torch.equal(f["P"], a["P"]), "the three forms diverged"
    say(f"optimizer pass over the C2 generator's flat master, n = {n} fp32 parameters, device counter past the warm-up; us per pass,")
    say("median of five alternating rounds of 200 passes; bytes = the traffic the form needs (B per parameter x n)")
    med = {}
    for name, _, bpp in forms:
        med[name] = statistics.median(res[name])
        say(f"  {name:32s} {bpp} B/param  {med[name]:8.1f} us  {bpp * n / med[name] / 1e6:6.2f} TB/s  (rounds {[round(v, 1) for v in res[name]]})")
    k_plain, k_fused, k_two = (med[name] for name, _, _ in forms)
    say(f"  fused - plain AdamW {k_fused - k_plain:+.1f} us;  two launches - fused {k_two - k_fused:+.1f} us;  round-to-round spread "
        f"{max(spread(v) for v in res.values()):.1f} us")

    # ---- 2. engine step
    def make(ema_decay):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, ema_decay=ema_decay)

    engines = {"plain": make(0.0), "ema": make(0.999)}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    sres = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            sres[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a_, b_ = statistics.median(sres["plain"]), statistics.median(sres["ema"])
    sp = 1e3 * max(spread(v) for v in sres.values())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  without the average              {a_:.4f}  (rounds {[round(v, 4) for v in sres['plain']]})")
    say(f"  ema_decay=0.999                  {b_:.4f}  (rounds {[round(v, 4) for v in sres['ema']]})")
    say(f"  difference {1e3 * (b_ - a_):+.1f} us per step ({100 * (b_ - a_) / a_:+.2f} %), no launch more; the kernel's own increment above "
        f"{k_fused - k_plain:+.1f} us; round-to-round spread {sp:.1f} us")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
