"""Cost of balanced consistency regularisation at the C2 shape, measured in one process on one box:

  python tools/bcr_bench.py [--batch 256] [--out profiles/bcr_bench.txt]

1. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) with diffaug="color,translation,cutout" against the same step
   with bcr=(10, 10) on top - the discriminator's own pass on 4B images in place of 2B - alternating, five rounds of 40 steps, device
   events around each round.
2. the vg_bcr_loss launch alone on [2B, 1] logits, back to back in the stream.
3. the worst fraction of the operator's error bound (tests/bcr_ref.py) over the sizes and logit scales of the tests."""
import argparse
import ctypes as C
import os
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

POLICY = "color,translation,cutout"


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


def worst_fraction(dev):
    import bcr_ref as br
    from second_order_ref import assert_elementwise
    from test_bcr_cpu import SCALES, SIZES, W_FAKE, W_REAL, logits
    L, p = ops._lib.lib(), ops._p
    worst = {"loss": 0.0, "grad": 0.0}
    for B, Kc in SIZES:
        for scale in SCALES:
            lx, la = logits(B, Kc, scale)
            x, a = lx.to(dev), la.to(dev)
            dx, da, out = torch.empty_like(x), torch.empty_like(a), torch.empty(2, device=dev)
            ops._lib.check(L.vg_bcr_loss(p(x), p(a), p(dx), p(da), p(out), B, B, Kc, W_REAL, W_FAKE, 0, 0, 1.0, None), "vg_bcr_loss")
            ref = br.consistency(lx, la, B, W_REAL, W_FAKE)
            worst["loss"] = max(worst["loss"], assert_elementwise(out, ref["loss"], ref["loss_mag"], br.kappa_losses(2 * B, B, Kc), "loss", rel=0.0))
            for got, k in ((dx, "gx"), (da, "ga")):
                worst["grad"] = max(worst["grad"], assert_elementwise(got, ref[k], ref[k + "_mag"], br.kappa_grad(), k, rel=0.0))
    return worst


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

    # ---- 1. engine step
    def make(bcr):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, diffaug=POLICY, bcr=bcr)

    engines = {"diffaug": make((0.0, 0.0)), "bcr": make((10.0, 10.0))}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    res = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a, b = statistics.median(res["diffaug"]), statistics.median(res["bcr"])
    e = engines["bcr"]
    assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all()) and bool(torch.isfinite(e.bcr_losses).all())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  diffaug {POLICY}                   {a:.4f}  (rounds {[round(v, 4) for v in res['diffaug']]})")
    say(f"  the same + bcr=(10, 10), D on 4B = {4 * B}   {b:.4f}  (rounds {[round(v, 4) for v in res['bcr']]})")
    say(f"  difference {b - a:+.4f} ms per step ({100 * (b - a) / a:+.2f} %), 1 launch more; D's own pass runs on {4 * B * 65} token rows "
        f"instead of {2 * B * 65}")
    say(f"  losses after the run {[round(v, 4) for v in e.losses.tolist()]}, consistency (real, fake) {[round(v, 6) for v in e.bcr_losses.tolist()]}")

    # ---- 2. the launch alone
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    x, t = torch.randn(2 * B, 1, device=dev), torch.randn(2 * B, 1, device=dev)
    dx, da, out = torch.zeros_like(x), torch.zeros_like(t), torch.zeros(2, device=dev)
    one = lambda: L.vg_bcr_loss(p(x), p(t), p(dx), p(da), p(out), B, B, 1, C.c_float(10.0), C.c_float(10.0), 1, 0, C.c_float(1.0), st)  # noqa: E731
    timed(one, 50)
    alone = [timed(one, 500) for _ in range(3)]
    say(f"vg_bcr_loss alone, [2B = {2 * B}, 1] logits, back to back in the stream: {statistics.median(alone):.2f} us per launch "
        f"(rounds {[round(v, 2) for v in alone]})")

    # ---- 3. the bound
    w = worst_fraction(dev)
    say(f"worst fraction of the operator bound over B in (1, 7, 256, 1000), Kc in (1, 10), both logit scales: losses {w['loss']:.3f}, "
        f"gradients {w['grad']:.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
