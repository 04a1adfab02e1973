"""Cost of adaptive discriminator augmentation at the C2 shape, measured in one process on one box:

  python tools/ada_bench.py [--batch 256] [--out profiles/ada_bench.txt]

1. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) with diffaug="color,translation,cutout" against the same step
   with ada_target=0.6 on top - the gated kernels at both sites and one vg_ada_update launch - alternating, five rounds of 40 steps,
   device events around each round.
2. the gated launch (vg_diffaug_p_fwd, p = 0.5 and p = 1) against the ungated one (vg_diffaug_fwd) on [2B, 3, 32, 32], alternating, back
   to back in the stream; and the vg_ada_update launch alone on B logits."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
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
    def make(**kw):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, diffaug=POLICY, **kw)

    engines = {"diffaug": make(), "ada": make(ada_target=0.6, ada_interval=4, ada_kimg=100.0)}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    res = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a, b = statistics.median(res["diffaug"]), statistics.median(res["ada"])
    e = engines["ada"]
    assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  diffaug {POLICY}                        {a:.4f}  (rounds {[round(v, 4) for v in res['diffaug']]})")
    say(f"  the same + ada_target=0.6 (gated kernels, controller)   {b:.4f}  (rounds {[round(v, 4) for v in res['ada']]})")
    say(f"  difference {b - a:+.4f} ms per step ({100 * (b - a) / a:+.2f} %), 1 launch more")
    say(f"  after {e.steps} steps: p = {e.ada_p:.6f}, r_t = {e.ada_rt:+.4f}, losses {[round(v, 4) for v in e.losses.tolist()]}")

    # ---- 2. the launches alone
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    x = (torch.rand(2 * B, 3, IH, IH, device=dev) * 2 - 1).to(torch.bfloat16)
    y = torch.empty_like(x)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    calls = {"vg_diffaug_fwd": lambda: L.vg_diffaug_fwd(p(x), p(y), None, 2 * B, 3, IH, 7, 5, 0, p(step), st)}
    for pv in (1.0, 0.5):
        prob = torch.full((1,), pv, dtype=torch.float32, device=dev)
        calls[f"vg_diffaug_p_fwd p={pv:g}"] = lambda prob=prob: L.vg_diffaug_p_fwd(p(x), p(y), None, 2 * B, 3, IH, 7, 5, 0, p(step), p(prob), st)
    alone = {k: [] for k in calls}
    for fn in calls.values():
        timed(fn, 50)
    for _ in range(5):
        for k, fn in calls.items():
            alone[k].append(timed(fn, 500))
    say(f"augmentation launch alone, [2B = {2 * B}, 3, {IH}, {IH}], policy 7, back to back in the stream, us per launch, alternating rounds of 500")
    for k, v in alone.items():
        say(f"  {k:28s} {statistics.median(v):7.2f}  (rounds {[round(t, 2) for t in v]})")
    logits, state = torch.randn(B, device=dev), torch.zeros(4, device=dev)
    one = lambda: L.vg_ada_update(p(logits), B, p(state), C.c_float(0.6), C.c_float(1e-5), 4, p(step), st)  # noqa: E731
    timed(one, 50)
    ctl = [timed(one, 500) for _ in range(3)]
    say(f"vg_ada_update alone, {B} logits, back to back in the stream: {statistics.median(ctl):.2f} us per launch (rounds {[round(v, 2) for v in ctl]})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
