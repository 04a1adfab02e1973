"""Cost of the discriminator's spectral normalisation (csrc/spectral.hip) at the C2 shape, two measurements in one process on one box:

  python tools/spectral_bench.py [--batch 256] [--out profiles/spectral_bench.txt]

1. the two calls alone on the C2 discriminator's flat buffer, set "all": vg_spectral_update (3 launches: W^T u, W v, the scaled cast) and
   vg_spectral_project (2 launches: the partial dots, the rank-one correction).  Device events around 200 repetitions, five alternating
   rounds; us per call and bytes of master per normalised parameter and microsecond.  The 29 MB of normalised weights stay in the
   Infinity Cache between the repetitions, as they do inside a step (AdamW has just written them).
2. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) with spectral_norm="all" against the same step without it -
   launch for launch the step of an engine built without the argument - alternating, five rounds of 40 steps."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_gan_amd  # noqa: E402,F401
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

    def make(which):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, spectral_norm=which)

    engines = {"plain": make(""), "all": make("all")}
    # ---- 1. the two calls alone, on the normalised engine's own buffers and state
    e = engines["all"]
    sp, fd = e.spec, e.vit._flat
    n_norm = sum(N * K for _, N, K in sp.entries)
    grad = torch.randn_like(fd.flat) * 1e-3
    forms = (("vg_spectral_update (3 launches)", lambda: sp.update(fd.flat, fd.shadow, True), 3 * 4 + 2),
             ("vg_spectral_project (2 launches)", lambda: sp.project(grad, fd.flat), 2 * 4 + 2 * 4 + 4),
             ("scaled cast alone (1 launch)", lambda: sp.update(fd.flat, fd.shadow, False), 4 + 2))
    keep = sp.state.clone()
    for _, fn, _ in forms:
        timed(fn, 20)
    res = {name: [] for name, _, _ in forms}
    for _ in range(5):
        for name, fn, _ in forms:
            res[name].append(timed(fn, 200))
    sp.state.copy_(keep)
    fd.refresh_shadow()
    say(f"the C2 discriminator's flat buffer: {fd.total} fp32 parameters, {sp.n} normalised matrices holding {n_norm} of them (set 'all');")
    say("us per call, median of five alternating rounds of 200 calls; B/param = bytes of W, G and shadow the call moves per normalised parameter")
    med = {}
    for name, _, bpp in forms:
        med[name] = statistics.median(res[name])
        say(f"  {name:34s} {bpp:2d} B/param  {med[name]:7.1f} us  {bpp * n_norm / med[name] / 1e6:5.2f} TB/s  (rounds {[round(v, 1) for v in res[name]]})")
    say(f"  round-to-round spread {max(spread(v) for v in res.values()):.1f} us")

    # ---- 2. engine step
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    sres = {k: [] for k in engines}
    for eng in engines.values():
        for _ in range(10):
            eng.step(real)
    for _ in range(5):
        for k, eng in engines.items():
            sres[k].append(timed(lambda: eng.step(real), 40) / 1e3)
    a_, b_ = statistics.median(sres["plain"]), statistics.median(sres["all"])
    spr = 1e3 * max(spread(v) for v in sres.values())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  without the option               {a_:.4f}  (rounds {[round(v, 4) for v in sres['plain']]})")
    say(f"  spectral_norm='all'              {b_:.4f}  (rounds {[round(v, 4) for v in sres['all']]})")
    say(f"  difference {1e3 * (b_ - a_):+.1f} us per step ({100 * (b_ - a_) / a_:+.2f} %), five launches more; the two calls alone "
        f"{med[forms[0][0]] + med[forms[1][0]]:.1f} us; round-to-round spread {spr:.1f} us")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
