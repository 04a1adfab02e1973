"""Cost of the R1 penalty and of lazy regularisation at the C2 shape, measured in one process on one box:

  python tools/r1_bench.py [--batch 256] [--out profiles/r1_bench.txt] [--commit ID]

bench.py's C2 step (hipGraph replay, train-mode dropout), ms per step, for four engines: plain, gp_weight=10 (the WGAN-GP call, same
loss otherwise), r1_gamma=10 at interval 1, and r1_gamma=10 at interval 16 - alternating, five rounds of 48 steps (a multiple of 16:
every round of the lazy engine holds exactly 3 penalty steps), device events around each round.  No threshold; what the numbers are
read against: interval 1 should be no slower than the GP step (the same passes minus the interpolation launch), interval 16 should
average about plain + (R1 - plain) / 16."""
import argparse
import os
import platform
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import vit_gan_amd  # noqa: E402,F401
from vit_gan_amd.config import Config  # noqa: E402
from vit_gan_amd.engine import GanEngine  # noqa: E402
from vit_gan_amd.generator import SirenGenerator  # noqa: E402
from vit_gan_amd.modules import ViTDiscriminator  # noqa: E402

ROUND = 48


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms per repetition


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit measured, where the tree is not a git checkout")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, B = torch.device("cuda:0"), args.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def make(**kw):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, **kw)

    engines = {"plain": make(), "gp_weight=10": make(gp_weight=10.0), "r1_gamma=10, interval 1": make(r1_gamma=10.0),
               "r1_gamma=10, interval 16": make(r1_gamma=10.0, r1_interval=16)}
    real = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    for e in engines.values():  # both kinds of step of the lazy engine captured and replayed, and the schedule back at a due step
        for _ in range(ROUND):
            e.step(real)
    res = {k: [] for k in engines}
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), ROUND))
    for k, e in engines.items():
        assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all()), k
    med = {k: statistics.median(v) for k, v in res.items()}
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown (not a git checkout)"
    say(f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}; commit {commit}")
    say(f"engine step, C2 (B = {B}, loss ns, hipGraph replay, train-mode dropout), ms per step, alternating rounds of {ROUND} steps, median of 5")
    for k in engines:
        say(f"  {k:28s} {med[k]:8.4f}  (rounds {[round(v, 4) for v in res[k]]})")
    plain, gp, r1, lazy = (med[k] for k in engines)
    say(f"  R1 at interval 1 against the GP step: {r1 - gp:+.4f} ms ({100 * (r1 - gp) / gp:+.2f} %); expectation: not slower (one launch fewer)")
    say(f"  R1 at interval 16: {lazy:.4f} ms; plain + (R1 - plain) / 16 = {plain + (r1 - plain) / 16:.4f} ms")
    e = engines["r1_gamma=10, interval 16"]
    say(f"  after {e.steps} steps of the lazy engine: r1_loss {float(e.r1_loss):.6f}, losses {[round(v, 4) for v in e.losses.tolist()]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
