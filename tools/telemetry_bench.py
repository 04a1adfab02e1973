"""Cost of the step's telemetry at the C2 shape, measured in one process on one box:

  python tools/telemetry_bench.py [--batch 256] [--out profiles/telemetry_bench.txt]

1. engine step: bench.py's C2 step (hipGraph replay, train-mode dropout) twice - plain and with telemetry=64 (seven launches more:
   two vg_logit_stats, two vg_grad_stats of two launches each, vg_telemetry_commit) - alternating, five rounds of 40 steps, device
   events around each round.
2. vg_grad_stats alone on the C2 gradient buffers, back to back in the stream, against torch.linalg.vector_norm over the same flat
   buffer - a comparator that does strictly less (no segments, no counts, and it reads the padding too) - with the bytes per second
   each achieves (bytes = 4 per gradient element read: the slots' elements for vg_grad_stats, the whole buffer for vector_norm).  Two
   legs: "warm" reads ONE buffer again and again - 29 / 64 MB stay resident in the 256 MB last-level cache, so that rate is a cache
   rate, not an HBM rate - and "rotating" walks copies of the buffer that total more than 512 MB, so every call reads memory the cache
   no longer holds (closer to the step, where the gradient was written by the backward kernels long before).  Each timed round runs
   for about half a second."""
import argparse
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

    say(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")

    # ---- 1. engine step
    def make(**kw):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, **kw)

    engines = {"plain": make(), "telemetry": make(telemetry=64)}
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    res = {k: [] for k in engines}
    for e in engines.values():
        for _ in range(10):
            e.step(real)
    for _ in range(5):
        for k, e in engines.items():
            res[k].append(timed(lambda: e.step(real), 40) / 1e3)
    a, b = statistics.median(res["plain"]), statistics.median(res["telemetry"])
    for e in engines.values():
        assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all())
    spread = max(max(v) - min(v) for v in res.values())
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, alternating rounds of 40 steps")
    say(f"  plain                 {a:.4f}  (rounds {[round(v, 4) for v in res['plain']]})")
    say(f"  telemetry=64          {b:.4f}  (rounds {[round(v, 4) for v in res['telemetry']]})")
    say(f"  difference {(b - a) * 1e3:+.1f} us per step ({100 * (b - a) / a:+.2f} %), seven launches more; round-to-round spread {spread * 1e3:.1f} us")
    same = all(torch.equal(x, y) for x, y in zip((engines["plain"].vit._flat.flat, engines["plain"].gen._flat.flat),
                                                 (engines["telemetry"].vit._flat.flat, engines["telemetry"].gen._flat.flat)))
    rec = engines["telemetry"].history()
    say(f"  weights of the two engines after {engines['plain'].steps} steps bit-equal: {same}; records read: {len(rec['step'])} (dropped {rec['dropped']}), "
        f"last gnorm_d_sum {rec['gnorm_d_sum'][-1]:.4f}, gnorm_g_sum {rec['gnorm_g_sum'][-1]:.4f}, nonfinite {rec['nonfinite_d'][-1]:.0f} / {rec['nonfinite_g'][-1]:.0f}")

    # ---- 2. the kernel alone against torch's whole-buffer norm
    st = ops._st()
    say("vg_grad_stats alone (two launches), back to back in the stream, against torch.linalg.vector_norm over the same flat buffer, us per call "
        "(median of three rounds of about 0.5 s each); warm = one buffer, cache-resident; rotating = copies totalling > 512 MB, read in turn")
    for name, fp in (("D", engines["plain"].vit._flat), ("G", engines["plain"].gen._flat)):
        g = torch.randn(fp.total, device=dev) * 1e-3
        copies = [g] + [g.clone() for _ in range((512 << 20) // (4 * fp.total) + 1)]
        plan = ops.GradStatsPlan(fp.slots, fp.total, dev)
        covered = int(plan.chunks[:, 1].sum())
        out = torch.empty((), device=dev)
        say(f"  {name}: {fp.total} elements, {plan.n_seg} tensors, {plan.n_chunks} chunks, {len(copies)} copies in the rotating leg")
        for leg, bufs in (("warm", copies[:1]), ("rotating", copies)):
            turn = [0]

            def nxt(bufs=bufs, turn=turn):
                turn[0] = (turn[0] + 1) % len(bufs)
                return bufs[turn[0]]
            jobs = (("vg_grad_stats", lambda: plan.enqueue(nxt(), 1.0, st), 4 * covered),
                    ("torch vector_norm", lambda: torch.linalg.vector_norm(nxt(), out=out), 4 * fp.total))
            for what, fn, nbytes in jobs:
                fn()
                reps = max(200, int(0.5e6 / timed(fn, 50)))
                t = [timed(fn, reps) for _ in range(3)]
                m = statistics.median(t)
                say(f"    {leg:8s} {what:18s} {m:8.2f} us  {nbytes / m / 1e6:7.2f} TB/s  ({reps} calls a round; rounds {[round(v, 2) for v in t]})")
        torch.cuda.synchronize()
        say(f"    l2 {float(plan.totals[1]):.6f} against vector_norm {float(out):.6f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
