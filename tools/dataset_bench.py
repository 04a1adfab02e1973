"""Cost of fetching the real batch on the device, at the C2 shape, measured in one process on one box:

  python tools/dataset_bench.py [--batch 256] [--out profiles/dataset_bench.txt]

The C2 step (bench.py's: hipGraph replay, train-mode dropout) on a CIFAR-10-sized set of random bytes (50 000 x 3 x 32 x 32 uint8; the
pixel values cannot matter to the time).  Legs, alternating in rounds of 40 steps, each warmed and ending in a synchronise:
  (a)  host-fed: ``step(real)`` on ONE device-resident fp32 batch - what bench.py times
  (a') leg (a) again in a slot of its own: the difference of the two medians is the spread the verdict allows
  (b)  an engine with the dataset, ``step()``
  (c)  the same engine, ``run(40)``
  (d)  for information: a host pipeline feeding leg (a)'s engine - gather, ToTensor and Normalize of uint8 on the CPU (torch, the
       process's threads), then the copy of each batch from pageable and from pinned memory
and the fetch kernel alone, back to back in the stream."""
import argparse
import os
import platform
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import vit_gan_amd  # noqa: E402,F401
from vit_gan_amd import ops  # noqa: E402
from vit_gan_amd.config import Config  # noqa: E402
from vit_gan_amd.data import DeviceDataset  # noqa: E402
from vit_gan_amd.engine import GanEngine  # noqa: E402
from vit_gan_amd.generator import SirenGenerator  # noqa: E402
from vit_gan_amd.modules import ViTDiscriminator  # noqa: E402

ROUNDS, STEPS = 7, 40


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


def wall(fn, reps):
    """host pipelines are timed on the wall clock: their cost is host time the device waits for"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, B, IH, N = torch.device("cuda:0"), args.batch, 32, 50000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}, {torch.get_num_threads()} host threads")

    def make(**kw):
        torch.manual_seed(0)
        cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, mlp_ratio=2, patch_size=4, image_size=32,
                     input_channels=3, classes_count=1, dropout_rate=0.1, batch_size=B)
        D = ViTDiscriminator(cfg).to(dev).train()
        G = SirenGenerator(dropout=0.2).to(dev).train()
        return GanEngine(D, G, batch=B, use_graph=True, seed=1000, **kw)

    host_images = torch.randint(0, 256, (N, 3, IH, IH), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    ds = DeviceDataset(host_images, layout="nchw", flip=True)
    fed, own = make(), make(dataset=ds)
    real = torch.rand(B, 3, IH, IH, device=dev) * 2 - 1
    legs = {"a": lambda: timed(lambda: fed.step(real), STEPS), "b": lambda: timed(own.step, STEPS), "c": lambda: timed(lambda: own.run(STEPS), 1) / STEPS,
            "a'": lambda: timed(lambda: fed.step(real), STEPS)}
    for _ in range(10):
        fed.step(real)
        own.step()
    own.run(10)
    res = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            res[k].append(leg() / 1e3)
    for e in (fed, own):
        assert e.graph_active and e.graph_fallback_reason is None and bool(torch.isfinite(e.losses).all())
    med = {k: statistics.median(v) for k, v in res.items()}
    allowed = abs(med["a"] - med["a'"])
    say(f"engine step, C2 (B = {B}, hipGraph replay, train-mode dropout), ms per step, {ROUNDS} alternating rounds of {STEPS} steps; dataset {N} x 3 x {IH} x {IH} "
        f"uint8, shuffle and flip on, {own.steps_per_epoch} steps per epoch")
    names = {"a": "(a)  host-fed, one resident fp32 batch", "a'": "(a') the same again", "b": "(b)  dataset, step()", "c": f"(c)  dataset, run({STEPS})"}
    for k in ("a", "a'", "b", "c"):
        say(f"  {names[k]:40s} {med[k]:.4f}  ({B / med[k]:.1f} k img/s)  (rounds {[round(v, 4) for v in res[k]]})")
    say(f"  |(a) - (a')| = {allowed * 1e3:.1f} us;  (b) - (a) = {(med['b'] - med['a']) * 1e3:+.1f} us;  (c) - (a) = {(med['c'] - med['a']) * 1e3:+.1f} us;  "
        f"round-to-round spread of (a): {(max(res['a']) - min(res['a'])) * 1e3:.1f} us")
    ok = med["b"] - med["a"] <= allowed and med["c"] - med["a"] <= allowed
    say(f"  requirement ((b) and (c) no slower than (a) by more than |(a) - (a')|): {'met' if ok else 'NOT met'}")
    say(f"  the dataset engine is at epoch {own.epoch} after {own.steps} steps; losses host-fed {[round(v, 4) for v in fed.losses.tolist()]}, "
        f"dataset {[round(v, 4) for v in own.losses.tolist()]}")

    # ---- (d) a host pipeline in front of the host-fed engine: decode on the CPU, copy each batch
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2))
    pinned = torch.empty(B, 3, IH, IH, dtype=torch.float32).pin_memory()
    at = [0]

    def host_batch():
        i = at[0] = (at[0] + B) % (N - B)
        x = host_images[perm[i:i + B]].float().div_(255).sub_(0.5).div_(0.5)
        return x

    def pageable():
        fed.step(host_batch().to(dev))

    def from_pinned():
        pinned.copy_(host_batch())
        fed.step(pinned.to(dev, non_blocking=True))

    say("(d) host pipeline (CPU gather + ToTensor + Normalize in this process, then the copy) feeding the host-fed engine, ms per step on the wall "
        "clock, 3 rounds of 40 steps - for information")
    for name, fn in (("decode only (no copy, no step)", host_batch), ("pageable copy + step", pageable), ("pinned copy + step", from_pinned)):
        wall(fn, 5)
        t = [wall(fn, STEPS) / 1e3 for _ in range(3)]
        say(f"  {name:40s} {statistics.median(t):.4f}  (rounds {[round(v, 4) for v in t]})")

    # ---- the fetch alone
    L, p, st = ops._lib.lib(), ops._p, ops._st()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    imgs = torch.empty(B, 3, IH, IH, dtype=torch.bfloat16, device=dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    fetch = lambda: L.vg_dataset_fetch(p(ds.images), None, N, 3, IH, 0, p(ds.lut_bf16), p(imgs), None, p(idx), B, 0, 1, 3, 7, p(counter), st)  # noqa: E731
    assert not fetch()
    timed(fetch, 50)
    t = [timed(fetch, 500) for _ in range(3)]
    say(f"vg_dataset_fetch alone, back to back in the stream (B = {B}: {B * 3 * IH * IH / 1e6:.2f} MB in, {2 * B * 3 * IH * IH / 1e6:.2f} MB out), us per launch: "
        f"{statistics.median(t):.2f}  (rounds {[round(v, 2) for v in t]})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
