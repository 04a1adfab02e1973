"""Cost of one Frechet-distance evaluation at the C2 geometry, measured in one process on one box:

  python tools/fid_bench.py [--n-fake 10000] [--batch 256] [--out profiles/fid_bench.txt]

The evaluator ``train_model(fid="random-vit")`` builds (a frozen random ViT of C2's geometry: 32 x 32 x 3, 4 x 4 patches, E = 384,
6 blocks) on the default SLN/SIREN generator, real statistics from a 2 048-image set of random bytes (fitted once, not timed).  Legs,
alternating in rounds, each warmed and timed on the wall clock around a synchronise (an evaluation ends on the host: the moments are
copied back for the eigendecompositions):
  (a)  one whole evaluation: generator forward, quantisation, feature forward and vg_moments_update per batch, then
       vg_moments_finish, the copy and ``frechet_distance`` on the host
  (a') leg (a) again in a slot of its own: the difference of the two medians is a spread
  (b)  the same with the moment launches skipped: the features are computed and dropped (no finish, no host formula)
  (h)  the host formula alone, ``frechet_distance`` at d = 384
and (c) vg_moments_update alone, back to back in the stream, n = 256 at d = 384, 512, 768, 2048, next to torch's own fp64 ``addmm_``
on the widened tensor (gram.addmm_(x64.T, x64), the widening not timed, plus the column sum as a second launch) as the vendor's
yardstick."""
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
from vit_gan_amd.config import Config  # noqa: E402
from vit_gan_amd.data import DeviceDataset  # noqa: E402
from vit_gan_amd.generator import SirenGenerator  # noqa: E402
from vit_gan_amd.metrics import FeatureMoments, FrechetDistance, frechet_distance, quantize_images  # noqa: E402

ROUNDS = 5


def wall(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps  # ms per repetition


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per repetition


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-fake", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fid_bench needs the MI355X: there is nothing to time without it")
    torch.manual_seed(0)
    c2 = Config(embeddings_dimension=384, transformer_blocks_count=6, classes_count=1)
    G = SirenGenerator().cuda()
    images = torch.randint(0, 256, (2048, 3, 32, 32), dtype=torch.uint8)
    ev = FrechetDistance.random_vit(c2, seed=0, n_fake=args.n_fake, batch=args.batch).fit_real(DeviceDataset(images, device="cuda"))

    def whole():
        return ev(G)

    def dropped():  # the evaluator's loop from its public pieces, without the accumulator
        G.eval()
        with torch.no_grad():
            for z, labels in ev.latents(G, torch.device("cuda", torch.cuda.current_device())):
                ev.features(quantize_images(G(z), ev.lut))

    score = whole()  # warm-up of every shape, the smaller last batch included
    dropped()
    legs = {"a": [], "a2": [], "b": []}
    for _ in range(ROUNDS):
        legs["a"].append(wall(whole))
        legs["b"].append(wall(dropped))
        legs["a2"].append(wall(whole))
    assert whole() == score, "two evaluations of an unchanged generator differ"
    mean, cov = ev.fake.moments()
    host = [wall(lambda: frechet_distance(ev.real["mean"], ev.real["cov"], mean, cov)) for _ in range(ROUNDS)]

    batches = -(-args.n_fake // args.batch)
    lines = [f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}, {torch.get_num_threads()} host threads",
             f"one evaluation at the C2 geometry, n_fake = {args.n_fake}, batch = {args.batch} ({batches} batches), quantize on, ms on the wall clock, "
             f"{ROUNDS} alternating rounds after one warm-up of each leg; distance {score:.6f} (random bytes against an untrained generator)"]
    names = {"a": "(a)  whole evaluation", "a2": "(a') the same again", "b": "(b)  moment launches skipped"}
    for k in ("a", "a2", "b"):
        lines.append(f"  {names[k]:<32} {med(legs[k]):9.3f}  (rounds {[round(v, 3) for v in legs[k]]})")
    lines.append(f"  (h)  frechet_distance on the host   {med(host):9.3f}  (rounds {[round(v, 3) for v in host]})")
    spread = max(legs["a"]) - min(legs["a"])
    lines.append(f"  |(a) - (a')| = {abs(med(legs['a']) - med(legs['a2'])):.3f} ms;  (a) - (b) = {med(legs['a']) - med(legs['b']):.3f} ms "
                 f"(of which the host formula {med(host):.3f});  round-to-round spread of (a): {spread:.3f} ms;  "
                 f"per batch (a) {med(legs['a']) / batches * 1e3:.1f} us")

    lines.append("(c) vg_moments_update alone, n = 256, back to back in the stream, us per launch (3 rounds of 200 after 20 warm-up); "
                 "torch: gram.addmm_(x64.T, x64) + sum.add_(x64.sum(0)) on the already widened tensor")
    for d in (384, 512, 768, 2048):
        x = torch.randn(256, d, device="cuda")
        x64 = x.double()
        m = FeatureMoments(d, "cuda")
        gram, s = torch.zeros(d, d, dtype=torch.float64, device="cuda"), torch.zeros(d, dtype=torch.float64, device="cuda")

        def ours():
            m.update(x)

        def vendor():
            gram.addmm_(x64.t(), x64)
            s.add_(x64.sum(0))
        for fn in (ours, vendor):
            timed(fn, 20)
        o, v = [timed(ours, 200) for _ in range(3)], [timed(vendor, 200) for _ in range(3)]
        flop = 2.0 * 256 * d * d  # the full product's count; the kernel computes the upper tile triangle and mirrors it
        lines.append(f"  d = {d:<5} vg_moments_update {med(o):8.2f}  (rounds {[round(t, 2) for t in o]})   torch fp64 addmm_ + sum {med(v):8.2f}  "
                     f"(rounds {[round(t, 2) for t in v]})   {flop / 1e6:.0f} MFLOP of fp64 as a full product -> {flop / med(o) / 1e6:.2f} TFLOP/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
