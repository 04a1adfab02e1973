"""Cost of precision / recall / density / coverage and KID, measured in one process on one box:

  python tools/manifold_bench.py [--n 10000] [--d 384] [--k 5] [--n-real 50000] [--out profiles/manifold_bench.txt]

Legs, alternating in rounds after one warm-up of each, timed on the wall clock around a synchronise:
  (a) each launch alone on standard-normal features, n x n at width d: vg_knn_radii (k), vg_ball_counts, vg_poly_kernel_sum, each next
      to the formulation a user would write on the same device - fp64 ``addmm`` of the widened rows in chunks of 2 500 queries (the
      n x n fp64 matrix is 800 MB at n = 10 000), then ``kthvalue`` / the comparison and ``min`` / the cube and ``sum``; the widening
      to fp64 is not timed.  The rate 2 n^2 d / t is quoted against the 34.75 TFLOP/s vg_moments_update reaches at d = 2048
      (profiles/fid_bench.txt).
  (b) one whole evaluation at the C2 geometry (tools/fid_bench.py's), n_fake = n, a real set of n images of random bytes, with the
      options off and on (manifold_k = k, kid): the difference is what an epoch pays.
  (c) the one-time real-side cost at N = n-real rows: the radii and the kernel self-sum that ``fit_real`` computes once."""
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
from vit_gan_amd.metrics import FrechetDistance, ball_counts, knn_radii, poly_kernel_sum  # noqa: E402

ROUNDS = 3
CHUNK = 2500
MOMENTS_TFLOPS = 34.75  # vg_moments_update at d = 2048, profiles/fid_bench.txt


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3  # ms


def med(v):
    return statistics.median(v)


def rounds(v):
    return f"(rounds {[round(t, 3) for t in v]}, spread {max(v) - min(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--n-real", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("manifold_bench needs the MI355X: there is nothing to time without it")
    n, d, k = args.n, args.d, args.k
    g = torch.Generator(device="cuda").manual_seed(0)
    q, c = torch.randn(n, d, device="cuda", generator=g), torch.randn(n, d, device="cuda", generator=g)
    q64, c64 = q.double(), c.double()
    rad = knn_radii(c, k)

    def t_radii():
        nrm, out = (c64 * c64).sum(1), []
        for lo in range(0, n, CHUNK):
            d2 = torch.addmm(nrm[lo:lo + CHUNK, None] + nrm[None, :], c64[lo:lo + CHUNK], c64.t(), alpha=-2.0)
            d2[torch.arange(d2.shape[0]), torch.arange(lo, lo + d2.shape[0])] = float("inf")
            out.append(torch.kthvalue(d2, k, dim=1).values)
        return torch.cat(out)

    def t_balls():
        nq_, nc_, cnt, mn = (q64 * q64).sum(1), (c64 * c64).sum(1), [], []
        for lo in range(0, n, CHUNK):
            d2 = torch.addmm(nq_[lo:lo + CHUNK, None] + nc_[None, :], q64[lo:lo + CHUNK], c64.t(), alpha=-2.0)
            cnt.append((d2 <= rad[None, :]).sum(1))
            mn.append(d2.min(1).values)
        return torch.cat(cnt), torch.cat(mn)

    def t_sum():
        total = torch.zeros((), dtype=torch.float64, device="cuda")
        for lo in range(0, n, CHUNK):
            total += ((q64[lo:lo + CHUNK] @ c64.t() / d + 1.0) ** 3).sum()
        return total

    legs = [("vg_knn_radii", lambda: knn_radii(c, k), "torch addmm + kthvalue", t_radii),
            ("vg_ball_counts", lambda: ball_counts(q, c, rad), "torch addmm + <= + min", t_balls),
            ("vg_poly_kernel_sum", lambda: poly_kernel_sum(q, c), "torch matmul + cube + sum", t_sum)]
    lines = [f"box: {torch.cuda.get_device_name(0)}, host {platform.node()}, torch {torch.__version__}, {torch.get_num_threads()} host threads",
             f"(a) each launch alone, n = {n} x {n}, d = {d}, k = {k}, standard-normal fp32 features, ms on the wall clock, {ROUNDS} alternating "
             f"rounds after one warm-up of each leg; torch: fp64 on the already widened rows, chunks of {CHUNK} queries"]
    flop = 2.0 * n * n * d
    agree = (float((knn_radii(c, k) - t_radii()).abs().max()), int((ball_counts(q, c, rad)[0] != t_balls()[0]).sum()),
             float((poly_kernel_sum(q, c) - t_sum()).abs() / t_sum().abs()))
    for name, ours, tname, theirs in legs:
        wall(ours), wall(theirs)
        o, v = [], []
        for _ in range(ROUNDS):
            o.append(wall(ours))
            v.append(wall(theirs))
        rate = flop / (med(o) * 1e-3) / 1e12
        lines.append(f"  {name:<20} {med(o):9.3f} {rounds(o)}   {tname:<26} {med(v):9.3f} {rounds(v)}   "
                     f"{rate:.2f} TFLOP/s of fp64 = {100 * rate / MOMENTS_TFLOPS:.0f} % of vg_moments_update's {MOMENTS_TFLOPS}")
    lines.append(f"  agreement with the torch legs: max |rad2 difference| {agree[0]:.3e}, counts that differ {agree[1]} of {n}, "
                 f"relative difference of the sums {agree[2]:.3e}")

    torch.manual_seed(0)
    c2 = Config(embeddings_dimension=384, transformer_blocks_count=6, classes_count=1)
    G = SirenGenerator().cuda()
    ds = DeviceDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8), device="cuda")
    off = FrechetDistance.random_vit(c2, seed=0, n_fake=n, batch=args.batch).fit_real(ds)
    on = FrechetDistance.random_vit(c2, seed=0, n_fake=n, batch=args.batch, manifold_k=k, kid=True, bank_real=n)
    t_fit = wall(lambda: on.fit_real(ds))
    s_off, s_on = off(G), on(G)
    assert s_off == s_on, "the distance moved with the options"
    e_off, e_on = [], []
    for _ in range(ROUNDS):
        e_off.append(wall(lambda: off(G)))
        e_on.append(wall(lambda: on(G)))
    last = {key: on.last[key] for key in ("precision", "recall", "density", "coverage", "kid")}
    lines.append(f"(b) one evaluation at the C2 geometry, n_fake = {n}, batch = {args.batch}, {on.last['n_real_bank']} real rows kept, ms; "
                 f"distance {s_on:.6f}, {last} (random bytes against an untrained generator)")
    lines.append(f"  options off                 {med(e_off):9.3f} {rounds(e_off)}")
    lines.append(f"  manifold_k = {k}, kid = True   {med(e_on):9.3f} {rounds(e_on)}")
    lines.append(f"  an epoch pays {med(e_on) - med(e_off):.3f} ms;  fit_real with the options on, once, first call: {t_fit:.3f} ms")

    N = args.n_real
    real = torch.randn(N, d, device="cuda", generator=g)
    wall(lambda: knn_radii(real[:4096], k))
    r_t = [wall(lambda: knn_radii(real, k)) for _ in range(2)]
    s_t = [wall(lambda: poly_kernel_sum(real, real, True)) for _ in range(2)]
    lines.append(f"(c) the real side, once, N = {N}, d = {d}: vg_knn_radii (k = {k}) {med(r_t):.3f} ms {rounds(r_t)}, "
                 f"{2.0 * N * N * d / (med(r_t) * 1e-3) / 1e12:.2f} TFLOP/s;  kernel self-sum {med(s_t):.3f} ms {rounds(s_t)}, "
                 f"{2.0 * N * N * d / (med(s_t) * 1e-3) / 1e12:.2f} TFLOP/s;  no N x N buffer: the fp64 matrix would be {8.0 * N * N / 1e9:.0f} GB")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
