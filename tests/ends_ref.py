"""float64 restatements, input makers and derived bounds for the kernels at the two ends of the networks (csrc/elementwise.hip): the
classifier head, the batch sum and the embedding's small gradients, the row movers, patchify, the slab folds, the position table and
the SIREN gradient.  A plain helper module, imported like norm_ref; tests/test_ends_gpu.py holds the kernels to it through their own C
entry points, tests/test_ends_ref_cpu.py checks this module itself.  Nothing here is tuned to what a GPU returns.

The bound for an fp32 sum.  A sum of n fp32 terms, added in ANY order, is within gamma(n) sum|terms| of the exact sum, gamma(n) =
n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: every term passes at most n - 1
additions).  A term that is a product rounded on its own passes one rounding more: n + 1.  So the restatements never encode a
kernel's order of summation, and a rewrite that changes the order stays inside the same contract.

The condition on the inputs.  The random probes draw every factor with a magnitude in [lo, hi] bounded away from zero and a random
sign, so every summed term is at least min_term in magnitude; `detects` asserts 2 bound < min_term: a result with one term dropped or
doubled is off by at least min_term - bound > bound, and fails by construction.

The exact probes use small integers and halves, where every intermediate is exactly representable: any order gives the float64
result bit for bit.
"""
import math

import numpy as np
import torch

from exact_util import BF, bf16_ulp, counting, gen, rne

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
HEAD_KMAX, HEAD_ROWS = 16, 32   # VG_HEAD_KMAX, VG_HEAD_ROWS of csrc/elementwise.hip
COS_EPS_MAX = 2.0 ** -10        # the largest epsilon_cos the SIREN gradient's limit may use: a quarter of a bf16 ulp of a unit cosine


def gamma(n):
    return n * U / (1.0 - n * U)


def detects(bound, min_term, what):
    """the random probe's condition: a dropped or doubled term is outside the bound"""
    worst = float(torch.as_tensor(bound).max())
    assert 2.0 * worst < min_term, f"{what}: bound {worst:.3e} is not below half the smallest term {min_term:.3e}"


def within(got, ref64, lim, what, stats=None, key=None):
    """|got - ref| <= lim elementwise (fp64, cpu); returns and records the worst err / limit"""
    got64 = got.detach().double().cpu()
    ref64, lim = ref64.double(), torch.as_tensor(lim, dtype=F64)
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got64).all()), f"{what}: non-finite values"
    err = (got64 - ref64).abs()
    lim = lim.expand_as(err)
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if stats is not None:
        stats[key or what] = max(stats.get(key or what, 0.0), worst)
    if worst > 1.0:
        idx = tuple(int(i) for i in (ratio > 1.0).nonzero()[0])
        raise AssertionError(f"{what}: {int((ratio > 1.0).sum())} of {err.numel()} elements outside the bound; first at {idx}: got "
                             f"{float(got64[idx])!r} want {float(ref64[idx])!r} limit {float(lim[idx]):.3e}")
    return worst


# ------------------------------------------------------------------------------------------------------------------ inputs
def mags(shape, g, lo=0.25, hi=2.0, dtype=F32):
    """magnitudes uniform in [lo, hi], random signs, rounded to `dtype` (which keeps them inside [lo, hi] for the dyadic ends used
    here), returned as fp64"""
    m = lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)
    s = torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0
    x = (m * s).to(dtype).double()
    assert float(x.abs().min()) >= lo and float(x.abs().max()) <= hi
    return x


def choice(values, shape, g):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


T_HI = 0.96875  # the random head probe's |t| stays below 1 (a tanh output), at a bf16 value


def head_inputs(B, E, Kc, seed=0):
    """random probe: |t| in [0.25, T_HI] (bf16), |W2|, |b2|, |dlog| in [0.25, 2] (fp32); start values of the accumulated outputs"""
    g = gen(seed * 1009 + B * 7 + E * 3 + Kc)
    return {"t": mags((B, E), g, 0.25, T_HI, BF), "W2": mags((Kc, E), g), "b2": mags((Kc,), g), "dlog": mags((B, Kc), g),
            "dW2_0": mags((Kc, E), g), "db2_0": mags((Kc,), g), "db1_0": mags((E,), g)}


def head_exact_inputs(B, E, Kc, seed=0):
    """exact probe: t in {0, +-0.5, +-1} (row 0 is all +-1: the saturated tanh, whose gradient is exactly zero), dlog in {-1, 0, 1},
    integer W2 in [-2, 2] (so |sum_k dlog W2| <= 2 Kc <= 85 at Kc <= 40 and dz = a (1 - t^2), a multiple of 1/4 below 86, is a bf16),
    integer b2 and integer start values"""
    assert 2 * Kc <= 85
    g = gen(seed * 1013 + B * 7 + E * 3 + Kc)
    t = choice([0.0, 0.5, -0.5, 1.0, -1.0], (B, E), g)
    t[0] = choice([1.0, -1.0], (E,), g)
    return {"t": t, "W2": counting((Kc, E), g, -2, 2), "b2": counting((Kc,), g, -8, 8), "dlog": counting((B, Kc), g, -1, 1),
            "dW2_0": counting((Kc, E), g, -8, 8), "db2_0": counting((Kc,), g, -8, 8), "db1_0": counting((E,), g, -8, 8)}


# ---------------------------------------------------------------------------------------------------------- classifier head
def head_fwd(inp):
    """logits [B, Kc] and their bound: E products and the bias, E + 1 terms, each product rounded once (or fused: fewer roundings)"""
    t, W2, b2 = inp["t"], inp["W2"], inp["b2"]
    E = t.shape[1]
    ref = t @ W2.T + b2
    mag = t.abs() @ W2.abs().T + b2.abs()
    return ref, gamma(E + 2) * mag


def head_dz(inp):
    """dz [B, E] in fp64 (before its rounding to bf16) and the floor next to its one bf16 ulp.  a = sum_k dlog W2 is a sum of Kc products
    (gamma(Kc + 1) S, S = sum_k |dlog W2|); d = 1 - t^2 is off by at most 2 u absolutely (the square and the subtraction, both below 1
    in magnitude; none if fused); the product a d is rounded once more: gamma(Kc + 2) S d + 2 u S (1 + gamma)."""
    t, W2, dlog = inp["t"], inp["W2"], inp["dlog"]
    Kc = W2.shape[0]
    d = 1.0 - t * t
    S = dlog.abs() @ W2.abs()
    return (dlog @ W2) * d, gamma(Kc + 2) * S * d + 2.0 * U * S * (1.0 + gamma(Kc + 2))


def head_wgrad(inp, rows=slice(None), start=True):
    """dW2 [Kc, E], db2 [Kc] over the batch rows `rows` (a partial row of the one-launch kernel: its own 32 rows), with their bounds.
    n batch rows, the start value one term more; dW2's terms are products."""
    t, dlog = inp["t"][rows], inp["dlog"][rows]
    n = t.shape[0] + (1 if start else 0)
    w0 = inp["dW2_0"] if start else torch.zeros_like(inp["dW2_0"])
    b0 = inp["db2_0"] if start else torch.zeros_like(inp["db2_0"])
    dW2, magW = dlog.T @ t + w0, dlog.abs().T @ t.abs() + w0.abs()
    db2, magb = dlog.sum(0) + b0, dlog.abs().sum(0) + b0.abs()
    return {"dW2": (dW2, gamma(n + 1) * magW), "db2": (db2, gamma(n) * magb)}


def head_db1(dz_rounded, start=None, rows=slice(None)):
    """the documented contract of db1: the fp32 sum over the batch of the kernel's OWN rounded dz (the tensor fc1's weight gradient
    reads).  dz_rounded: the kernel's output, widened to fp64.  Its terms are not bounded away from zero (they are computed values)."""
    z = dz_rounded[rows].double()
    s0 = torch.zeros(z.shape[1], dtype=F64) if start is None else start
    n = z.shape[0] + (0 if start is None else 1)
    return z.sum(0) + s0, gamma(n) * (z.abs().sum(0) + s0.abs())


def head_parts(B):
    return -(-B // HEAD_ROWS)


def head_part_width(E, Kc):
    return (Kc + 1) * E + Kc


def head_min_terms():
    """the smallest |term| of the random head probe: logits (t W2), dz's inner sum (dlog W2), dW2 (dlog t), db2 (dlog)"""
    return {"logits": 0.25 * 0.25, "dz": 0.25 * 0.25, "dW2": 0.25 * 0.25, "db2": 0.25}


# ------------------------------------------------------------------------------------------ batch sum, embedding's small gradients
def batch_sum_inputs(B, S, E, exact, seed=0):
    g = gen(seed * 1019 + B * 5 + S * 3 + E)
    return counting((B, S, E), g, -4, 4) if exact else mags((B, S, E), g, dtype=BF)


def batch_sum(g):
    """out [S, E] = sum_b g[b]; B exact bf16 terms"""
    return g.sum(0), gamma(g.shape[0]) * g.abs().sum(0)


def embed_inputs(S, E, exact, seed=0):
    g = gen(seed * 1021 + S * 3 + E)
    mk = (lambda shape: counting(shape, g, -8, 8)) if exact else (lambda shape: mags(shape, g))
    return {"tok": mk((S, E)), "cls_0": mk((E,)), "pos_0": mk((S - 1, E)), "bias_0": mk((E,))}


def embed_small_grads(inp):
    """d_cls, d_pos: one addition onto the start value (2 terms); d_bias: S - 1 rows and the start value"""
    tok = inp["tok"]
    S = tok.shape[0]
    return {"d_cls": (inp["cls_0"] + tok[0], gamma(2) * (inp["cls_0"].abs() + tok[0].abs())),
            "d_pos": (inp["pos_0"] + tok[1:], gamma(2) * (inp["pos_0"].abs() + tok[1:].abs())),
            "d_bias": (inp["bias_0"] + tok[1:].sum(0), gamma(S) * (inp["bias_0"].abs() + tok[1:].abs().sum(0)))}


# --------------------------------------------------------------------------------------------------------------- row movers
def take_rows(x, B, S, first, n):
    """x [B S, E] -> [B n, E]: rows first .. first + n - 1 of every image"""
    E = x.shape[1]
    return x.reshape(B, S, E)[:, first:first + n].reshape(B * n, E)


def scatter_cls(src, S):
    """src [B, E] -> [B S, E]: row b S = src[b], zero elsewhere"""
    B, E = src.shape
    g = torch.zeros(B, S, E, dtype=src.dtype)
    g[:, 0] = src
    return g.reshape(B * S, E)


def patchify(img, P):
    """img [B, C, IH, IH] -> [B G G, C P P], patch (gy, gx) row-major, columns in (c, py, px) order"""
    B, C, IH, _ = img.shape
    G = IH // P
    return img.reshape(B, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * P * P)


def unpatchify(A, B, C, IH, P):
    G = IH // P
    return A.reshape(B, G, G, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, IH, IH)


def add_table(x_bf16, table_f32, T):
    """one float32 addition and one rounding per element: (x.float() + table[r % T]).to(bfloat16)"""
    rows = x_bf16.shape[0]
    return (x_bf16.float() + table_f32[torch.arange(rows) % T]).to(BF)


# --------------------------------------------------------------------------------------------------------------- slab folds
def slab_inputs(nslab, n, stride, exact, seed=0):
    """a [nslab * stride] fp32 buffer whose slices hold n values each and a sentinel (1e30) between them; dst's start values"""
    g = gen(seed * 1031 + nslab * 7 + n)
    mk = (lambda shape: counting(shape, g, -64, 64)) if exact else (lambda shape: torch.randn(shape, generator=g, dtype=F32).double())
    buf = torch.full((nslab, stride), 1e30, dtype=F64)
    buf[:, :n] = mk((nslab, n))
    return buf.float(), mk((n,)).float()


def slab_reduce(slab, n, start, accumulate):
    """the kernel adds whole slices in slice order onto dst (or +0): a numpy float32 loop in that order, bit for bit"""
    a = start.numpy().astype(np.float32).copy() if accumulate else np.zeros(n, dtype=np.float32)
    s = slab.numpy()
    for k in range(s.shape[0]):
        a = (a + s[k, :n]).astype(np.float32)
    return torch.from_numpy(a)


# ----------------------------------------------------------------------------------------------------------- SIREN gradient
W0 = 30.0
SIN_ARG_MAX = 120.0


def sin_inputs(n, seed=0):
    """dy bf16 with |dy| in [0.25, 2]; z fp32 with |w0 z| <= 120: the first values sit at the multiples k pi / (2 w0), k = -76 .. 76 (the
    zero crossings of the cosine at odd k, its extrema at even k), the rest are uniform over the range"""
    g = gen(seed * 1033 + n)
    kmax = int(SIN_ARG_MAX / (math.pi / 2))
    grid = torch.arange(-kmax, kmax + 1, dtype=F64) * (math.pi / (2 * W0))
    z = (torch.rand(n, generator=g, dtype=F64) * 2 - 1) * (SIN_ARG_MAX - 1.0) / W0
    m = min(n, grid.numel())
    z[:m] = grid[torch.randperm(grid.numel(), generator=g)[:m]]
    z = z.float()
    assert float((z.double() * W0).abs().max()) <= SIN_ARG_MAX
    return mags((n,), g, dtype=BF), z


def sin_arg(z_f32):
    """the fp32 argument the kernel hands to the cosine, w0 z rounded once, as fp64"""
    return (z_f32 * torch.tensor(W0, dtype=F32)).double()


def sin_grad(dy, z_f32, eps_cos):
    """dz = dy w0 cos(w0 z) in fp64 and its limit: one bf16 ulp of the value, the rounding of w0 z carried through |cos'| <= 1
    (2^-24 |w0 z|) and the absolute error eps_cos of the hardware cosine, both scaled by |dy| w0"""
    assert eps_cos <= COS_EPS_MAX, f"epsilon_cos {eps_cos:.3e} exceeds 2^-10: a finding, not a tolerance"
    a = z_f32.double() * W0
    ref = dy * W0 * torch.cos(a)
    return ref, bf16_ulp(ref) + dy.abs() * W0 * (U * a.abs() + eps_cos)


# -------------------------------------------------------------------------------------------- float32 emulations of a sum
def sum_f32(terms, order):
    """float32 sum over axis 0 of fp32 `terms` [n, ...] in one of three orders: 'seq' (first to last), 'rev' (last to first), 'lanes'
    (64 lanes take the terms lane, lane + 64, ... in order, then a butterfly over the lanes)"""
    assert terms.dtype == F32
    n = terms.shape[0]
    if order in ("seq", "rev"):
        idx = range(n) if order == "seq" else range(n - 1, -1, -1)
        a = torch.zeros_like(terms[0])
        for i in idx:
            a = a + terms[i]
        return a
    assert order == "lanes"
    lanes = torch.zeros((64,) + terms.shape[1:], dtype=F32)
    for i in range(n):
        lanes[i % 64] = lanes[i % 64] + terms[i]
    while lanes.shape[0] > 1:
        h = lanes.shape[0] // 2
        lanes = lanes[:h] + lanes[h:]
    return lanes[0]


ORDERS = ("seq", "lanes", "rev")


def exact_in(x64, dtype):
    """x equals its own rounding to dtype"""
    return torch.equal(rne(x64, dtype).double(), x64.double())
