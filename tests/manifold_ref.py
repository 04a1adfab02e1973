"""Brute-force numpy restatements for the manifold-metric tests (precision / recall / density / coverage, KID) and the case generator
both test files share.  Squared distances come from DIFFERENCES, sum (a - b)^2 - int64 for integer-valued features, fp64 otherwise -
never from the Gram identity |a|^2 + |b|^2 - 2 a.b, so nothing here shares a cancellation with the kernels.  A plain helper module
(imported like metrics_ref); nothing here imports the product code."""
import numpy as np

U = 2.0 ** -53  # the unit round-off of fp64


def _is_int(*arrays):
    return all(np.issubdtype(np.asarray(a).dtype, np.integer) for a in arrays)


def d2(a, b):
    """[na, nb] squared distances: int64 when both sets are integer arrays, else fp64, from differences, a block of rows at a time"""
    dt = np.int64 if _is_int(a, b) else np.float64
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)
    out = np.empty((a.shape[0], b.shape[0]), dtype=dt)
    step = max(1, (1 << 22) // max(1, b.shape[0] * b.shape[1]))
    for lo in range(0, a.shape[0], step):
        diff = a[lo:lo + step, None, :] - b[None, :, :]
        out[lo:lo + step] = (diff * diff).sum(-1)
    return out


def sq_norms(a):
    a = np.asarray(a).astype(np.float64)
    return (a * a).sum(-1)


def radii(x, k, d2_fn=d2):
    """rad2_k(x_i; X): the k-th smallest of { d2(x_i, x_j) : j != i }, self excluded by index"""
    dd = d2_fn(x, x)
    n = dd.shape[0]
    off = dd[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.sort(off, axis=1)[:, k - 1]


def ball_counts(q, c, rad2_c, d2_fn=d2):
    """(count [nq] int64, min_d2 [nq]): #{ j : d2(q_i, c_j) <= rad2_c[j] } and min_j d2(q_i, c_j)"""
    dd = d2_fn(q, c)
    return (dd <= np.asarray(rad2_c)[None, :]).sum(1).astype(np.int64), dd.min(1)


def prdc(real, fake, k, d2_fn=d2):
    """the four ratios, integer counts over integer sizes (the definitions of DESIGN.md s7)"""
    rad_r, rad_g = radii(real, k, d2_fn), radii(fake, k, d2_fn)
    count_g, _ = ball_counts(fake, real, rad_r, d2_fn)
    count_r, min_r = ball_counts(real, fake, rad_g, d2_fn)
    M, N = len(fake), len(real)
    return {"precision": int((count_g > 0).sum()) / M, "recall": int((count_r > 0).sum()) / N,
            "density": int(count_g.sum()) / (k * M), "coverage": int((min_r <= rad_r).sum()) / N}


def kappa(q, c):
    """(q_i . c_j / d + 1)^3 in fp64, [nq, nc]"""
    q, c = np.asarray(q).astype(np.float64), np.asarray(c).astype(np.float64)
    return (q @ c.T / q.shape[1] + 1.0) ** 3


def kernel_sum(q, c, skip_diagonal=False):
    kap = kappa(q, c)
    if skip_diagonal:
        kap = kap.copy()
        np.fill_diagonal(kap, 0.0)
    return float(kap.sum())


def kernel_sum_int(q, c, skip_diagonal=False):
    """the same for integer features and d a power of two, in int64: sum (q.c + d)^3, to be divided by d^3 (exact in fp64 while the
    sum stays below 2^53) -> (numerator, d^3)"""
    q, c = np.asarray(q).astype(np.int64), np.asarray(c).astype(np.int64)
    d = q.shape[1]
    cube = (q @ c.T + d) ** 3
    if skip_diagonal:
        np.fill_diagonal(cube, 0)
    return int(cube.sum()), d ** 3


def kernel_sum_bound(q, c):
    """nq nc 2^-52 sum |kappa|: the worst-case bound of an fp64 sum of nq nc terms in any order, the terms' own rounding included"""
    return len(q) * len(c) * 2.0 ** -52 * float(np.abs(kappa(q, c)).sum())


def kid(real, fake):
    """the unbiased MMD^2 estimate over the full sets"""
    M, N = len(fake), len(real)
    return kernel_sum(fake, fake, True) / (M * (M - 1)) + kernel_sum(real, real, True) / (N * (N - 1)) - 2.0 * kernel_sum(fake, real) / (M * N)


def kid_bound(real, fake):
    M, N = len(fake), len(real)
    return kernel_sum_bound(fake, fake) / (M * (M - 1)) + kernel_sum_bound(real, real) / (N * (N - 1)) + 2.0 * kernel_sum_bound(fake, real) / (M * N)


def gram_bound(a, b):
    """[na, nb]: 4 (d + 2) 2^-53 (|a|^2 + |b|^2), the bound on a squared distance formed by the Gram identity from fp64 dot products of d
    terms (two norms and a doubled dot, gamma_d each, and the three roundings of the combination)"""
    d = np.asarray(a).shape[1]
    return 4.0 * (d + 2) * U * (sq_norms(a)[:, None] + sq_norms(b)[None, :])


def margin(q, c, rad2_c):
    """min_ij |d2(q_i, c_j) - rad2_c[j]| / (|q_i|^2 + |c_j|^2): how far the nearest comparison is from flipping, in the bound's units"""
    dd = d2(q, c).astype(np.float64)
    return float((np.abs(dd - np.asarray(rad2_c, dtype=np.float64)[None, :]) / (sq_norms(q)[:, None] + sq_norms(c)[None, :])).min())


def case_margin(real, fake, k):
    """the smallest margin of EVERY comparison behind prdc(real, fake, k): fakes in real balls, reals in fake balls, and each real's
    nearest fake against its own radius (coverage)"""
    rad_r, rad_g = radii(real, k), radii(fake, k)
    dd = d2(real, fake).astype(np.float64)
    own = np.abs(dd.min(1) - rad_r) / (sq_norms(real) + sq_norms(fake)[dd.argmin(1)])
    return min(margin(fake, real, rad_r), margin(real, fake, rad_g), float(own.min()))


def margin_needed(d):
    """1000 x the kernel's relative error bound"""
    return 1000.0 * 4.0 * (d + 2) * U


# ----------------------------------------------------------------------------------------------------------------------- cases
# normal (non-integer) feature cases of the GPU tests: name -> (nq, nc, d, k, mean, seed).  The seeds are chosen in
# tests/test_manifold_cpu.py's margin test, on the CPU: every comparison d2 <= rad2 of a case is further than 1000 error bounds from
# flipping, so exact equality of the counts on the GPU is a fair demand.
NORMAL_CASES = {
    "unit-48": (100, 257, 48, 3, 0.0, 1),
    "unit-384": (40, 65, 384, 5, 0.0, 2),
    "tiny-16": (17, 33, 16, 1, 0.0, 3),
    "offset100-48": (65, 130, 48, 5, 100.0, 4),
    "offset100-384": (20, 40, 384, 3, 100.0, 5),
}


def normal_case(name):
    """(q [nq, d], c [nc, d]) fp32: mean + standard normal"""
    nq, nc, d, _, mean, seed = NORMAL_CASES[name]
    g = np.random.default_rng(seed)
    return ((mean + g.standard_normal((nq, d))).astype(np.float32), (mean + g.standard_normal((nc, d))).astype(np.float32))


def integer_set(n, d, seed, lo=-3, hi=3, copies=0):
    """int64 [n, d] in [lo, hi]; with ``copies`` the first row is repeated at the last ``copies`` indices (exact duplicates, ties)"""
    x = np.random.default_rng(seed).integers(lo, hi + 1, (n, d)).astype(np.int64)
    if copies:
        x[n - copies:] = x[0]
    return x
