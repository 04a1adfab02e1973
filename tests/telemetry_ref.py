"""The step's telemetry kernels (include/vitgan_hip.h: vg_grad_stats, vg_logit_stats, vg_telemetry_commit) restated off the device - a
plain helper module, no product code:

  * ``grad_stats_ref`` / ``logit_stats_ref`` / ``commit_ref``: the DEFINITIONS in numpy float64, from a slot table.
  * ``grad_stats_emul`` / ``logit_stats_emul``: the kernels' exact fp32 reduction trees, operation for operation (numpy float32 rounds
    every elementwise operation once, as the uncontracted kernel does), with the planted defects the CPU test needs.
  * ``KAPPA`` and the bounds, derived below from the tree - not from anything the code under test returns.
  * ``grad_case``: the synthetic buffer both the CPU and the GPU test use.

The bound on a norm.  u = 2^-24 (fp32 unit roundoff).  An element's square reaches its chunk's partial through
    1 rounding   the product x x
    2 roundings  (x0 x0 + x1 x1) + (x2 x2 + x3 x3) inside its float4 (a peeled head / tail element skips these)
    6 roundings  the thread's serial chain: at most 4 vector terms, then the head term, then the tail term
    6 roundings  the wave butterfly (xor 32 .. 1)
    2 roundings  (w0 + w1) + (w2 + w3)
= 17, so the partial is sum x^2 (1 + d), |d| <= 17 u (all terms are non-negative: no cancellation; second order is below the slack).
Chunk partials are added in fp64 (at most 2^19 of them: 2^19 2^-53 = 2^-34, far below u), sqrt and the product with gscale are fp64.
The square root halves the relative error: 8.5 u; 0.5 u of slack covers everything fp64 and the second-order term; the cast to fp32
adds 1 u.  KAPPA = 10:  |norm - ref| <= 10 * 2^-24 * ref.
fp32 squares below 2^-126 are subnormal (absolute error up to 2^-150 each, or flushed: up to 2^-126): a segment of n elements can lose
at most n 2^-126 of its sum, sqrt(n) 2^-63 of its norm - the absolute floor ``norm_bound`` adds (it matters only for gradients that are
zero to fp32 anyway).
l2 is the same tree with one more fp64 sum: the same KAPPA.  sum_norms adds the rounded norms in fp64 and casts once: the sum of the
segments' bounds plus 1 u of the sum.

The bound on a logit mean.  Thread chain 16, butterfly 6, second butterfly 6, division 1 = 29 roundings on the way of any element:
|mean - ref| <= 29 * 2^-24 * mean|x|.  The fractions are exact integers divided once: float32(count) / float32(n), bit for bit.
"""
from collections import OrderedDict

import numpy as np

U = 2.0 ** -24
KAPPA = 10.0
KAPPA_MEAN = 29.0
CHUNK = 4096
TEL_FIELDS = ("loss_d_real", "loss_d_fake", "loss_g", "d_real_mean", "d_fake_mean", "d_real_acc", "d_fake_acc", "g_mean", "g_frac_pos",
              "gnorm_d_sum", "gnorm_d_l2", "gnorm_g_sum", "gnorm_g_l2", "nonfinite_d", "nonfinite_g", "penalty", "bcr_real", "bcr_fake",
              "ada_p", "ada_rt", "lr_d", "lr_g", "diversity")
TEL_NF = 24
DEFECTS = ("drop_last_partial_chunk", "neighbour_element", "head_as_if_aligned", "no_gscale")


def numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def norm_bound(ref, n, gscale=1.0):
    """the admissible |norm - ref| of a segment of n elements whose fp64 norm is ref"""
    return KAPPA * U * np.abs(ref) + gscale * np.sqrt(np.asarray(n, dtype=np.float64)) * 2.0 ** -63


# ------------------------------------------------------------------------------------------ the definitions, float64
def grad_stats_ref(g, slots, gscale=1.0):
    """norms [n_seg], sum_norms, l2, nonfinite (element count, saturating at 2^24) of the slots of ``g`` in float64"""
    g = np.asarray(g)
    norms, total, bad = [], 0.0, 0
    with np.errstate(invalid="ignore", over="ignore"):
        for off, shape in slots.values():
            x = g[off:off + numel(shape)].astype(np.float64)
            s = float(np.sum(x * x))
            norms.append(gscale * np.sqrt(s))
            total += s
            bad += int(np.count_nonzero(~np.isfinite(x)))
        norms = np.asarray(norms, dtype=np.float64)
        return {"norms": norms, "sum_norms": float(np.sum(norms)), "l2": float(gscale * np.sqrt(total)), "nonfinite": min(bad, 1 << 24)}


def logit_stats_ref(x):
    """(mean in float64, count > 0, count < 0): +-0 and NaN count in neither"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return float(np.mean(x)), int(np.count_nonzero(x > 0)), int(np.count_nonzero(x < 0))


def commit_ref(ring_step, ring, t, cap, fields, order=TEL_FIELDS):
    """one vg_telemetry_commit: row (t - 1) % cap receives t and ``fields`` (name -> value; a missing name is NaN); ``order``: the
    field names by index (the binding's ``_lib.TEL_FIELDS`` when the caller checks that table)"""
    if t < 1:
        return
    r = (t - 1) % cap
    ring_step[r] = t
    ring[r, :] = np.nan
    for i, name in enumerate(order):
        if name in fields:
            ring[r, i] = np.float32(fields[name])


# ------------------------------------------------------------------------------------------ the chunk table (the definition's own builder)
def chunk_table(slots, limit=CHUNK):
    rows, seg_first = [], [0]
    for s, (off, shape) in enumerate(slots.values()):
        n, at = numel(shape), int(off)
        while n > 0:
            c = min(limit, n)
            rows.append((at, c, s))
            at, n = at + c, n - c
        seg_first.append(len(rows))
    return np.asarray(rows, dtype=np.int64), np.asarray(seg_first, dtype=np.int64)


# ------------------------------------------------------------------------------------------ the kernel's trees, float32
_LANE = np.arange(64)


def _butterfly(w):
    """[.., 64] float32: the xor butterfly 32 .. 1; every lane ends with the same value"""
    o = 32
    while o:
        w = w + w[..., _LANE ^ o]
        o >>= 1
    return w


def chunk_partial_emul(g, first, count, head_as_if_aligned=False):
    """(sum of squares of g[first, first + count) by the kernel's tree in float32, its non-finite elements)"""
    f32 = np.float32
    if head_as_if_aligned:  # the planted defect: the vector loop starts at the 16-byte boundary below ``first``
        first -= first % 4
    head = min((4 - first % 4) % 4, count)
    nv, tail = (count - head) // 4, (count - head) % 4
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.zeros(256, dtype=f32)
        body = np.asarray(g[first + head:first + head + 4 * nv], dtype=f32).reshape(nv, 4)
        sq = body * body
        q = np.zeros(1024, dtype=f32)
        q[:nv] = (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3])
        for k in range(4):
            a = a + q[256 * k:256 * (k + 1)]
        if head:
            h = np.asarray(g[first:first + head], dtype=f32)
            a[:head] = a[:head] + h * h
        if tail:
            h = np.asarray(g[first + head + 4 * nv:first + count], dtype=f32)
            a[:tail] = a[:tail] + h * h
        w = _butterfly(a.reshape(4, 64))[:, 0]
        part = (w[0] + w[1]) + (w[2] + w[3])
    return f32(part), int(np.count_nonzero(~np.isfinite(np.asarray(g[first:first + count], dtype=f32))))


def grad_stats_emul(g, slots, gscale=1.0, defect=None, limit=CHUNK, table=None):
    """vg_grad_stats as the kernel computes it; ``defect``: one of DEFECTS planted into it; ``table``: (chunks, seg_first) to walk
    instead of this module's own - the product's ``ops.grad_chunks(slots)[:2]``, the table the kernel is really given"""
    assert defect is None or defect in DEFECTS, defect
    chunks, seg_first = chunk_table(slots, limit) if table is None else (np.asarray(table[0], dtype=np.int64), np.asarray(table[1], dtype=np.int64))
    n_seg = len(seg_first) - 1
    norms32, sums, bad = np.zeros(n_seg, dtype=np.float32), np.zeros(n_seg), 0
    scale = 1.0 if defect == "no_gscale" else float(np.float32(gscale))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(n_seg):
            acc = 0.0
            cs = chunks[seg_first[s]:seg_first[s + 1]]
            for i, (first, count, _) in enumerate(cs):
                last = i == len(cs) - 1
                if defect == "drop_last_partial_chunk" and last and count < limit and len(cs) > 1:
                    continue
                if defect == "neighbour_element" and last:
                    count += 1
                p, b = chunk_partial_emul(g, int(first), int(count), head_as_if_aligned=defect == "head_as_if_aligned")
                acc += float(p)
                bad += b
            sums[s] = acc
            norms32[s] = np.float32(scale * np.sqrt(acc))
        return {"norms": norms32, "sum_norms": np.float32(np.sum(norms32.astype(np.float64))),
                "l2": np.float32(scale * np.sqrt(np.sum(sums))), "nonfinite": min(bad, 1 << 24)}


def logit_stats_emul(x):
    """(mean, frac_pos, frac_neg) float32 as vg_logit_stats computes them"""
    f32 = np.float32
    x = np.asarray(x, dtype=f32).reshape(-1)
    n = x.size
    pad = np.zeros(16 * 1024, dtype=f32)
    pad[:n] = x
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.zeros(1024, dtype=f32)
        for k in range((n + 1023) // 1024):
            a = a + pad[1024 * k:1024 * (k + 1)]
        w = _butterfly(a.reshape(16, 64))[:, 0]
        lane = np.zeros(64, dtype=f32)
        lane[:16] = w
        s = _butterfly(lane)[0]
        fn = f32(n)
        return f32(s / fn), f32(f32(np.count_nonzero(x > 0)) / fn), f32(f32(np.count_nonzero(x < 0)) / fn)


# ------------------------------------------------------------------------------------------ the shared synthetic case
CASE_LENGTHS = (1, 3, 4, 5, 64, 4095, 4096, 4097, 1000003, 4097, 7, 5, 4096, 1)
CASE_ADJACENT = (10, 11, 13)  # these segments start directly behind their predecessor: no padding element between


def grad_case(seed=0):
    """(g float32 [total], slots): segments of CASE_LENGTHS, their first elements walking through offsets 0, 1, 2, 3 mod 4, NaN in every
    padding element, N(0, 1) values with the first and the last element of a segment set to sqrt(n) / 4 - each about 6 % of the
    segment's sum of squares, so a reduction that misses either is far outside the bound."""
    rng = np.random.default_rng(seed)
    slots, cur = OrderedDict(), 0
    for i, n in enumerate(CASE_LENGTHS):
        if i == 0 or i in CASE_ADJACENT:
            off = cur
        else:
            off = cur + 1 + (((i + 1) % 4) - (cur + 1)) % 4  # at least one padding element, and offset (i + 1) mod 4
        slots[f"seg{i}.n{n}"] = (off, (n,))
        cur = off + n
    total = (cur + 1 + 3) // 4 * 4
    g = np.full(total, np.nan, dtype=np.float32)
    for off, (n,) in slots.values():
        x = rng.standard_normal(n).astype(np.float32)
        x[0] = x[-1] = np.float32(max(np.sqrt(n) / 4.0, 0.5))
        g[off:off + n] = x
    return g, slots
