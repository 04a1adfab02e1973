"""float64 restatements and checkers for the bf16 first-order normalisation family of csrc/norm.hip: LayerNorm and self-modulated
LayerNorm (SLN) forward and backward, and the two column sums.  A plain helper module, imported like second_order_ref.

Every function is written once and evaluated in the precision it is asked for.  dtype = float64 is the reference that
tests/test_norm_gpu.py holds the kernels to.  dtype = float32 is an emulation of the kernel: the same operations, every tensor cast
to float32 on entry, the row and column sums in the kernel's own order (lanes, shuffles, trips of the grid-stride loop, waves, the
fold of vg_colsum_f32), no float64 inside.  tests/test_norm_ref_cpu.py feeds the emulation, and every planted mistake of MUTANTS,
through the assertions the GPU test uses: the emulation must pass them all, every mutant must fail one.

All inputs are bf16-valued; gamma, beta, lw, lb, gs and bs are fp32-valued.  Next to every output the functions return ``mag``, in the
convention of second_order_ref: an fp32 evaluation of depth kappa is within kappa * 2^-24 * mag of the exact value.
"""
import torch

from exact_util import BF, assert_bitwise, bf16_ulp, rne
from second_order_ref import F64, LN_EPS, assert_elementwise, assert_fit, fit_terms, ln_fit_runs, ln_inputs, ln_stats

F32 = torch.float32
U = 2.0 ** -24
WIDTHS = [128, 256, 384, 512, 640, 768, 896, 1024]
FWD_LPR, BWD_LPR = 16, 32      # lanes per row: forward kernels, backward kernels (LN_BWD_LPR = SLN_BWD_LPR = 32 in csrc/norm.hip)
LN_MAX_PARTS = 512             # grid cap of the backward kernels
CS_ROWS = 256                  # rows per workgroup of vg_colsum_bf16
# Maximum error of rsqrtf in ulp.  The single-precision table of the HIP math API reference ("HIP math API", section "Single precision
# mathematical functions", row rsqrtf) gives 1 ulp; the function is __ocml_rsqrt_f32 (clang's __clang_hip_math.h), which is the
# hardware's v_rsq_f32 behind a rescaling of denormal arguments.  An ulp is at most 2^-23 of the value.
RSQRT_ULPS = 1


def bwd_parts(R):
    """vg_layernorm_bwd_parts: one workgroup pass covers 4 waves x (64 / LPR = 2) rows, but the grid is sized for 16 rows a workgroup"""
    return min(-(-R // 16), LN_MAX_PARTS)


def bwd_trips(R):
    """trips of the backward's grid-stride loop: a pass of the whole grid covers 8 * parts rows"""
    return -(-R // (8 * bwd_parts(R)))


def colsum_bf16_parts(R):
    return -(-R // CS_ROWS)


# ------------------------------------------------------------------------------------------------------------------- kappa
def kappa_stat(E):
    """mean: 8 NV serial adds in a lane (NV = E / 128 chunks of 8 columns), 4 shuffle levels over the 16 lanes of a row, then the
    product with the rounded constant 1 / E (2: the constant and the product).  In units of 2^-24 * mean_c |x|."""
    return 8 * (E // 128) + 4 + 2


def kappa_var(E):
    """var + eps, relative to itself given the computed mean: c = x - mu is rounded and enters squared (2), the square (1), 8 NV serial
    adds, 4 shuffle levels, the product with 1 / E (2), the rounding of eps to fp32 and the addition (2)."""
    return 2 + 1 + 8 * (E // 128) + 4 + 2 + 2


def rstd_rel_bound(mean_abs_x, var, E, eps):
    """relative bound on rstd per row.  v = var + eps is computed around the kernel's own mean mu', off by d <= kappa_stat 2^-24
    mean_c |x|; as sum_c (x - mu) = 0, that adds exactly d^2 to the variance.  So v is off by at most r_v = kappa_var 2^-24 + d^2 / v
    relative, v^-1/2 by r_v / 2 (1 + r_v) for r_v < 0.01, and rsqrtf adds RSQRT_ULPS ulp of at most 2^-23 each."""
    d = kappa_stat(E) * U * mean_abs_x
    rv = kappa_var(E) * U + d * d / (var + eps)
    return 0.5 * rv * (1 + rv) + RSQRT_ULPS * 2.0 ** -23


def kappa_fwd(E, sln=False):
    """the longest path to one y, every operation counted once: the mean (kappa_stat), x - mu, the square, the second row sum and its
    1 / E (8 NV + 4 + 2), eps and its addition (2), rsqrtf (2 RSQRT_ULPS: an ulp is two units of 2^-24), then (x - mu) rs gamma + beta
    (the subtraction is already counted: 3).  SLN: g_s l + b_s and the product with w (3 more).  The error of the mean is taken
    relative to mag_y's |x| + |mean|; where mean_c |x| is larger than that, |beta| (|lb|, |bs|) in mag_y carries it."""
    nv = E // 128
    return kappa_stat(E) + 1 + 1 + (8 * nv + 4 + 2) + 2 + 2 * RSQRT_ULPS + 3 + (3 if sln else 0)


def kappa_dx(E, sln=False):
    """the longest path to one dx, through c2 = mean_c(g xh): xh = (x - mu) rs (2), g = dy gamma (1), g xh (1), CH NV serial adds in a
    lane with CH = 128 / LPR = 4 columns a chunk, log2(LPR) = 5 shuffle levels, 1 / E (2), xh c2 (1), g - c1 - xh c2 (2), the product
    with rs (1), + gres (1).  SLN: dy_eff = dy (w g_s) (2 more).  mean and rstd are inputs of the kernel: they carry no error."""
    ch = 128 // BWD_LPR
    return 2 + 1 + 1 + ch * (E // 128) + 5 + 2 + 1 + 2 + 1 + 1 + (2 if sln else 0)


def fold_depth(rows):
    """vg_colsum_f32: thread (rl, c) adds rows rl, rl + 16, ... serially (ceil(rows / 16)), then one thread adds the 16 partials (16)"""
    return -(-rows // 16) + 16


def kappa_colsums(E, R, sln=False, scalar=False):
    """the column sums of the backward.  The element dy_eff xh: xh (2), the product (1), SLN dy_eff (2).  A lane adds one such element
    per trip of the grid-stride loop (trips), the 64 / LPR = 2 row groups of a wave are folded by one shuffle level (1), the four waves in
    two levels (2), then vg_colsum_f32 over the parts partial rows.
    scalar (d gs, d bs of the SLN): the element dy w l with l = xh lw + lb (2 + 2 + 2); a lane adds its CH NV columns of every trip
    serially, a wave sum of 6 shuffle levels, the four waves (2), then the fold."""
    parts, trips = bwd_parts(R), bwd_trips(R)
    if scalar:
        return 6 + (128 // BWD_LPR) * (E // 128) * trips + 6 + 2 + fold_depth(parts)
    return 3 + (2 if sln else 0) + trips + 1 + 2 + fold_depth(parts)


def kappa_dw():
    """dw_acc (+)= dy (g_s (xh lw + lb) + b_s): xh (2), four operations inside, the product with dy (1), the accumulation (1)"""
    return 2 + 4 + 1 + 1


def kappa_colsum_bf16(R):
    """vg_colsum_bf16: a thread adds rows rl, rl + 8, ... of its chunk of CS_ROWS = 256 rows (ceil(256 / 8) = 32), one thread adds the 8
    row lanes (8), then vg_colsum_f32 over the ceil(R / 256) chunks"""
    return CS_ROWS // 8 + 8 + fold_depth(colsum_bf16_parts(R))


# ---------------------------------------------------------------------------------------------- sums in the kernel's order
def _halve(s):
    """a butterfly over the last dimension (__shfl_xor with the offsets high to low): every lane ends with the same sum"""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def _rowsum(t, lpr):
    """sum over the columns of [R, E]: float64 plainly; float32 as the kernel does: lane `sub` of a row owns the chunks sub, sub + lpr,
    ... of 128 / lpr columns and adds them in order, then the lanes of the row are folded by shuffles"""
    if t.dtype == F64:
        return t.sum(-1)
    R, E = t.shape
    ch = 128 // lpr
    v = t.reshape(R, E // 128, lpr, ch)
    s = torch.zeros(R, lpr, dtype=F32)
    for i in range(E // 128):
        for j in range(ch):
            s = s + v[:, i, :, j]
    return _halve(s)


def _rowmean(t, lpr):
    return _rowsum(t, lpr) * (1.0 / t.shape[-1])


def fold(part):
    """vg_colsum_f32 over the rows of an fp32 [rows, C] in its own order (float64: a plain sum)"""
    if part.dtype == F64:
        return part.sum(0)
    rows, C = part.shape
    n = -(-rows // 16)
    p = torch.zeros(n * 16, C, dtype=F32)
    p[:rows] = part
    p = p.reshape(n, 16, C)
    lane = torch.zeros(16, C, dtype=F32)
    for i in range(n):
        lane = lane + p[i]
    a = torch.zeros(C, dtype=F32)
    for k in range(16):
        a = a + lane[k]
    return a


def _slots(t):
    """[R, C] -> [trips, parts, 4 waves, 2 row groups, C], zero rows behind R: the backward's dealing of rows to lanes"""
    R, C = t.shape
    parts, trips = bwd_parts(R), bwd_trips(R)
    p = torch.zeros(trips * parts * 8, C, dtype=t.dtype)
    p[:R] = t
    return p.reshape(trips, parts, 4, 2, C)


def _colsum(t):
    """sum over the rows of [R, C] as the backward kernels and vg_colsum_f32 do it between them"""
    if t.dtype == F64:
        return t.sum(0)
    s = _slots(t)
    acc = torch.zeros_like(s[0])
    for trip in range(s.shape[0]):
        acc = acc + s[trip]
    a = acc[:, :, 0] + acc[:, :, 1]
    return fold((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3]))


def _allsum(t):
    """sum of every element of [R, E] as the SLN backward does it for d gs and d bs"""
    if t.dtype == F64:
        return t.sum()
    R, E = t.shape
    ch = 128 // BWD_LPR
    s = _slots(t).reshape(-1, bwd_parts(R), 4, 2, E // 128, BWD_LPR, ch)
    acc = torch.zeros_like(s[0, :, :, :, 0, :, 0])
    for trip in range(s.shape[0]):
        for i in range(E // 128):
            for j in range(ch):
                acc = acc + s[trip, :, :, :, i, :, j]
    w = _halve(acc.reshape(acc.shape[0], 4, 64))
    return fold(((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])).unsqueeze(1))[0]


def colsum_bf16_f32(x):
    """float32 emulation of vg_colsum_bf16 on a bf16-valued [R, N]"""
    x = x.to(F32)
    R, N = x.shape
    chunks = colsum_bf16_parts(R)
    p = torch.zeros(chunks * CS_ROWS, N, dtype=F32)
    p[:R] = x
    p = p.reshape(chunks, CS_ROWS // 8, 8, N)
    lane = torch.zeros(chunks, 8, N, dtype=F32)
    for i in range(CS_ROWS // 8):
        lane = lane + p[:, i]
    t = torch.zeros(chunks, N, dtype=F32)
    for k in range(8):
        t = t + lane[:, k]
    return fold(t)


# ----------------------------------------------------------------------------------------------------------------- mutants
# planted mistakes, each a value of the `mut` keyword of the function family named next to it
MUTANTS = {"unbiased_var": "fwd", "eps_outside_sqrt": "fwd", "one_pass_var": "fwd",
           "drop_c1": "bwd", "drop_c2": "bwd", "c2_without_invE": "bwd", "dgamma_without_xhat": "bwd", "dbeta_of_g": "bwd",
           "gres_twice": "bwd",
           "sln_dw_without_bs": "sln_bwd", "sln_dgs_without_lb": "sln_bwd", "sln_dy_eff_without_gs": "sln_bwd",
           "bcast_off_by_one": "bcast"}


def _cast(dtype, *ts):
    return [None if t is None else t.to(dtype) for t in ts]


def _bcast(h, R, bcast_rows, mut):
    """the row of h that problem row r reads"""
    if bcast_rows <= 0:
        return h
    r = torch.arange(R)
    idx = (r % (bcast_rows + 1)).clamp_max(bcast_rows - 1) if mut == "bcast_off_by_one" else r % bcast_rows
    return h[idx]


def _stats(x, eps, mut):
    E = x.shape[-1]
    mean = _rowmean(x, FWD_LPR)
    if mut == "one_pass_var":   # E[x^2] - mean^2, in float32 whatever the precision of the rest
        x32 = x.to(F32)
        m32 = x32.mean(-1)
        var = ((x32 * x32).mean(-1) - m32 * m32).clamp_min(0.0).to(x.dtype)
    else:
        c = x - mean.unsqueeze(-1)
        var = _rowmean(c * c, FWD_LPR)
    if mut == "unbiased_var":
        var = var * (E / (E - 1.0))
    rstd = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_outside_sqrt" else torch.rsqrt(var + eps)
    return mean, var, rstd


# ----------------------------------------------------------------------------------------------------------------- forward
def ln_fwd(x, gamma, beta, eps=LN_EPS, mut=None, dtype=F64):
    """y = (x - mean) rstd gamma + beta with the biased variance and rstd = (var + eps)^-1/2.  Returns y, mean, rstd and
    mag_y = (|x| + |mean|) rstd |gamma| + |beta|, and for the bounds on the statistics mean_c |x| and the relative bound on rstd."""
    x, gamma, beta = _cast(dtype, x, gamma, beta)
    mean, var, rstd = _stats(x, eps, mut)
    m, r = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    y = (x - m) * r * gamma + beta
    mag = (x.abs() + m.abs()) * r * gamma.abs() + beta.abs()
    max_ = x.abs().mean(-1)
    return {"y": y, "mean": mean, "rstd": rstd, "mag_y": mag, "mean_abs_x": max_, "rstd_rel": rstd_rel_bound(max_, var, x.shape[-1], eps)}


def sln_fwd(h, w, lw, lb, gs, bs, eps=LN_EPS, bcast_rows=0, mut=None, dtype=F64):
    """y = w (gs (LN(h) lw + lb) + bs); bcast_rows > 0: h has that many rows and row r of the problem reads row r % bcast_rows.  mean and
    rstd are per row of the problem, as the kernel writes them."""
    h, w, lw, lb = _cast(dtype, h, w, lw, lb)
    hx = _bcast(h, w.shape[0], bcast_rows, mut)
    mean, var, rstd = _stats(hx, eps, mut)
    m, r = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    y = w * (gs * ((hx - m) * r * lw + lb) + bs)
    mag = w.abs() * (abs(gs) * ((hx.abs() + m.abs()) * r * lw.abs() + lb.abs()) + abs(bs))
    max_ = hx.abs().mean(-1)
    return {"y": y, "mean": mean, "rstd": rstd, "mag_y": mag, "mean_abs_x": max_, "rstd_rel": rstd_rel_bound(max_, var, h.shape[-1], eps)}


# ---------------------------------------------------------------------------------------------------------------- backward
def _bwd_core(d, xh, rstd, gamma, gres, mut):
    """dx = gres + rstd (g - c1 - xh c2) with g = d gamma, c1 = mean_c(g), c2 = mean_c(g xh), and the column sums of d xh and d.
    mag_dx = |gres| + rstd (|g| + mean_c |g| + |xh| mean_c |g xh|): the sum of the absolute values of the terms, taken through the two
    means as second_order_ref does.  The error of a sum is bounded by the absolute values of what it adds, not by its own: with |c1| and
    |c2| in their place the float32 emulation's own error, before any bf16 rounding, reaches 18 x kappa 2^-24 mag at E = 384 (columns
    where gamma = 0 and the two means happen to be small), and 0.12 x with the means of absolute values."""
    E = d.shape[-1]
    r = rstd.unsqueeze(-1)
    g = d * gamma
    c1 = _rowmean(g, BWD_LPR).unsqueeze(-1)
    c2 = _rowmean(g * xh, BWD_LPR).unsqueeze(-1)
    if mut == "c2_without_invE":
        c2 = c2 * E
    if mut == "drop_c1":
        c1 = c1 * 0.0
    if mut == "drop_c2":
        c2 = c2 * 0.0
    dx = r * (g - c1 - xh * c2)
    if gres is not None:
        dx = dx + gres * (2.0 if mut == "gres_twice" else 1.0)
    terms = [r * g, (-r * c1).expand_as(g), -r * xh * c2]
    mag = r * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if gres is not None:
        mag = mag + gres.abs()
    ga = d if mut == "dgamma_without_xhat" else d * xh
    be = g if mut == "dbeta_of_g" else d
    out = {"dx": dx, "dx_terms": terms, "mag_dx": mag,
           "dgamma": _colsum(ga), "mag_dgamma": (d * xh).abs().sum(0), "dbeta": _colsum(be), "mag_dbeta": d.abs().sum(0)}
    if d.dtype == F32:   # the third partial segment: the column sum of the rounded dx itself
        out["dxsum"] = _colsum(dx.to(BF).to(F32))
    return out


def ln_bwd(dy, x, mean, rstd, gamma, gres=None, mut=None, dtype=F64):
    """mean and rstd are arguments, as for the kernel.  Returns dx, its three terms (dx - gres), mag_dx, dgamma = sum_r dy xh and
    dbeta = sum_r dy with the column sums of absolute values as magnitudes.  (float32 only: dxsum, the column sum of rne(dx).)"""
    dy, x, mean, rstd, gamma, gres = _cast(dtype, dy, x, mean, rstd, gamma, gres)
    xh = (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    return _bwd_core(dy, xh, rstd, gamma, gres, mut)


def sln_bwd(dy, h, w, mean, rstd, lw, lb, gs, bs, gres=None, bcast_rows=0, mut=None, dtype=F64):
    """dh (per row of the problem, before any sum over the batch of a broadcast h) from dy_eff = dy w gs; dw = dy (gs (xh lw + lb) + bs);
    dlw, dlb as dgamma, dbeta of dy_eff; dgs = sum dy w l and dbs = sum dy w with l = xh lw + lb."""
    dy, h, w, mean, rstd, lw, lb, gres = _cast(dtype, dy, h, w, mean, rstd, lw, lb, gres)
    hx = _bcast(h, dy.shape[0], bcast_rows, mut)
    xh = (hx - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    l = xh * lw + lb
    mag_l = (xh * lw).abs() + lb.abs()
    d = dy * w if mut == "sln_dy_eff_without_gs" else dy * (w * gs)
    out = _bwd_core(d, xh, rstd, lw, gres, mut)
    out = {{"dx": "dh", "dx_terms": "dh_terms", "mag_dx": "mag_dh", "dgamma": "dlw", "mag_dgamma": "mag_dlw", "dbeta": "dlb",
            "mag_dbeta": "mag_dlb"}.get(k, k): v for k, v in out.items()}
    out["dw"] = dy * (gs * l) if mut == "sln_dw_without_bs" else dy * (gs * l + bs)
    out["mag_dw"] = dy.abs() * (abs(gs) * mag_l + abs(bs))
    out["dgs"] = _allsum(dy * w * (xh * lw)) if mut == "sln_dgs_without_lb" else _allsum(dy * w * l)
    out["mag_dgs"] = ((dy * w).abs() * mag_l).sum()
    out["dbs"] = _allsum(dy * w)
    out["mag_dbs"] = (dy * w).abs().sum()
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def norm_inputs(R, E, seed, bcast_rows=0):
    """ln_inputs' x (mixed rows, rows with mean 8 and std 2^-5, rows with std 30, one constant row, one spike row), dy and gamma (two
    exact zeros; also the SLN's lw), its u as gres, and beta ~ 0.3 N, lb ~ 0.3 N, w ~ N(0, 1) with one zero row (R >= 4),
    (gs, bs) = (0.7, -0.4) as fp32 values.  bcast_rows > 0: h is ln_inputs' x of that many rows (else h = x)."""
    u, dy, x, gamma = ln_inputs(R, E, seed)
    g = torch.Generator().manual_seed(seed * 7919 + R * 13 + E + 5)
    beta = (0.3 * torch.randn(E, generator=g, dtype=F64)).float().double()
    lb = (0.3 * torch.randn(E, generator=g, dtype=F64)).float().double()
    w = torch.randn(R, E, generator=g, dtype=F64).to(BF).double()
    if R >= 4:
        w[R // 2] = 0.0
    h = ln_inputs(bcast_rows, E, seed + 77)[2] if bcast_rows > 0 else x
    gs, bs = (float(torch.tensor(v, dtype=F32)) for v in (0.7, -0.4))
    return {"x": x, "dy": dy, "gres": u, "gamma": gamma, "beta": beta, "w": w, "h": h, "lw": gamma, "lb": lb, "gs": gs, "bs": bs}


def tight_rows(R):
    """the rows of ln_inputs with mean 8 and std 2^-5 (the constant and spike rows, R - 2 and R - 1, overwrite two of the pattern)"""
    r = torch.arange(R)
    return r[(r % 8 == 5) & (r < R - 2)]


# -------------------------------------------------------------------------------------------------------------- fit bounds
# floors of |c - 1| when rne(sum(terms), bf16) is fitted on the three terms of dx (LayerNorm) and dh (SLN), reference against
# reference: largest of 16 seeds of norm_inputs, R = 1040 for E <= 512 and R = 8192 above, as measured and printed by
# tests/test_norm_ref_cpu.py::test_fit_floors (which asserts 4 x floor <= the bound below).  The fit runs where ln_fit_runs holds.
_FIT_FLOOR = {128: 1.47e-4, 256: 1.31e-4, 384: 1.13e-4, 512: 1.17e-4, 640: 4.02e-5, 768: 3.79e-5, 896: 6.15e-5, 1024: 5.91e-5}
FIT_ROWS = {E: (1040 if E <= 512 else 8192) for E in WIDTHS}


def fit_bound(E):
    """4 x the measured floor of the width (more rows than FIT_ROWS[E] only lower the floor)"""
    return 4.0 * _FIT_FLOOR[E]


def fit_dropped_rows(terms):
    """rows that fit_terms leaves out: their exact sum is zero"""
    return int((sum(terms).abs().amax(-1) == 0).sum())


# ---------------------------------------------------------------------------------------------------------------- checkers
def _sel(t, rows):
    return t if rows is None or t.dim() == 0 else t[rows]


def fwd_assertions(got, ref, E, sln=False, rows=None, what=""):
    """the assertions of the GPU test on a forward (got: y bf16, mean and rstd fp32; ref: ln_fwd / sln_fwd in float64) as (name, thunk)
    pairs; a thunk raises AssertionError or returns the worst err / limit.  rows: restrict to these rows."""
    s = lambda t: _sel(t, rows)  # noqa: E731
    return [
        ("y", lambda: assert_elementwise(s(got["y"]), s(ref["y"]), s(ref["mag_y"]), kappa_fwd(E, sln), f"{what} y")),
        ("mean", lambda: assert_elementwise(s(got["mean"]), s(ref["mean"]), s(ref["mean_abs_x"]), kappa_stat(E), f"{what} mean", rel=0.0)),
        ("rstd", lambda: assert_elementwise(s(got["rstd"]), s(ref["rstd"]), s(ref["rstd_rel"] * ref["rstd"]) * 2.0 ** 24, 1, f"{what} rstd",
                                            rel=0.0)),
    ]


def bwd_assertions(got, ref, R, E, sln=False, rows=None, fit=False, what=""):
    """the assertions on a backward and its folded column sums.  got: dx (dh) bf16 and whichever of dgamma, dbeta (dlw, dlb), dxsum, dw,
    dgs, dbs it holds (fp32); ref: ln_bwd / sln_bwd in float64.  rows restricts the per-row outputs (dx, dw); fit adds the fit of dx
    on its three terms (for a run without gres)."""
    s = lambda t: _sel(t, rows)  # noqa: E731
    dx = "dh" if sln else "dx"
    out = [(dx, lambda: assert_elementwise(s(got[dx]), s(ref[dx]), s(ref["mag_" + dx]), kappa_dx(E, sln), f"{what} {dx}"))]
    if fit:
        out.append((f"fit {dx}", lambda: assert_fit(s(got[dx]), [s(t) for t in ref[dx + "_terms"]], fit_bound(E), f"{what} {dx}") / fit_bound(E)))
    if rows is not None:
        return out
    kc = kappa_colsums(E, R, sln)
    for n in (("dlw", "dlb") if sln else ("dgamma", "dbeta")):
        if n in got:
            out.append((n, lambda n=n: assert_elementwise(got[n], ref[n], ref["mag_" + n], kc, f"{what} {n}", rel=0.0)))
    if "dxsum" in got:   # the column sum of the dx that was returned, in float64
        d64 = got[dx].detach().double().cpu()
        out.append(("dxsum", lambda: assert_elementwise(got["dxsum"], d64.sum(0), d64.abs().sum(0), kc, f"{what} colsum({dx})", rel=0.0)))
    if sln:
        if "dw" in got:
            start = got.get("dw_start")
            ref_dw, mag_dw = (ref["dw"], ref["mag_dw"]) if start is None else (start + ref["dw"], start.abs() + ref["mag_dw"])
            out.append(("dw", lambda: assert_elementwise(got["dw"], ref_dw, mag_dw, kappa_dw(), f"{what} dw", rel=0.0)))
        ks = kappa_colsums(E, R, True, scalar=True)
        for n in ("dgs", "dbs"):
            if n in got:
                out.append((n, lambda n=n: assert_elementwise(got[n].reshape(()), ref[n], ref["mag_" + n], ks, f"{what} {n}", rel=0.0)))
    return out


def const_row_assertions(got, beta, eps, row, what=""):
    """the constant row of a LayerNorm forward: the row sum of E equal bf16 values and its product with 1 / E are exact for the 1.25 of
    ln_inputs, so x - mu = 0 and y = rne(beta) bit for bit; var = 0, so rstd is rsqrtf of the fp32 eps itself"""
    def y():
        assert_bitwise(got["y"][row].detach().cpu().contiguous(), rne(beta, BF), f"{what} y of the constant row {row}")
        return 0.0

    def rstd():
        want = float(torch.tensor(eps, dtype=F32).double()) ** -0.5
        err, lim = abs(float(got["rstd"][row].double()) - want), RSQRT_ULPS * 2.0 ** -23 * want
        assert err <= lim, f"{what} rstd of the constant row {row}: {float(got['rstd'][row])!r} is not eps^-1/2 = {want!r} within {RSQRT_ULPS} ulp"
        return err / lim
    return [("const y", y), ("const rstd", rstd)]


def gres_pair_assertions(got_g, got_0, gres, key, what=""):
    """a run with gres against the same run without.  Both round the same fp32 t = rstd (g - c1 - xh c2): b = rne(t) and
    a = rne(fl(t + gres)), where the product and the addition may be one fma.  So a - b - gres is within half a bf16 ulp of each of the
    two plus the fp32 roundings of t and of the sum (2^-23 |a| + 2^-23 |b|): no kappa, no reference.  The column sums of dy_eff xh and
    dy_eff do not see gres: bit-equal."""
    def diff():
        a, b = got_g[key].detach().double().cpu(), got_0[key].detach().double().cpu()
        lim = 0.5 * bf16_ulp(a) + 0.5 * bf16_ulp(b) + 2.0 ** -23 * (a.abs() + b.abs())
        err = (a - b - gres).abs()
        bad = ~(err <= lim)
        if bool(bad.any()):
            idx = tuple(int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{what} {key}: {int(bad.sum())} elements of (with gres) - (without) differ from gres by more than the two "
                                 f"roundings; first at {idx}: {float(a[idx])!r} - {float(b[idx])!r} vs gres {float(gres[idx])!r}")
        return float((err / lim).max())

    def sums():
        for n in ("dgamma", "dbeta", "dlw", "dlb", "dgs", "dbs"):
            if n in got_g and n in got_0:
                assert_bitwise(torch.atleast_1d(got_g[n].detach().cpu()).contiguous(), torch.atleast_1d(got_0[n].detach().cpu()).contiguous(),
                               f"{what} {n} with and without gres")
        return 0.0
    return [(f"{key} with - without gres", diff), ("sums with = without gres", sums)]


def _named(prefix, pairs):
    return [(prefix + n, f) for n, f in pairs]


def _with_gres(b0, gres, dx):
    """the float64 backward with gres from the one without: gres enters dx and its magnitude, and nothing else"""
    return dict(b0, **{dx: b0[dx] + gres, "mag_" + dx: b0["mag_" + dx] + gres.abs()})


def ln_refs(inp, eps=LN_EPS):
    """float64 references of one LayerNorm case: the forward, the fp32 roundings of its statistics (what the backward kernel and its
    reference are both handed), the backward with gres ('bg') and without ('b0')"""
    f = ln_fwd(inp["x"], inp["gamma"], inp["beta"], eps)
    mean, rstd = f["mean"].float(), f["rstd"].float()
    b0 = ln_bwd(inp["dy"], inp["x"], mean, rstd, inp["gamma"])
    return {"f": f, "mean": mean, "rstd": rstd, "b0": b0, "bg": _with_gres(b0, inp["gres"], "dx")}


def ln_assertions(got, refs, inp, R, E, eps=LN_EPS, what=""):
    """every assertion on one LayerNorm case; got: {'f', 'bg', 'b0'} -> outputs as the kernels (or the emulation) return them.
    The fit of dx - gres on its three terms is made on the run without gres, where dx - gres is dx itself: the floors are those of
    rne(sum(terms)), and with gres the rounding of dx scales with |gres| as well, thirty times the terms on the rows with std 30."""
    out = _named("fwd ", fwd_assertions(got["f"], refs["f"], E, what=what))
    if R >= 4:
        out += _named("fwd ", const_row_assertions(got["f"], inp["beta"], eps, R - 2, what))
    out += _named("bwd gres ", bwd_assertions(got["bg"], refs["bg"], R, E, what=what + " gres"))
    out += _named("bwd ", bwd_assertions(got["b0"], refs["b0"], R, E, fit=ln_fit_runs(R, E), what=what + " no gres"))
    return out + _named("bwd ", gres_pair_assertions(got["bg"], got["b0"], inp["gres"], "dx", what))


def sln_refs(inp, T, eps=LN_EPS):
    a = (inp["h"], inp["w"], inp["lw"], inp["lb"], inp["gs"], inp["bs"])
    f = sln_fwd(*a, eps, T)
    mean, rstd = f["mean"].float(), f["rstd"].float()
    b = (inp["dy"], inp["h"], inp["w"], mean, rstd, inp["lw"], inp["lb"], inp["gs"], inp["bs"])
    b0 = sln_bwd(*b, None, T)
    return {"f": f, "mean": mean, "rstd": rstd, "b0": b0, "bg": _with_gres(b0, inp["gres"], "dh")}


def sln_assertions(got, refs, inp, R, E, what=""):
    """as ln_assertions for the SLN; got['bg'] may carry dw_start (dw_accumulate = 1 from that tensor)"""
    out = _named("sln fwd ", fwd_assertions(got["f"], refs["f"], E, sln=True, what=what))
    out += _named("sln bwd gres ", bwd_assertions(got["bg"], refs["bg"], R, E, sln=True, what=what + " gres"))
    out += _named("sln bwd ", bwd_assertions(got["b0"], refs["b0"], R, E, sln=True, fit=ln_fit_runs(R, E), what=what + " no gres"))
    return out + _named("sln bwd ", gres_pair_assertions(got["bg"], got["b0"], inp["gres"], "dh", what))


def ln_emulated(inp, refs, mut=None, eps=LN_EPS):
    """the float32 emulation of one LayerNorm case, with a planted mistake if asked"""
    fam = MUTANTS.get(mut)
    f = ln_fwd(inp["x"], inp["gamma"], inp["beta"], eps, mut if fam == "fwd" else None, F32)
    m = mut if fam == "bwd" else None
    a = (inp["dy"], inp["x"], refs["mean"], refs["rstd"], inp["gamma"])
    return {"f": to_kernel_outputs(f), "bg": to_kernel_outputs(ln_bwd(*a, inp["gres"], m, F32)), "b0": to_kernel_outputs(ln_bwd(*a, None, m, F32))}


def sln_emulated(inp, refs, T, mut=None, eps=LN_EPS):
    fam = MUTANTS.get(mut)
    f = sln_fwd(inp["h"], inp["w"], inp["lw"], inp["lb"], inp["gs"], inp["bs"], eps, T, mut if fam in ("fwd", "bcast") else None, F32)
    m = mut if fam in ("bwd", "sln_bwd", "bcast") else None
    b = (inp["dy"], inp["h"], inp["w"], refs["mean"], refs["rstd"], inp["lw"], inp["lb"], inp["gs"], inp["bs"])
    return {"f": to_kernel_outputs(f), "bg": to_kernel_outputs(sln_bwd(*b, inp["gres"], T, m, F32)), "b0": to_kernel_outputs(sln_bwd(*b, None, T, m, F32))}


def run_assertions(pairs, stats=None):
    """run every (name, thunk); returns the names that failed.  stats: worst ratio per name, kept as a running maximum"""
    failed = []
    for name, fn in pairs:
        try:
            v = fn()
            if stats is not None:
                stats[name] = max(stats.get(name, 0.0), v)
        except AssertionError as e:
            failed.append(f"{name}: {e}")
    return failed


def to_kernel_outputs(res):
    """what the kernel would hand back of a float32 evaluation: y, dx, dh rounded to bf16 (one RNE), the rest fp32"""
    assert all(v.dtype == F32 for v in res.values() if torch.is_tensor(v)), "the emulation left float32"
    return {k: (v.to(BF) if k in ("y", "dx", "dh") else v) for k, v in res.items() if torch.is_tensor(v)}


__all__ = [n for n in dir() if not n.startswith("_")]
