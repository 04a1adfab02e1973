"""float64 references and checkers for the second-order (gradient-penalty) kernels: a plain helper module, imported like exact_util.

Every operator has two independent forms: (a) torch autograd's double backward of the plain forward, and (b) the closed form of the
kernel headers (csrc/second_order.hip, vg_attn_bwd_bwd2_kernel in csrc/attention.hip) written term by term, so that each term can be
returned, dropped, re-signed or mis-scaled on its own.  tests/test_second_order_ref_cpu.py holds (a) == (b) to 1e-10 and shows that the
checkers below reject every defective closed form; tests/test_second_order_gpu.py holds the kernels to (b).

Next to every output the closed forms return ``mag``: the sum of the absolute values of the terms and products that make up the element
(the Sigma|ab| convention of the fp32-mode GEMM bound): an fp32 evaluation of depth kappa is within kappa * 2^-24 * mag of the exact value.
"""
import math

import torch
import torch.nn.functional as F

from exact_util import BF, rne

F64 = torch.float64
LN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------- checkers
def assert_elementwise(got, ref64, mag, kappa, what="", rel=2.0 ** -8):
    """every element within rel |ref| + kappa 2^-24 mag: one RNE bf16 rounding of the result (2^-9 |ref|; 2^-8 leaves room for the
    rounding boundary moving with the fp32 error) plus an fp32 evaluation of depth kappa.  rel = 0 for an fp32 output.  No element is
    excluded; a non-finite element fails."""
    got64 = got.detach().double().cpu()
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    lim = rel * ref64.abs() + kappa * 2.0 ** -24 * mag
    err = (got64 - ref64).abs()
    bad = ~(err <= lim)
    n = int(bad.sum())
    worst = float((err / lim.clamp_min(1e-300)).nan_to_num(posinf=0.0).max()) if err.numel() else 0.0
    if n:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside {rel:g} |ref| + {kappa} * 2^-24 * mag; first at {idx}: "
                             f"got {float(got64[idx])!r} want {float(ref64[idx])!r} (limit {float(lim[idx]):.3e}); worst err/limit {worst:.2f}")
    return worst


def fit_terms(got, terms):
    """least-squares coefficients of `got` on the fp64 terms (rows = the leading dimensions, the last one is the row).  Each row is
    first divided by the RMS of the rows' exact sum, so that no row outweighs the others by its scale (a LayerNorm row with a small
    variance has a thousand times the gradient of one with a large variance); rows whose exact sum is zero carry no information and
    are left out of the fit (they are still held elementwise)."""
    got64 = got.detach().double().cpu()
    tot = sum(terms)
    w = tot.pow(2).mean(-1, keepdim=True).sqrt()
    keep = (w > 0).expand_as(tot)
    w = torch.where(w > 0, 1.0 / w, torch.zeros_like(w))
    A = torch.stack([(t * w).expand_as(tot)[keep] for t in terms], 1)
    b = (got64 * w)[keep]
    return torch.linalg.lstsq(A, b.unsqueeze(1)).solution.squeeze(1)


def assert_fit(got, terms, bound, what=""):
    c = fit_terms(got, terms)
    dev = float((c - 1).abs().max())
    assert dev <= bound, f"{what}: fitted coefficients {[f'{float(v):.5f}' for v in c]} are not 1 within {bound:.2e}"
    return dev


def rel_rms(got, ref64):
    got64 = got.detach().double().cpu()
    return float(((got64 - ref64).pow(2).mean() / ref64.pow(2).mean().clamp_min(1e-300)).sqrt())


# -------------------------------------------------------------------------------------------------------------- activations
def act_funcs(kind, h):
    """f, f', f'' of gelu (exact erf) or tanh at a float64 h, with the magnitude sums of f' and f''"""
    h = h.double()
    if kind == "gelu":
        Phi = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
        Phi = torch.where(h < -1.0, 0.5 * torch.erfc(-h / math.sqrt(2.0)), Phi)  # no cancellation in the lower tail
        phi = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
        hphi = torch.where(phi == 0, torch.zeros_like(h), h * phi)
        h2phi = torch.where(phi == 0, torch.zeros_like(h), h * hphi)
        return h * Phi, Phi + hphi, 2.0 * phi - h2phi, Phi + hphi.abs(), 2.0 * phi + h2phi
    if kind == "tanh":
        t = torch.tanh(h)
        d1 = 1.0 / torch.cosh(h.clamp(-400, 400)) ** 2  # 1 - t^2 without the cancellation
        return t, d1, -2.0 * t * d1, d1, 2.0 * t.abs() * d1
    raise ValueError(kind)


def act_closed(kind, h, dy, u):
    """d_dy = u f'(h), d_h = u dy f''(h)"""
    _, d1, d2, m1, m2 = act_funcs(kind, h)
    u, dy = u.double(), dy.double()
    return {"d_dy": u * d1, "d_h": u * dy * d2, "mag_d_dy": u.abs() * m1, "mag_d_h": (u * dy).abs() * m2}


def act_autograd(kind, h, dy, u):
    """double backward of F.gelu / torch.tanh in float64"""
    fn = F.gelu if kind == "gelu" else torch.tanh
    h = h.double().clone().requires_grad_(True)
    dy = dy.double().clone().requires_grad_(True)
    (dh,) = torch.autograd.grad(fn(h), h, dy, create_graph=True)
    d_dy, d_h = torch.autograd.grad((dh * u.double()).sum(), (dy, h))
    return {"d_dy": d_dy, "d_h": d_h}


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_stats(x):
    """mean and rstd of the rows of a (bf16-valued) x in float64"""
    x = x.double()
    mu = x.mean(-1)
    var = (x - mu.unsqueeze(-1)).pow(2).mean(-1)
    return mu, 1.0 / torch.sqrt(var + LN_EPS)


LN_MUTANTS = ([f"drop_dx{k}" for k in range(4)] + [f"flip_dx{k}" for k in range(4)] + [f"drop_ddy{k}" for k in range(3)]
              + [f"flip_ddy{k}" for k in range(3)] + ["invE", "swap_means", "rstd"])
LN_GROSS = [m for m in LN_MUTANTS if m != "invE"]


def ln_closed(u, dy, x, mean, rstd, gamma, mut=None):
    """The double backward of LayerNorm in the decomposition of vg_ln_bwd_bwd_kernel's header.  mean / rstd are ARGUMENTS (the kernel
    reads them as fp32 tensors), so the forward's statistics are not part of what is checked.  With xh = (x - mu) r, g = dy gamma,
    b = mean(g xh), c = <u, g - mean(g) - xh b>:
      d_dy    = r gamma u  -  r gamma mean(u)  -  r gamma xh mean(u xh)                            (three terms)
      d_gamma = sum over rows of  r (u - mean(u) - xh mean(u xh)) dy
      d_x     = r dxh  -  r mean(dxh)  -  r xh mean(dxh xh)  -  r^2 xh c / E,   dxh = -r (g mean(u xh) + b u)   (four terms)
    mut: one of LN_MUTANTS - a defective form, for the mutation table."""
    u, dy, x, gamma = u.double(), dy.double(), x.double(), gamma.double()
    E = x.shape[-1]
    r = rstd.double().unsqueeze(-1)
    xh = (x - mean.double().unsqueeze(-1)) * r
    g = dy * gamma
    m = lambda t: t.mean(-1, keepdim=True)  # noqa: E731
    m_u, m_ux, a, b = m(u), m(u * xh), m(g), m(g * xh)
    M_u, M_ux, A_, B_ = m(u.abs()), m((u * xh).abs()), m(g.abs()), m((g * xh).abs())
    ddy_ux = b if mut == "swap_means" else m_ux
    ddy_terms = [r * gamma * u, -r * gamma * m_u, -r * gamma * xh * ddy_ux]
    mag_dg = r * (u.abs() + M_u + xh.abs() * M_ux)
    dg = r * (u - m_u - xh * m_ux)
    c = (u * (g - a - xh * b)).sum(-1, keepdim=True)
    C_ = (u.abs() * (g.abs() + A_ + xh.abs() * B_)).sum(-1, keepdim=True)
    dxh = -r * (g * b + m_ux * u) if mut == "swap_means" else -r * (g * m_ux + b * u)
    mag_dxh = r * (g.abs() * M_ux + B_ * u.abs())
    inv_e = 1.0 / (E - 1) if mut == "invE" else 1.0 / E
    r2 = r if mut == "rstd" else r * r
    dx_terms = [r * dxh, -r * m(dxh), -r * xh * m(dxh * xh), -r2 * xh * c * inv_e]
    mag_dx = r * mag_dxh + r * m(mag_dxh) + r * xh.abs() * m(mag_dxh * xh.abs()) + r * r * xh.abs() * C_ / E
    for name, terms in (("dx", dx_terms), ("ddy", ddy_terms)):
        if mut and mut[:-1] in (f"drop_{name}", f"flip_{name}"):
            k = int(mut[-1])
            terms[k] = terms[k] * (0.0 if mut.startswith("drop") else -1.0)
    return {"d_dy": sum(ddy_terms), "d_dy_terms": ddy_terms, "mag_d_dy": mag_dg * gamma.abs(),
            "d_x": sum(dx_terms), "d_x_terms": dx_terms, "mag_d_x": mag_dx,
            "d_gamma": (dg * dy).sum(0), "mag_d_gamma": (mag_dg * dy.abs()).sum(0)}


def ln_autograd(u, dy, x, gamma):
    """double backward of F.layer_norm (eps 1e-5) in float64: gradients of <u, dx> with respect to dy, x and gamma"""
    E = x.shape[-1]
    x = x.double().clone().requires_grad_(True)
    dy = dy.double().clone().requires_grad_(True)
    gamma = gamma.double().clone().requires_grad_(True)
    y = F.layer_norm(x, (E,), gamma, torch.zeros(E, dtype=F64), LN_EPS)
    (dx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    d_dy, d_x, d_gamma = torch.autograd.grad((dx * u.double()).sum(), (dy, x, gamma))
    return {"d_dy": d_dy, "d_x": d_x, "d_gamma": d_gamma}


def ln_kappa(E):
    """dependent fp32 operations on the longest path of vg_ln_bwd_bwd_kernel to one element of d_x: three chained row sums
    (mean(u xh) -> dxh -> mean(dxh xh) -> d_x; c is a fourth, in parallel with the second), each E/64 serial adds in a lane + 6 shuffle
    levels, and 10 elementwise operations (x - mu, * r, dy gamma, the products inside the sums, * invE, the four-term combination)."""
    return 3 * (E // 64 + 6) + 10


def ln_kappa_gamma(E, R):
    """d_gamma: one row sum + 5 elementwise operations for d_g dy, then the serial sum over the rows of one wave (trips of the grid-stride
    loop), 2 levels over the workgroup's four waves, and vg_colsum_f32's fold: ceil(parts / 16) serial adds + 16"""
    parts = min((R + 3) // 4, 2048)
    trips = -(-R // (4 * parts))
    return (E // 64 + 6) + 5 + trips + 2 + -(-parts // 16) + 16


def ln_inputs(R, E, seed):
    """(u, dy, x, gamma) as bf16-valued float64 (gamma fp32-valued).  Rows of mixed character inside one launch: most N(0.2, 1.3); every
    8th row (5 mod 8) mean 8 and std 2^-5; every 8th (6 mod 8) std 30; with R >= 4 one constant row (variance 0: rstd = eps^-1/2) and one
    row that is a single spike.  gamma ~ 1 + 0.3 N with two exact zeros."""
    g = torch.Generator().manual_seed(seed * 1000003 + R * 1031 + E)
    x = torch.randn(R, E, generator=g, dtype=F64) * 1.3 + 0.2
    rows = torch.arange(R)
    tight, wide = rows % 8 == 5, rows % 8 == 6
    x[tight] = 8.0 + (x[tight] - 0.2) / 1.3 * 2.0 ** -5
    x[wide] = (x[wide] - 0.2) / 1.3 * 30.0
    if R >= 4:
        x[R - 2] = 1.25
        x[R - 1] = 0.0
        x[R - 1, (7 * R) % E] = 24.0
    u = torch.randn(R, E, generator=g, dtype=F64)
    dy = torch.randn(R, E, generator=g, dtype=F64)
    gamma = 1.0 + 0.3 * torch.randn(E, generator=g, dtype=F64)
    gamma[3] = 0.0
    gamma[E - 2] = 0.0
    bf = lambda t: t.to(BF).double()  # noqa: E731
    return bf(u), bf(dy), bf(x), gamma.float().double()


# bounds on |c - 1| of fit_terms for the LayerNorm outputs: 4 x the floor of rne(sum(terms), bf16), largest of 16 seeds, as measured by
# tests/test_second_order_ref_cpu.py::test_layernorm_fit_floor (which prints the floors and asserts 4 x floor <= these)
LN_FIT_ROWS_NARROW, LN_FIT_ROWS_WIDE = 1040, 8192   # least R for the fit at E <= 512 and above


def ln_fit_runs(R, E):
    return R >= (LN_FIT_ROWS_NARROW if E <= 512 else LN_FIT_ROWS_WIDE)


# measured floors (d_x and d_dy together, 16 seeds, ln_inputs): {E: floor at R = 8192} and {E: floor at R = 1040}
_LN_FLOOR_8192 = {128: 6.9e-5, 256: 5.5e-5, 384: 6.9e-5, 512: 5.4e-5, 640: 4.9e-5, 768: 5.1e-5, 896: 4.6e-5, 1024: 5.5e-5}
_LN_FLOOR_1040 = {384: 1.63e-4, 512: 1.24e-4}


def ln_fit_bound(R, E):
    """4 x the measured floor of the shape's class: R >= 8192 uses the R = 8192 floor (more rows only lower it), 1040 <= R < 8192 the
    R = 1040 one"""
    assert ln_fit_runs(R, E)
    return 4.0 * (_LN_FLOOR_8192[E] if R >= 8192 else _LN_FLOOR_1040[E])


# ---------------------------------------------------------------------------------------------------------------- attention
ATTN_MUTANTS = ["scale_dq_twice", "scale_dq_never", "scale_dk_twice", "scale_dk_never", "drop_gam_dp", "mask_off_by_one", "lse_next_head"]


def attn_lse(q, k, scale):
    return torch.logsumexp(scale * (q.double() @ k.double().transpose(-1, -2)), -1)


def attn_closed(q, k, v, d_o, uq, uk, uv, lse, scale, bf16_operands=False, dtype=F64, mut=None):
    """The double backward of softmax attention, all tensors [B, H, S, HE], lse [B, H, S] an ARGUMENT, in the kernel header's
    decomposition (G, gam, H, Pi, pi, Sg).  bf16_operands: P, H, dS, Sg are rounded to bf16 before the output products, which is
    where the kernel rounds them (its S x S matrices enter the MFMA as bf16).  dtype: the precision everything is evaluated in."""
    q, k, v, d_o, uq, uk, uv = (t.to(dtype) for t in (q, k, v, d_o, uq, uk, uv))
    lse = lse.to(dtype)
    S = q.shape[-2]
    if mut == "lse_next_head":
        lse = lse.roll(1, 1)
    if mut == "mask_off_by_one":   # row S of the buffer - the first token of the following image - takes part as a key
        pad = lambda t: torch.cat([t, t[..., :1, :].roll(-1, 0)], -2)  # noqa: E731
        k, v, uk, uv = pad(k), pad(v), pad(uk), pad(uv)
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    rs = lambda t: t.sum(-1, keepdim=True)  # noqa: E731
    P = torch.exp(scale * (q @ T(k)) - lse.unsqueeze(-1))
    dP = d_o @ T(v)
    delta = rs(P * dP)
    A = dP - delta
    G = scale * (uq @ T(k) + q @ T(uk))
    gam = rs(G * P)
    Hm = P * (G - gam)
    Pi = d_o @ T(uv) + G * A - (0.0 if mut == "drop_gam_dp" else gam * dP)
    pi = rs(P * Pi)
    Sg = P * (Pi - pi)
    dS = P * A
    inter = {"G": G, "gam": gam, "H": Hm, "Pi": Pi, "pi": pi, "Sg": Sg, "P": P, "dS": dS}
    if bf16_operands:
        P, Hm, dS, Sg = (t.to(BF).to(dtype) for t in (P, Hm, dS, Sg))
    sq = {"scale_dq_twice": scale * scale, "scale_dq_never": 1.0}.get(mut, scale)
    sk = {"scale_dk_twice": scale * scale, "scale_dk_never": 1.0}.get(mut, scale)
    ddo_terms = [P @ uv, Hm @ v]
    dq_terms = [sq * (dS @ uk), sq * (Sg @ k)]
    dk_terms = [(sk * (T(dS) @ uq))[..., :S, :], (sk * (T(Sg) @ q))[..., :S, :]]
    dv = (T(Hm) @ d_o)[..., :S, :]
    # magnitude sums through every cancellation (Sigma|ab|): what an fp32 evaluation, or a perturbed P, can move the result by
    a = torch.abs
    adP = a(d_o) @ T(a(v))
    aA = adP + rs(P * adP)
    aG = abs(scale) * (a(uq) @ T(a(k)) + a(q) @ T(a(uk)))
    aGam = rs(aG * P)
    aH = P * (aG + aGam)
    aPi = a(d_o) @ T(a(uv)) + aG * aA + aGam * adP
    aSg = P * (aPi + rs(P * aPi))
    adS = P * aA
    return {"d_do": sum(ddo_terms), "d_do_terms": ddo_terms, "mag_d_do": P @ a(uv) + aH @ a(v),
            "d_q": sum(dq_terms), "d_q_terms": dq_terms, "mag_d_q": abs(sq) * (adS @ a(uk) + aSg @ a(k)),
            "d_k": sum(dk_terms), "d_k_terms": dk_terms, "mag_d_k": (abs(sk) * (T(adS) @ a(uq) + T(aSg) @ a(q)))[..., :S, :],
            "d_v": dv, "mag_d_v": (T(aH) @ a(d_o))[..., :S, :], **inter}


def attn_autograd(q, k, v, d_o, uq, uk, uv, scale):
    """double backward of softmax(scale q k^T) v in float64"""
    q, k, v, d_o = (t.double().clone().requires_grad_(True) for t in (q, k, v, d_o))
    o = torch.softmax(scale * (q @ k.transpose(-1, -2)), -1) @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o, create_graph=True)
    L = (dq * uq.double()).sum() + (dk * uk.double()).sum() + (dv * uv.double()).sum()
    d_do, d_q, d_k, d_v = torch.autograd.grad(L, (d_o, q, k, v))
    return {"d_do": d_do, "d_q": d_q, "d_k": d_k, "d_v": d_v}


def attn_inputs(B, H, S, HE, seed):
    """random bf16-valued q, k, v, d_o, uq, uk, uv [B, H, S, HE] (float64) with head- and image-dependent scales, so that a head or
    image mix-up changes the result"""
    g = torch.Generator().manual_seed(seed * 7919 + S * 131 + HE + 17 * B + H)
    amp = 0.75 + 0.5 * torch.rand(7, B, H, 1, 1, generator=g, dtype=F64)
    ts = [(torch.randn(B, H, S, HE, generator=g, dtype=F64) * amp[i]).to(BF).double() for i in range(7)]
    return ts


def heads_to_rows(t):
    """[B, H, S, HE] -> [B*S, H*HE] (the kernels' row layout)"""
    B, H, S, HE = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * HE)


def rows_to_heads(t, B, H, S, HE):
    return t.reshape(B, S, H, HE).permute(0, 2, 1, 3)


ATTN_OUTPUTS = ("d_do", "d_q", "d_k", "d_v")
ATTN_FIT_OUTPUTS = ("d_do", "d_q", "d_k")
# 4 x the floors of tests/test_second_order_ref_cpu.py::test_attention_floors (reference against reference, worst of 16 seeds, every
# tested S, HE = 32 / 64 / 96).  With one key (S = 1) the second term of every output is exactly zero: nothing to fit.
ATTN_FIT_MIN_S = 2
ATTN_RMS_BOUND = 4 * 1.76e-3   # floors 1.75e-3 / 1.72e-3 / 1.74e-3: almost all of it is the output's own bf16 rounding
ATTN_FIT_BOUND = 4 * 1.64e-4   # floors 1.63e-4 / 1.23e-4 / 1.13e-4


def attn_simulated(inp, lse, scale, mut=None):
    """what a kernel that rounds where vg_attn_bwd_bwd2_kernel rounds would return, from a float32 evaluation: bf16 tensors"""
    r = attn_closed(*inp, lse, scale, bf16_operands=True, dtype=torch.float32, mut=mut)
    return {n: r[n].to(BF) for n in ATTN_OUTPUTS}


__all__ = [n for n in dir() if not n.startswith("_")] + ["rne"]
