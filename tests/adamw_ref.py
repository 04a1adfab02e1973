"""One AdamW step in float64 on an explicit state (p, m, v, g, t): the reference the optimizer kernels are held to.

torch.optim.AdamW semantics (decoupled weight decay before the moments):
    g *= gscale;  p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
    p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc_i = 1 - b_i^t.
The bias corrections are formed as -expm1(t * log1p(-(1 - b))), which does not cancel at small t.

A kernel receives its hyperparameters as float32: pass them through ``f32`` first (0.999f differs from 0.999 by 1.3e-8,
which moves 1 - b2 by 1.3e-5 relative - far more than any bound on v below could absorb).
"""
import math

import numpy as np
import torch


def f32(x: float) -> float:
    """The float32 value a kernel receives for the host value x, widened to float64."""
    return float(np.float32(x))


def bias_correction(b: float, t: int) -> float:
    """1 - b^t in float64 without cancellation."""
    return -math.expm1(t * math.log1p(-(1.0 - b)))


def adamw_step(p, m, v, g, t: int, lr: float, b1: float, b2: float, eps: float, wd: float, gscale: float = 1.0):
    """(p1, m1, v1) as float64 tensors after one AdamW step at step count t (t >= 1; m, v are the moments after step t-1)."""
    p, m, v, g = (torch.as_tensor(a).detach().to(torch.float64) for a in (p, m, v, g))
    g = g * gscale
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = bias_correction(b1, t), bias_correction(b2, t)
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def ulp32(x) -> torch.Tensor:
    """Spacing of float32 at |x| (float64 tensor on x's device): one unit in the last place of x's float32 neighbourhood."""
    a = torch.as_tensor(x).detach().abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(torch.float64)


TINY = float(np.finfo(np.float32).tiny)  # smallest normal float32: the absolute floor of the moment bounds
UPD_REL = 2.0 ** -12


def check_adamw_step(p0, m0, v0, g, t: int, hyper, gscale: float, P, M, V, SH, what: str = ""):
    """Every element of a kernel's result (P, M, V fp32, SH bf16) of one step from (p0, m0, v0, g) at step count t, against
    ``adamw_step`` in float64 with the hyperparameters ``hyper = (lr, b1, b2, eps, wd)`` and ``gscale`` as the kernel receives them
    (rounded to float32 here).  Bounds:
      m1, v1: 2^-20 relative per element, the smallest normal float32 as an absolute floor; m's scale is the magnitude of its two
              terms b1|m0| + (1-b1)|g| (they may cancel), v's terms are never negative;
      p1:     |p1 - p_ref| <= 2^-12 |p_ref - p0| + 2 ulp32(p_ref), where p_ref is the float64 step from p0 with the kernel's own m1, v1
              (themselves held to the reference above).  Where m's two terms cancel, m1 carries an fp32 rounding error of 2^-24 of the
              terms, which can be many times 2^-12 of the small m1 - and of the small update it makes (seen on an engine trajectory:
              |m1| ~ 1e-5 of its terms, the update 4 x 2^-12 off for that reason alone).  No fp32 kernel avoids that; everything
              else the update computes (decay, bias corrections, step size, denominator) must stay within 2^-12;
      SH:     bit-equal to the round-to-nearest-even of the kernel's own P.
    Works on any device (all tensors on one).  Returns (worst error as a fraction of the p1 bound, worst update error as a fraction
    of 2^-12 |p_ref - p0| over the elements whose update exceeds 2^16 ulp, where the ulp term does not hide it)."""
    lr, b1, b2, eps, wd = (f32(x) for x in hyper)
    gs = f32(gscale)
    _, m_ref, v_ref = adamw_step(p0, m0, v0, g, t, lr, b1, b2, eps, wd, gs)
    P, M, V = (x.detach() for x in (P, M, V))
    assert bool(torch.isfinite(P).all() and torch.isfinite(M).all() and torch.isfinite(V).all()), f"{what}: non-finite result"
    gg = g.detach().double() * gs
    m_scale = b1 * m0.detach().double().abs() + (1 - b1) * gg.abs()
    m_err = (M.double() - m_ref).abs()
    bad = m_err > 2.0 ** -20 * m_scale + TINY
    assert not bool(bad.any()), f"{what}: m off at {int(bad.sum())} elements, worst {float((m_err / (m_scale + TINY)).max()):.3e} relative"
    v_err = (V.double() - v_ref).abs()
    bad = v_err > 2.0 ** -20 * v_ref.abs() + TINY
    assert not bool(bad.any()), f"{what}: v off at {int(bad.sum())} elements, worst {float((v_err / (v_ref.abs() + TINY)).max()):.3e} relative"
    p0d = p0.detach().double()
    p_ref = p0d * (1.0 - lr * wd) - (lr / bias_correction(b1, t)) * M.double() / (V.double().sqrt() / math.sqrt(bias_correction(b2, t)) + eps)
    upd = (p_ref - p0d).abs()
    ulp = ulp32(p_ref)
    err = (P.double() - p_ref).abs()
    bound = UPD_REL * upd + 2 * ulp
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: p off at {int(bad.sum())} elements, worst {float((err / bound).max()):.3f} of the bound (element {i}: "
                             f"p0 {float(p0[i]):.9e} got {float(P[i]):.9e} want {float(p_ref[i]):.9e})")
    sh_bad = SH.detach().view(torch.int16) != P.to(torch.bfloat16).view(torch.int16)
    assert not bool(sh_bad.any()), f"{what}: bf16 shadow != RNE(master) at {int(sh_bad.sum())} elements"
    clean = upd > 2.0 ** 16 * ulp
    frac_upd = float((err[clean] / (UPD_REL * upd[clean])).max()) if bool(clean.any()) else 0.0
    return float((err / bound).max()), frac_upd
