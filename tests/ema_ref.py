"""The exponential moving average of the generator's weights in float64: the reference vg_adamw_ema_step / vg_ema_update are held to.

With t the 1-based step count, p_t the fp32 master after step t, d the decay and k = max(1, start):
    e_t = p_t                                   for t <= k   (the average follows the weights through the warm-up; the FIRST step
                                                              always copies, whatever the buffer held)
    e_t = e_{t-1} + (1 - d) (p_t - e_{t-1})     for t >  k.
A kernel receives d as float32: pass it through ``f32`` first (0.999f differs from 0.999 by 1.3e-8, 1.3e-5 of 1 - d).
"""
import numpy as np
import torch

from adamw_ref import f32, ulp32


def copies(t: int, start: int) -> bool:
    """True on the steps whose average is a copy of the weights."""
    return t <= max(1, start)


def ema_step(e0, p1, t: int, decay: float, start: int):
    """e_t (float64 tensor) from e_{t-1} = e0 and the updated weights p1 at step count t."""
    p1 = torch.as_tensor(p1).detach().to(torch.float64)
    if copies(t, start):
        return p1.clone()
    e0 = torch.as_tensor(e0).detach().to(torch.float64)
    return e0 + (1.0 - decay) * (p1 - e0)


def ema_bound(e0, P, e_ref, decay: float):
    """The per-step error bound of the fp32 form ``fmaf(1 - d, P - e0, e0)`` against ``e_ref`` (see check_ema_step)."""
    return ulp32(e_ref) + 2.0 ** -22 * (1.0 - decay) * (P.detach().double() - e0.detach().double()).abs()


def check_ema_step(e0, P, t: int, decay: float, start: int, E, what: str = ""):
    """Every element of a kernel's average E (fp32) after step t, from its previous value e0 and the kernel's OWN updated fp32 weights P.

    Where the step copies (t <= max(1, start)) E must be bit-equal to P.  Elsewhere, with d = f32(decay),
        e_ref = e0 + (1 - d)(P - e0)   in float64,      |E - e_ref| <= ulp32(e_ref) + 2^-22 (1 - d) |P - e0|.
    Derivation: the specified fp32 form is fmaf(1 - d, P - e0, e0), with 1 - d exact in fp32 for d in [0.5, 1) (and within 2^-24
    relative below).  It rounds twice: the subtraction P - e0 is off by at most 2^-24 of its own result, which the product turns
    into 2^-24 (1 - d)|P - e0|; the fma rounds once, at most half an ulp of the result.  The bound gives the first a factor of
    four (2^-22) - it also absorbs the rounding of 1 - d for d < 0.5 - and the second a factor of two (one ulp, taken at e_ref,
    which may sit one binade below the result's).  Nothing else is allowed: a form that rounds the product separately, or blends with
    d and 1 - d swapped, leaves the bound.
    Returns the worst error as a fraction of the bound (0.0 on a copying step)."""
    e0, P, E = (x.detach() for x in (e0, P, E))
    assert bool(torch.isfinite(E).all()), f"{what}: non-finite average"
    if copies(t, start):
        bad = E.view(torch.int32) != P.view(torch.int32)
        assert not bool(bad.any()), f"{what}: step {t} <= max(1, {start}) must copy the weights; {int(bad.sum())} elements differ"
        return 0.0
    d = f32(decay)
    e_ref = ema_step(e0, P, t, d, start)
    err = (E.double() - e_ref).abs()
    bound = ema_bound(e0, P, e_ref, d)
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: average off at {int(bad.sum())} elements, worst {float((err / bound).max()):.3f} of the bound (element {i}: "
                             f"e0 {float(e0.reshape(-1)[i]):.9e} p {float(P.reshape(-1)[i]):.9e} got {float(E.reshape(-1)[i]):.9e} "
                             f"want {float(e_ref.reshape(-1)[i]):.9e})")
    return float((err / bound).max())


def ema_trajectory(masters, decay: float, start: int):
    """(e_N, allowed error) in float64 for the masters p_1..p_N (fp32 tensors, masters[t-1] after step t): the recursion above with
    d = f32(decay), and the SUM of the per-step bounds of check_ema_step taken along it.  An error made at step t is multiplied by d
    at every later step (e_t depends on e_{t-1} with factor d < 1), so the plain sum is an upper bound of what can have accumulated."""
    d = f32(decay)
    e = None
    allowed = torch.zeros_like(masters[0], dtype=torch.float64)
    for t, p in enumerate(masters, start=1):
        if copies(t, start):
            e = p.detach().double().clone()
            allowed.zero_()  # a copy is exact and forgets what came before
        else:
            e1 = ema_step(e, p, t, d, start)
            allowed += ulp32(e1) + 2.0 ** -22 * (1.0 - d) * (p.detach().double() - e).abs()
            e = e1
    return e, allowed


def check_ema_trajectory(masters, decay: float, start: int, E, what: str = ""):
    """The engine's average E after N steps against ``ema_trajectory`` of the masters it wrote.  Returns the worst fraction of the bound."""
    e_ref, allowed = ema_trajectory(masters, decay, start)
    E = E.detach()
    assert bool(torch.isfinite(E).all()), f"{what}: non-finite average"
    err = (E.double() - e_ref).abs()
    if copies(len(masters), start):
        assert torch.equal(E, masters[-1]), f"{what}: the last step copies, the average must equal the master bitwise"
        return 0.0
    bad = err > allowed
    assert not bool(bad.any()), (f"{what}: average off at {int(bad.sum())} elements after {len(masters)} steps, worst "
                                 f"{float((err / allowed.clamp_min(1e-300)).max()):.3f} of the summed bound")
    return float((err / allowed.clamp_min(1e-300)).max())


def ema_f32_emulation(e0, p1, t: int, decay: float, start: int, copy_rule=copies, swap: bool = False):
    """numpy-float32 emulation of the specified expression (the fma as one rounding of the float64 value - the product of two
    float32 is exact in float64, and the sum's double rounding is far below the bound).  ``copy_rule`` / ``swap`` plant mistakes."""
    e0 = np.asarray(e0, dtype=np.float32)
    p1 = np.asarray(p1, dtype=np.float32)
    if copy_rule(t, start):
        return p1.copy()
    d = np.float32(decay)
    w = d if swap else np.float32(1) - d
    diff = (p1 - e0).astype(np.float32)
    return (np.float64(w) * diff.astype(np.float64) + e0.astype(np.float64)).astype(np.float32)
