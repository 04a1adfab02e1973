"""The differentiable augmentation (include/vitgan_hip.h, vg_diffaug_fwd / vg_diffaug_bwd) restated off the device: a plain helper
module, imported like exact_util.

Two independent pieces:
  * ``draw``: the parameter function in numpy, 32-bit arithmetic behind the 64-bit host key, written from the header's text.  The
    kernels' ``params_out`` must equal it bit for bit.
  * ``augment`` / ``adjoint``: the operator as the issue composes it - brightness, saturation, contrast, translation, cutout, one after
    the other - and its hand-written adjoint, in torch at any float dtype (float64 is the reference), taking EXPLICIT parameters
    [B, 8] = (b, s, k, tx, ty, cx, cy, policy).  A member that is off carries its identity (b = 0, s = k = 1, tx = ty = 0, cx = cy = -IH),
    so the parameters alone fix the transform.  ``augment`` is differentiable by autograd, which is how the adjoint is checked.
Both return ``mag`` next to the value: the sum of the magnitudes of everything that is added or subtracted on the way to an element
(second_order_ref's convention), so that an fp32 evaluation of depth kappa lies within kappa * 2^-24 * mag.
"""
import numpy as np
import torch

from drop_ref import h, site_key, step_mix  # noqa: F401  (the host key, the counter hash and the step mix of the dropout masks)


# ------------------------------------------------------------------------------------------------------------- parameters
def k24(seed, site, step, n, p):
    """the 24-bit value of parameter p for image n at step counter ``step`` (None: no device counter); step and n broadcast"""
    ks = h(step_mix(site_key(seed, site), step), 0)
    kn = h(ks, n)
    return h(kn, p).astype(np.uint64) >> np.uint64(8)


def draw(seed, site, step, B, IH, policy):
    """float32 [B, 8]: what vg_diffaug_fwd writes to params_out"""
    n = np.arange(B)
    u = lambda p: k24(seed, site, step, n, p).astype(np.float64) * 2.0 ** -24  # noqa: E731  (exact: 24 bits)
    I = lambda p, m: (k24(seed, site, step, n, p) * np.uint64(m)) >> np.uint64(24)  # noqa: E731,E741
    out = np.zeros((B, 8), dtype=np.float64)
    out[:, 1] = out[:, 2] = 1.0
    out[:, 5] = out[:, 6] = -IH
    out[:, 7] = policy
    if policy & 1:
        out[:, 0], out[:, 1], out[:, 2] = u(0) - 0.5, 2.0 * u(1), u(2) + 0.5
    if policy & 2:
        r = IH // 8
        out[:, 3] = I(3, 2 * r + 1).astype(np.int64) - r
        out[:, 4] = I(4, 2 * r + 1).astype(np.int64) - r
    if policy & 4:
        out[:, 5], out[:, 6] = I(5, IH + 1), I(6, IH + 1)
    f = out.astype(np.float32)  # u2 + 0.5 needs 25 bits above 1: the one fp32 addition rounds to nearest even, here as on the device
    exact = [i for i in range(8) if i != 2]
    assert (f[:, exact].astype(np.float64) == out[:, exact]).all()  # every other parameter is exactly representable
    return f


# --------------------------------------------------------------------------------------------------------------- operator
def _shift(x, ty, tx):
    """out[n, c, i, j] = x[n, c, i - ty[n], j - tx[n]], zero outside the frame"""
    B, _, IH, _ = x.shape
    ar = torch.arange(IH)
    si, sj = ar[None, :] - ty[:, None], ar[None, :] - tx[:, None]                   # [B, IH]
    ok = (((si >= 0) & (si < IH))[:, :, None] & ((sj >= 0) & (sj < IH))[:, None, :])  # [B, IH, IH]
    g = x[torch.arange(B)[:, None, None], :, si.clamp(0, IH - 1)[:, :, None], sj.clamp(0, IH - 1)[:, None, :]]  # [B, IH, IH, C]
    return g.permute(0, 3, 1, 2) * ok[:, None].to(x.dtype)


def _cut_mask(params, IH):
    """[B, 1, IH, IH] bool: True inside the cutout square"""
    cx, cy = params[:, 5].long(), params[:, 6].long()
    ar = torch.arange(IH)
    r0, c0 = cy - IH // 4, cx - IH // 4
    rows = (ar[None, :] >= r0[:, None]) & (ar[None, :] < (r0 + IH // 2)[:, None])
    cols = (ar[None, :] >= c0[:, None]) & (ar[None, :] < (c0 + IH // 2)[:, None])
    return (rows[:, :, None] & cols[:, None, :])[:, None]


def _pp(params, dtype):
    params = torch.as_tensor(params)
    b, s, k = (params[:, i].to(dtype).reshape(-1, 1, 1, 1) for i in range(3))
    return params, b, s, k, params[:, 3].long(), params[:, 4].long()


def augment(x, params, dtype=torch.float64):
    """T x and its magnitude sum; x [B, C, IH, IH] (cpu), params [B, 8]"""
    params, b, s, k, tx, ty = _pp(params, dtype)
    x = x.to(dtype)
    IH = x.shape[-1]
    x1, g1 = x + b, x.abs() + b.abs()                                         # brightness
    m, gm = x1.mean(1, keepdim=True), g1.mean(1, keepdim=True)
    x2, g2 = m + s * (x1 - m), gm + s.abs() * (g1 + gm)                       # saturation
    M, gM = x2.mean((1, 2, 3), keepdim=True), g2.mean((1, 2, 3), keepdim=True)
    x3, g3 = M + k * (x2 - M), gM + k.abs() * (g2 + gM)                       # contrast
    x4, g4 = _shift(x3, ty, tx), _shift(g3, ty, tx)                           # translation
    keep = (~_cut_mask(params, IH)).to(dtype)                                 # cutout
    return x4 * keep, g4 * keep


def adjoint(dy, params, dtype=torch.float64):
    """T^T dy (the linear part's transpose; the brightness is a constant and drops out) and its magnitude sum"""
    params, b, s, k, tx, ty = _pp(params, dtype)
    dy = dy.to(dtype)
    IH = dy.shape[-1]
    keep = (~_cut_mask(params, IH)).to(dtype)
    g, gg = _shift(dy * keep, -ty, -tx), _shift(dy.abs() * keep, -ty, -tx)    # mask by the cutout, shift back with zero fill
    hh = k * g + (1 - k) * g.mean((1, 2, 3), keepdim=True)
    gh = k.abs() * gg + (1 - k).abs() * gg.mean((1, 2, 3), keepdim=True)
    return s * hh + (1 - s) * hh.mean(1, keepdim=True), s.abs() * gh + (1 - s).abs() * gh.mean(1, keepdim=True)


def live_mask(params, IH):
    """[B, 1, IH, IH] bool: output pixels that carry a value (source inside the frame, outside the cutout); the rest is exactly 0"""
    params = torch.as_tensor(params)
    ones = torch.ones(params.shape[0], 1, IH, IH, dtype=torch.float64)
    return (_shift(ones, params[:, 4].long(), params[:, 3].long()) > 0) & ~_cut_mask(params, IH)


# ------------------------------------------------------------------------------------------------------------ error bound
def threads(IH):
    """workgroup size of the kernels (vg_aug_threads): one thread per chunk of 8 pixels of a plane, whole waves, 64 to 1024"""
    nch = (IH * IH + 7) // 8
    return min(1024, max(64, (nch + 63) // 64 * 64))


def kappa(C, IH):
    """Depth of the fp32 evaluation the kernels perform, for ``assert_elementwise``'s kappa * 2^-24 * mag - derived from the code
    as written (csrc/augment.hip), the way DESIGN's second-order table does it for LayerNorm:
      image mean   8 elements of a chunk pairwise (3), then the thread's chunks and channels one after the other
                   (C * ceil(chunks / NT) additions), the 64 lanes by a butterfly (6), the NT / 64 waves one after the other,
                   the product with the rounded 1 / (C IH IH) (2)
      pixel mean   C additions, the product with the rounded 1 / C (2)
      element      forward (Mx + b) + k ((mx - Mx) + s (g - mx)): 7 operations; adjoint k (s g + (1 - s) mx) + (1 - k) Mx: 8, one
                   more when it accumulates: 9 covers both
    Every term's error is at most (its own depth) * 2^-24 * (its magnitude), so the sum of the depths times the whole magnitude sum
    bounds the element.  The kernels work on the collapsed affine form, whose magnitude sum is term by term no larger than the
    ``mag`` of the member-by-member composition above (which counts the brightness once per subtraction it passes)."""
    nt = threads(IH)
    chunks = (IH * IH + 7) // 8
    trips = (chunks + nt - 1) // nt
    return (3 + C * trips + 6 + nt // 64 + 2) + (C + 2) + 9
