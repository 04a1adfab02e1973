"""Balanced consistency regularisation (include/vitgan_hip.h, vg_bcr_loss) restated off the device: a plain helper module, imported
like diffaug_ref.

  * ``consistency``: the definition in torch float64 - the two unweighted segment means, both gradients, the accumulate semantics -
    with, next to every value, ``mag``: the magnitude the fp32 error of that value is relative to (second_order_ref's convention, for
    ``assert_elementwise``'s kappa * 2^-24 * mag).
  * ``emulate32``: the kernel's operation order (csrc/elementwise.hip, vg_bcr_loss_body) in numpy float32, one rounding per operation;
    ``mistake`` plants one of four errors a wrong kernel could make.
  * ``kappa_grad`` / ``kappa_loss``: the depth of that evaluation, counted from the kernel as written.
"""
import numpy as np
import torch

F64 = torch.float64
NT = 256  # threads of a workgroup: one workgroup per segment


def _segments(n, n_real):
    return (slice(0, n_real), slice(n_real, n))


def consistency(lx, la, n_real, w_real, w_fake, grad_scale=1.0, into_x=None, into_a=None):
    """lx, la [n, Kc] (any float dtype, taken as exact): the logits on x and on T(x); rows [0, n_real) are the real segment.
    Returns a dict of float64 tensors:
      loss [2], loss_mag [2]      L_s = 1/B_s sum_{n in s} sum_k (lx - la)^2, the mean over the IMAGES of a segment
      gx, ga [n, Kc]              gx = (into_x +) g, ga = (into_a -) g with g = (2 w_s / B_s) grad_scale (lx - la); a zero weight leaves
                                  the target as it was (accumulate) or gives 0 (overwrite)
      gx_mag, ga_mag              |g| (+ |into|): the kernel forms lx - la from the given fp32 values, so its error is relative to the
                                  difference itself, not to |lx| + |la|"""
    lx, la = torch.as_tensor(lx).detach().to(F64), torch.as_tensor(la).detach().to(F64)
    n = lx.shape[0]
    d = lx - la
    loss = torch.zeros(2, dtype=F64)
    g = torch.zeros_like(d)
    for s, (sl, w) in enumerate(zip(_segments(n, n_real), (w_real, w_fake))):
        nb = sl.stop - sl.start
        loss[s] = d[sl].pow(2).sum() / nb
        g[sl] = (2.0 * float(w) / nb) * float(grad_scale) * d[sl]
    out = {"loss": loss, "loss_mag": loss.clone()}  # a sum of non-negative terms: its magnitude sum is the value
    for name, into, sign in (("gx", into_x, 1.0), ("ga", into_a, -1.0)):
        base = torch.zeros_like(g) if into is None else torch.as_tensor(into).detach().to(F64).reshape(g.shape)
        out[name], out[name + "_mag"] = base + sign * g, base.abs() + g.abs()
    return out


def autograd_consistency(lx, la, n_real, w_real, w_fake):
    """the formula of the issue written once more, for torch autograd: (weighted loss, [L_real, L_fake])"""
    n = lx.shape[0]
    parts = [((lx[sl] - la[sl]) ** 2).sum(1).mean() for sl in _segments(n, n_real)]
    return w_real * parts[0] + w_fake * parts[1], parts


# ------------------------------------------------------------------------------------------------- the kernel's order, in float32
def _segment32(lx, la, nb, Kc, w, grad_scale, into_x, into_a, mistake):
    f = np.float32
    n = nb * Kc
    lx, la = lx.reshape(-1).astype(f), la.reshape(-1).astype(f)
    div = f(n) if mistake == "mean_over_elements" else f(nb)
    inv = f(1.0) / div
    c = ((f(1.0 if mistake == "no_factor_2" else 2.0) * f(w)) / div) * f(grad_scale)
    d = lx - la
    g = c * d
    gx = g if into_x is None else into_x.reshape(-1).astype(f) + g
    if mistake == "same_sign":
        ga = g if into_a is None else into_a.reshape(-1).astype(f) + g
    else:
        ga = -g if into_a is None else into_a.reshape(-1).astype(f) - g
    if float(w) == 0.0:
        gx = np.zeros(n, f) if into_x is None else into_x.reshape(-1).astype(f)
        ga = np.zeros(n, f) if into_a is None else into_a.reshape(-1).astype(f)
    trips = (n + NT - 1) // NT
    sq = np.zeros(trips * NT, f)
    sq[:n] = d * d
    sq = sq.reshape(trips, NT)
    acc = np.zeros(NT, f)
    for t in range(trips):            # thread i adds elements i, i + 256, ... one after the other
        acc = acc + sq[t]             # (the padding adds +0 where the kernel's loop has ended: the same value)
    lane = np.arange(NT)
    for o in (32, 16, 8, 4, 2, 1):    # the butterfly inside each wave of 64
        acc = acc + acc[lane ^ o]
    r = acc[::64]
    loss = (((r[0] + r[1]) + r[2]) + r[3]) * inv
    return f(loss), gx.reshape(nb, Kc), ga.reshape(nb, Kc)


def emulate32(lx, la, n_real, w_real, w_fake, grad_scale=1.0, into_x=None, into_a=None, mistake=None):
    """numpy float32 (loss [2], gx, ga) in the kernel's order.  mistake: None, "same_sign" (the partner gradient with the sign of the
    clean one), "mean_over_elements" (1 / (B Kc) in place of 1 / B), "no_factor_2", "swapped_weights"."""
    lx, la = np.asarray(lx, dtype=np.float32), np.asarray(la, dtype=np.float32)
    n, Kc = lx.shape
    if mistake == "swapped_weights":
        w_real, w_fake = w_fake, w_real
    loss, gx, ga = np.zeros(2, np.float32), np.zeros_like(lx), np.zeros_like(lx)
    for s, (sl, w) in enumerate(zip(_segments(n, n_real), (w_real, w_fake))):
        ix = None if into_x is None else np.asarray(into_x, dtype=np.float32).reshape(n, Kc)[sl]
        ia = None if into_a is None else np.asarray(into_a, dtype=np.float32).reshape(n, Kc)[sl]
        loss[s], gx[sl], ga[sl] = _segment32(lx[sl], la[sl], sl.stop - sl.start, Kc, w, grad_scale, ix, ia,
                                             None if mistake == "swapped_weights" else mistake)
    return loss, gx, ga


# ------------------------------------------------------------------------------------------------------------ error bound
def kappa_grad():
    """Depth of a gradient element, from vg_bcr_loss_body as written: c = ((2 w) / B) grad_scale - 2 w is exact, the division and the
    product round (2); d = lx - la (1); g = c d (1); the accumulating add (1, relative to |into| + |g|, which is what ``mag`` holds);
    the negation is exact.  5 roundings; one more unit covers the second-order terms of their product and the weights' own rounding to
    fp32 at the call.  A contraction of c d + into to one fused operation only removes a rounding."""
    return 2 + 1 + 1 + 1 + 1


def kappa_loss(nb, Kc):
    """Depth of a segment's loss: every term d^2 carries the rounding of d twice and the product's once (3); the terms are summed by
    ceil(B Kc / 256) additions in a thread's strided chain, 6 levels of the wave butterfly and 3 additions over the four waves in
    order; the product with the rounded 1 / B (2).  All terms are non-negative, so every partial sum is at most the total and each
    addition's error is at most 2^-24 of it; one more unit for the second-order terms."""
    trips = (nb * Kc + NT - 1) // NT
    return 3 + trips + 6 + 3 + 2 + 1


def kappa_losses(n, n_real, Kc):
    """the larger of the two segments' depths: one kappa for ``assert_elementwise`` on the [2] vector"""
    return max(kappa_loss(n_real, Kc), kappa_loss(n - n_real, Kc))
