"""Adaptive discriminator augmentation (include/vitgan_hip.h: vg_diffaug_p_fwd / vg_diffaug_p_bwd / vg_ada_update) restated off the
device: a plain helper module built on diffaug_ref.

  * ``gates`` / ``draw_p``: which members of the policy stay on for an image at probability p - an integer compare of the per-image
    24-bit draws 8, 9, 10 against T = floor(clamp(p, 0, 1) 2^24) - and the parameter rows the gated kernels write.  Bit for bit.
  * ``controller``: one call of vg_ada_update in numpy float32, operation for operation as the header states it.  Bit for bit in
    p, acc_sign and acc_count; r_last is one division (1 ulp).
  * ``simulate64``: the textbook heuristic (Karras et al. 2020, "Training generative adversarial networks with limited data", the
    r_t = E[sign(D(real))] signal) in float64, to hold the controller against; ``trajectory_bound`` is how far fp32 may drift from it.
"""
import numpy as np

import diffaug_ref as dr

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ gates
def threshold(p):
    """T = (uint32) floorf(clamp(p, 0, 1) 2^24); a NaN clamps to 0.  The product is a power-of-two scaling: exact in fp32."""
    p = F32(p)
    pc = (p if p < F32(1) else F32(1)) if p > F32(0) else F32(0)
    return int(np.floor(F32(pc) * F32(2.0 ** 24)))


def gate_draws(seed, site, step, n, m):
    """k24(8 + m): the 24-bit draw behind member m's gate (0 color, 1 translation, 2 cutout); step and n broadcast"""
    return dr.k24(seed, site, step, n, 8 + m)


def gates(seed, site, step, B, policy, p):
    """int64 [B]: the effective policy of every image - member m is on iff it is in ``policy`` and k24(8 + m) < T"""
    T = np.uint64(threshold(p))
    n = np.arange(B)
    eff = np.zeros(B, dtype=np.int64)
    for m in range(3):
        if (policy >> m) & 1:
            eff |= (gate_draws(seed, site, step, n, m) < T).astype(np.int64) << m
    return eff


def draw_p(seed, site, step, B, IH, policy, p):
    """float32 [B, 8]: what vg_diffaug_p_fwd writes to params_out - every image's row is diffaug_ref.draw's row under the image's
    effective policy (the parameter draws themselves do not depend on the policy)"""
    eff = gates(seed, site, step, B, policy, p)
    out = np.empty((B, 8), dtype=np.float32)
    for q in np.unique(eff):
        rows = eff == q
        out[rows] = dr.draw(seed, site, step, B, IH, int(q))[rows]
    return out


# ------------------------------------------------------------------------------------------------------------- controller
def sgn(x):
    """sgn with sgn(+-0) = sgn(NaN) = 0, elementwise, as float32"""
    x = np.asarray(x, dtype=np.float32)
    return (x > 0).astype(np.float32) - (x < 0).astype(np.float32)


def controller(state, logits, target, step_per_image, interval, step, mistake=None):
    """One vg_ada_update: state = (p, acc_sign, acc_count, r_last) float32 [4] -> the new state.  Every operation is one float32
    operation, in the header's order.  ``mistake``: one of the planted ones, for the tests of the tests."""
    p, acc_sign, acc_count, r_last = (F32(v) for v in state)
    target, spi = F32(target), F32(step_per_image)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1)
    acc_sign = F32(acc_sign + F32(sgn(logits).sum(dtype=np.float64)))  # integer-valued, |sum| < 2^24: exact in any order
    acc_count = F32(acc_count + F32(logits.size))
    fire = int(step) % int(interval) == 0 or mistake == "every_step"
    if fire:
        d = F32(acc_sign - F32(target * acc_count))
        s = sgn(d)[()]
        if mistake == "sign_flipped":
            s = F32(-s)
        p = F32(p + F32(s * F32(spi * acc_count)))
        if mistake != "no_clamp":
            p = F32(min(max(p, F32(0)), F32(1)))
        with np.errstate(invalid="ignore", divide="ignore"):
            r_last = F32(acc_sign / acc_count)
        if mistake != "no_reset":
            acc_sign, acc_count = F32(0), F32(0)
    return np.array([p, acc_sign, acc_count, r_last], dtype=np.float32)


def simulate64(p0, batches, target, step_per_image, interval, first_step=1):
    """The textbook heuristic in float64: over every window of ``interval`` steps (ending on a step whose number divides by it),
    r_t = mean of sign(D(real)) over the window's images; p moves by sign(r_t - target) * (images in the window) * step_per_image and
    is clipped to [0, 1].  ``batches``: the real logits of steps first_step, first_step + 1, ...  Returns (p after every step, r_t
    after every step - NaN before the first update)."""
    p, signs, r = float(p0), [], float("nan")
    ps, rs = [], []
    for i, lg in enumerate(batches):
        lg = np.asarray(lg, dtype=np.float64).reshape(-1)
        signs.append(np.sign(np.where(np.isnan(lg), 0.0, lg)))
        if (first_step + i) % interval == 0:
            window = np.concatenate(signs)
            r = float(window.mean())
            p = min(max(p + float(np.sign(r - float(target))) * window.size * float(step_per_image), 0.0), 1.0)
            signs = []
        ps.append(p)
        rs.append(r)
    return np.array(ps), np.array(rs)


def trajectory_bound(updates):
    """|p_fp32 - p_float64| after ``updates`` updates: per update one rounding of step_per_image * acc_count (a value <= 1 wherever the
    clamp does not erase it) and one of the sum (<= 2 before the clamp), each half an ulp: 2^-25 + 2^-24, and the clamp does not expand
    a distance; plus one more 2^-24 for step_per_image itself being a rounded float32"""
    return updates * (2.0 ** -25 + 2.0 ** -24 + 2.0 ** -24)
