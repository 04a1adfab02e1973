"""The learning-rate schedule in Python float64 (a plain helper module, no product code): what vg_lr_schedule is held to.

    f = f_w f_d,   f_w = t / warmup for 1 <= t <= warmup, else exactly 1 (warmup == 0 too)
    f_d = 1 exactly while t <= warmup and for "constant";  f_d = final exactly once t >= total;  in between, with
    s = (t - warmup) / (total - warmup):   "linear" 1 - (1 - final) s;   "cosine" final + (1 - final) 0.5 (1 + cos(pi s))
    lr = base f scale

The kernel computes the same in fp64 and rounds ONCE to fp32, so it lies within one fp32 ulp of ``lr_now`` (half an ulp of rounding, and
the two fp64 evaluations differ by ~1e-16 relative, which can move a value across one rounding boundary and no further); where the
factor branch is exact and the products are exact in fp64 - a 24-bit base times a 24-bit scale is - it is fp32(lr_now) bit for bit.
A kernel receives base, final and scale as float32: they are widened with ``adamw_ref.f32`` here.  A counter below 1 counts as 1.
"""
import math

from adamw_ref import f32

KINDS = ("constant", "linear", "cosine")


def factor(kind: str, t: int, warmup: int, total: int, final: float) -> float:
    assert kind in KINDS and warmup >= 0
    t = max(int(t), 1)
    if t <= warmup:
        return 1.0 if t == warmup else t / warmup
    if kind == "constant":
        return 1.0
    fin = f32(final)
    if t >= total:
        return fin
    s = (t - warmup) / (total - warmup)
    if kind == "linear":
        return 1.0 - (1.0 - fin) * s
    return fin + (1.0 - fin) * 0.5 * (1.0 + math.cos(math.pi * s))


def exact(kind: str, t: int, warmup: int, total: int) -> bool:
    """Is the factor an explicit branch (1 or ``final``, no arithmetic)?"""
    t = max(int(t), 1)
    return t == warmup or (t > warmup and (kind == "constant" or t >= total))


def lr_now(base: float, kind: str, t: int, warmup: int, total: int, final: float, scale: float = 1.0) -> float:
    return f32(base) * factor(kind, t, warmup, total, final) * f32(scale)
