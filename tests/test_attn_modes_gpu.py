"""The fp8 (mode 2) and L2-distance (mode 1) instantiations of the short attention kernels (csrc/attention.hip), held to the
probes the dot-product bf16 kernels are held to: saturated-softmax probes bit for bit at every S from 1 to 80, with guard
rows and unwritten-element sentinels on every output, and a moderate regime checked element by element against fp64 within
a first-order error budget (tests/attn_modes_ref.py).  tests/test_attn_modes_cpu.py runs the same checkers on a plain-torch
emulation of the kernels' arithmetic (they admit a correct kernel) and on emulated defects (they reject a wrong one).

fp8: every value of AttnProbe is exact in OCP e4m3 (codes 64 / 128, V in [-3, 3], 256 p in {256, 128, 64}), so every fp8
product and fp32 sum is exact and the expectations are those of mode 0, bit for bit.  At S > 32 the backward is
vg_attn_bwd2_kernel<HE, 5, true>, a kernel the L2 mode never reaches.

L2: X.L2Probe.  O, dV and LSE are bit for bit (a tie's LSE within one fp32 ulp of m + log t); dQ and dK are bit for bit
wherever the exact value is nonzero, and an exactly-zero element on a tie may hold up to 2^-12 sum |W| c: the kernel keeps
rowsum(W) / colsum(W) in fp32, where p = exp(m - lse) carries the rounding of lse (one ulp of 2048 is 2^-12, a bound derived
from the format, not measured; with W = 0 it is 0).  The exact LSE of the permutation probe rests on sqrtf returning exactly
4 c for the exact square 16 c^2, i.e. on the compiler's default correctly-rounded square root.  A nonzero dQ cannot be made
exact in this family (no 'sum' kind: 20 c^2 is not a square); the budget tests below cover it.
"""
import math

import pytest
import torch

import attn_modes_ref as R
import exact_util as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CUDA = "cuda"
B, H = 2, 2
FN = {"fp8": ("vg_attention_fp8_fwd", "vg_attention_fp8_bwd"), "l2": ("vg_attention_l2_fwd", "vg_attention_l2_bwd")}
POW2 = {"perm": 1 / 8, "tie2a": 1 / 16, "tie2b": 1 / 8, "tie2c": 1 / 16, "tie4": 1 / 8, "sum": 1 / 16}  # as test_exact_attention_gpu.py
L2_SCALE = 8.0          # gap (4 - sqrt(14)) * 64 * 8 = 132
L2_V1_CODE = 2.0 ** 13  # the forward at v1's 1 / sqrt(H * HE): gap (4 - sqrt(14)) * 8192 / sqrt(192) = 152


def tie_places(S, kind):
    """the tie placements of test_exact_attention_gpu.py::_probe: (probe kind, tied keys), or ('perm', None) below the
    smallest S that has room for them"""
    if kind == "tie2a" and S >= 2:
        return "tie2", (0, S - 1)
    if kind == "tie2b" and S >= 2:
        a = 32 * ((S - 1) // 32)
        return "tie2", ((a, a + 1) if a + 1 < S else (a - 1, a))
    if kind == "tie2c" and S >= 17:
        return "tie2", (S - 17, S - 1)
    if kind == "tie4" and S >= 4:
        return "tie4", (0, S // 3, (2 * S) // 3, S - 1)
    return ("sum" if kind == "sum" else "perm"), None


def fp8_probe(S, HE, kind, seed=0):
    k, ties = tie_places(S, kind)
    return X.AttnProbe(B, H, S, HE, k, ties, seed)


def l2_probe(S, HE, kind, seed=0, code=X.CODE):
    k, ties = tie_places(S, kind)
    return X.L2Probe(B, H, S, HE, k, ties, seed, code)


def _launch_fwd(mode, qkv, S, HE, scale):
    u = X.gpu()
    O = X.guarded(B * S, H * HE, BF, CUDA)
    L = X.guarded(B * H * S, 1, F32, CUDA)
    u.call(FN[mode][0], u.ptr(qkv), u.ptr(O), u.ptr(L), B, H, S, HE, scale, u.stream())
    u.sync()
    return O, L


def _launch_bwd(mode, qkv, O, dO, L, S, HE, scale):
    u = X.gpu()
    dQKV = X.guarded(B * S, 3 * H * HE, BF, CUDA)
    u.call(FN[mode][1], u.ptr(qkv), u.ptr(O), u.ptr(dO), u.ptr(L), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    return dQKV


def _exact_fwd(mode, p, scale):
    qkv = p.qkv.to(CUDA).to(BF)
    O, L = _launch_fwd(mode, qkv, p.S, p.HE, scale)
    R.check_exact_fwd(p, scale, O, L)
    return qkv, O, L


def _exact_bwd(mode, p, scale):
    """forward, then the backward on the kernel's own O and LSE"""
    qkv, O, L = _exact_fwd(mode, p, scale)
    dQKV = _launch_bwd(mode, qkv, O, p.flat(p.dO).to(CUDA).to(BF), L, p.S, p.HE, scale)
    R.check_exact_bwd(p, scale, dQKV)


@pytest.mark.parametrize("kind", list(POW2))
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_fp8_attention_every_S(HE, kind):
    """vg_attention_fp8_fwd + _bwd at S = 1..80 with a power-of-two scale (exact dS), and the forward at 1/sqrt(HE)"""
    def one(S):
        p = fp8_probe(S, HE, kind)
        p.check_preconditions([POW2[kind], 1 / math.sqrt(HE)])
        p.check_fp8_preconditions()
        _exact_bwd("fp8", p, POW2[kind])
        _exact_fwd("fp8", p, 1 / math.sqrt(HE))
    X.collect(list(range(1, 81)), one, "S=")


@pytest.mark.parametrize("kind", ["perm", "tie2a", "tie2b", "tie2c", "tie4"])
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_l2_attention_every_S(HE, kind):
    """vg_attention_l2_fwd + _bwd at S = 1..80 with c = 64, scale 8, and the forward at v1's own 1/sqrt(H HE) with c = 2^13"""
    v1 = 1 / math.sqrt(H * HE)

    def one(S):
        p = l2_probe(S, HE, kind)
        p.check_preconditions([L2_SCALE], bwd_scale=L2_SCALE)
        _exact_bwd("l2", p, L2_SCALE)
        w = l2_probe(S, HE, kind, code=L2_V1_CODE)
        w.check_preconditions([v1])
        _exact_fwd("l2", w, v1)
    X.collect(list(range(1, 81)), one, "S=")


# --------------------------------------------------------------------------------------- the moderate regime, per element
def mode_scale(mode, HE):
    """fp8: the ViT's 1/sqrt(HE); l2: v1's 1/sqrt(H HE)"""
    return 1 / math.sqrt(HE) if mode == "fp8" else 1 / math.sqrt(H * HE)


@pytest.mark.parametrize("HE", [32, 64, 96])
@pytest.mark.parametrize("mode", ["fp8", "l2"])
def test_attention_modes_within_budget(mode, HE):
    """forward and backward on dyadic inputs at every S of R.S_LIST, every output element within its own first-order budget of
    the fp64 result; the backward is given the reference O (one bf16 rounding) and LSE (fp32), as the budget assumes; every
    launch is repeated once and must reproduce every bit.  Prints the largest fraction of the budget used."""
    worst = {"fwd": 0.0, "bwd": 0.0}
    scale = mode_scale(mode, HE)

    def one(S):
        Q, K, V, dO = R.dyadic_inputs(B, H, S, HE, mode)
        r = R.reference(mode, Q, K, V, dO, scale)
        bud = R.budget(r)
        qkv = torch.cat([R.flat(t) for t in (Q, K, V)], 1).to(CUDA).to(BF)
        O, L = _launch_fwd(mode, qkv, S, HE, scale)
        for buf, rows, name in ((O, B * S, "O"), (L, B * H * S, "LSE")):
            X.assert_written(buf, rows, name)
            X.assert_guard(buf, rows, name)
        worst["fwd"] = max(worst["fwd"], R.check_budget_fwd(r, bud, O[:B * S], L[:B * H * S, 0].reshape(B, H, S)))
        O_in = R.flat(r["O_bf"]).to(CUDA).to(BF)
        L_in = r["lse_f32"].reshape(-1).to(CUDA).to(F32)
        dOd = R.flat(dO).to(CUDA).to(BF)
        dQKV = _launch_bwd(mode, qkv, O_in, dOd, L_in, S, HE, scale)
        X.assert_written(dQKV, B * S, "dQKV")
        X.assert_guard(dQKV, B * S, "dQKV")
        worst["bwd"] = max(worst["bwd"], R.check_budget_bwd(r, bud, dQKV[:B * S]))
        O2, L2 = _launch_fwd(mode, qkv, S, HE, scale)
        dQKV2 = _launch_bwd(mode, qkv, O_in, dOd, L_in, S, HE, scale)
        for a, b_, name in ((O2, O, "O"), (L2, L, "LSE"), (dQKV2, dQKV, "dQKV")):
            assert torch.equal(X.bits(a), X.bits(b_)), f"{name}: a repeated launch differs"
    X.collect(R.S_LIST, one, "S=")
    print(f"{mode} HE={HE}: largest fraction of the budget used: forward {worst['fwd']:.3f}, backward {worst['bwd']:.3f}")


@pytest.mark.parametrize("S,HE", [(81, 64), (80, 48)])
@pytest.mark.parametrize("mode", ["fp8", "l2"])
def test_attention_modes_refuse_unsupported(mode, S, HE):
    """S = 81 and HE = 48: a nonzero status from forward and backward, and not one output element touched"""
    u = X.gpu()
    lib = u._lib.lib()
    E = H * HE
    qkv = torch.zeros(B * S, 3 * E, dtype=BF, device=CUDA)
    dO = torch.zeros(B * S, E, dtype=BF, device=CUDA)
    O = X.guarded(B * S, E, BF, CUDA)
    L = X.guarded(B * H * S, 1, F32, CUDA)
    dQKV = X.guarded(B * S, 3 * E, BF, CUDA)
    assert getattr(lib, FN[mode][0])(u.ptr(qkv), u.ptr(O), u.ptr(L), B, H, S, HE, 0.125, u.stream()) != 0
    assert getattr(lib, FN[mode][1])(u.ptr(qkv), u.ptr(O), u.ptr(dO), u.ptr(L), u.ptr(dQKV), B, H, S, HE, 0.125, u.stream()) != 0
    u.sync()
    for buf, name in ((O, "O"), (L, "LSE"), (dQKV, "dQKV")):
        X.assert_guard(buf, 0, name)
