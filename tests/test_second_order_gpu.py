"""The second-order (gradient-penalty) kernels through the C ABI against the float64 references of tests/second_order_ref.py.

vg_act_fwd / _bwd / _bwd_bwd on every finite bf16; vg_layernorm_bwd_bwd at every width, at row counts on both sides of its four-row
workgroups and of its 2048-workgroup grid cap; vg_attention_bwd_bwd on designed inputs at every S from 1 to 80 and on random inputs;
vg_vit_penalty against the float64 oracle.  No ops2 wrapper in between.  The statistical bounds (fit_terms, relative RMS) are 4 x the
floors that tests/test_second_order_ref_cpu.py measures from the references alone; kappa and A are derived next to their use."""
import math

import pytest
import torch

import exact_util as X
import second_order_ref as R
from exact_util import BF

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _u():
    return X.gpu()


def _rc(name, *args):
    """raw return code of a C-ABI call"""
    from vit_gan_amd import _lib
    return getattr(_lib.lib(), name)(*args)


def _flat_guarded(n, dtype=BF):
    """n elements (n % 4 == 0 or not: one row of n) with X.GUARD_ROWS rows of sentinel behind"""
    return X.guarded(1, n, dtype, "cuda")


# ------------------------------------------------------------------------------------------------------------- activations
def _all_finite_bf16():
    b = torch.arange(65536, dtype=torch.int32)
    b = b[(b & 0x7F80) != 0x7F80]
    assert b.numel() == 65280 and b.numel() % 4 == 0
    return b.to(torch.int16).view(BF)


def _act_three(h, dy, u, act):
    """(f, dy f', u f', u dy f'') from vg_act_fwd, vg_act_bwd, vg_act_bwd_bwd"""
    g = _u()
    n = h.numel()
    y, dh, d_dy, d_h = (torch.empty(n, dtype=BF, device="cuda") for _ in range(4))
    g.call("vg_act_fwd", g.ptr(h), g.ptr(y), n, act, g.stream())
    g.call("vg_act_bwd", g.ptr(dy), g.ptr(h), g.ptr(dh), n, act, g.stream())
    g.call("vg_act_bwd_bwd", g.ptr(u), g.ptr(dy), g.ptr(h), g.ptr(d_dy), g.ptr(d_h), n, act, g.stream())
    g.sync()
    return y.cpu(), dh.cpu(), d_dy.cpu(), d_h.cpu()


# absolute error allowances A of (f, f', f'') next to the 2^-8 |ref| of the bf16 result, from the formulas of vg_common.h (u = 2^-24):
#  gelu: Phi = (1 + erf) / 2 with erf by A&S 7.1.26, |err| < 1.5e-7, + the rounding of erf next to 1 (u) + the evaluation of poly * e
#        (five Horner steps on coefficients <= 1.5, 1-ulp v_rcp and v_exp, the rounded exponent: <= 6e-7 e, e = exp(-h^2/2)) and the
#        rounding of Phi (u/2):  dPhi <= 1.1e-7 + 3e-7 e.   phi = e / sqrt(2 pi): relative (4 + h^2) u.
#        f  = h Phi:  |h| dPhi, largest at the negative end of the unsaturated range (|h| = 5.6, above it erf rounds to -1): 6.2e-7;
#        f' = Phi + h phi:  dPhi + |h| phi (4 + h^2) u + 1.13 * 2u  <=  2.9e-7 + 1.5e-7 + 1.4e-7 = 5.8e-7 (at |h| = 1);
#        f''= phi (2 - h^2):  phi ((4 + h^2) |2 - h^2| + 2 + h^2) 2u, largest at h = 0: 0.399 * 10 * 1.2e-7 = 4.8e-7.
#  tanh: t = 1 - 2 / (e^{2h} + 1) =: 1 - r.  __expf(2h): relative (2|h| + 2) u; e + 1: u; v_rcp: 1 ulp of r.
#        dr <= r (e / (e + 1)) (2|h| + 3) u + ulp(r) <= 1.8e-7 + 2.4e-7 (r < 2), the subtraction u:  dt <= 4.8e-7 -> A_f = 5.4e-7 with the
#        rounding of 2h log2(e);  f' = 1 - t^2:  2 |t| dt + u <= 1.15e-6;  f'' = -2 t f':  2 dt (f' + 2 t^2) + 2u <= 4 dt + 2u = 2.3e-6.
ACT_A = {1: (6.2e-7, 5.8e-7, 4.8e-7), 3: (5.4e-7, 1.15e-6, 2.3e-6)}
ACT_KIND = {1: "gelu", 3: "tanh"}


def _assert_act(got, ref, A, what):
    got64 = got.double()
    assert bool(torch.isfinite(got64).all()), f"{what}: {int((~torch.isfinite(got64)).sum())} non-finite values, first at bit pattern " \
        f"{int((~torch.isfinite(got64)).nonzero()[0])}"
    err = (got64 - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + A
    # a result below bf16's normal range may be flushed: the allowance covers it (2^-126 << A)
    bad = ~(err <= lim)
    worst = float((err - 2.0 ** -8 * ref.abs()).max())
    print(f"{what}: largest |err| - 2^-8 |ref| = {worst:.3e} = {worst / A:.2f} A")
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside 2^-8 |ref| + {A:g}; first at index {i}: got {float(got64[i])!r} "
                             f"want {float(ref[i])!r}")


@pytest.mark.parametrize("act", [1, 3])
def test_activation_kernels_on_every_finite_bf16(act):
    """h = every finite bf16 bit pattern, dy = u = 1: the three kernels return f, f', f'' themselves.  Then dy, u = +-2^k: the products
    add no rounding, so d_dy and d_h must be the first pass scaled, bit for bit."""
    g = _u()
    hb = _all_finite_bf16()
    h = g.dev(hb)
    one = torch.ones_like(h)
    f, d1, d1b, d2 = _act_three(h, one, one, act)
    h64 = hb.double()
    rf, r1, r2, _, _ = R.act_funcs(ACT_KIND[act], h64)
    A = ACT_A[act]
    _assert_act(f, rf, A[0], f"act {act} f")
    _assert_act(d1, r1, A[1], f"act {act} f' (vg_act_bwd)")
    _assert_act(d2, r2, A[2], f"act {act} f''")
    X.assert_bitwise(d1b, d1, "f' of vg_act_bwd_bwd vs vg_act_bwd")
    # saturation: beyond |h| = 15 exp(-h^2/2) and 1 - tanh^2 are below half an fp32 ulp of anything they are added to
    sat = h64.abs() >= 15
    assert bool((d2.double()[sat] == 0).all()), "f'' is not exactly 0 beyond |h| = 15"
    assert bool((d1.double()[sat & (h64 < 0)] == 0).all()), "f' is not exactly 0 below -15"
    assert bool((d1.double()[sat & (h64 > 0)] == (1.0 if act == 1 else 0.0)).all()), "f' is not exactly saturated above 15"
    if act == 1:
        assert bool((f.double()[sat & (h64 > 0)] == h64[sat & (h64 > 0)]).all()) and bool((f.double()[sat & (h64 < 0)] == 0).all())
    else:
        assert bool((f.double()[sat] == torch.sign(h64[sat])).all())
    # second pass
    gen = X.gen(7)
    n = h.numel()
    pw = lambda: (2.0 ** torch.randint(-3, 4, (n,), generator=gen).double()) * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)  # noqa: E731
    dy64, u64 = pw(), pw()
    _, dh_s, ddy_s, dh2_s = _act_three(h, g.dev(dy64, BF), g.dev(u64, BF), act)
    # (where the unscaled bf16 result is tiny, the scaled one can leave bf16's normal range: those stay with the bound above)
    for got, base, s, what in ((dh_s, d1, dy64, "dh = dy f'"), (ddy_s, d1, u64, "d_dy = u f'"), (dh2_s, d2, u64 * dy64, "d_h = u dy f''")):
        ok = (base.double() == 0) | (base.double().abs() >= 2.0 ** -100)
        want = (base.double() * s).float().to(BF)
        X.assert_bitwise(torch.where(ok, got, want), want, what)


@pytest.mark.parametrize("act", [1, 3])
def test_activation_kernels_sizes_and_guards(act):
    g = _u()
    for n in (4, 1020, 1024, 1028):
        gen = X.gen(n)
        h64, dy64, u64 = ((torch.randn(n, generator=gen, dtype=F64) * s).to(BF).double() for s in (2.0, 1.0, 1.0))
        h, dy, u = (g.dev(t, BF) for t in (h64, dy64, u64))
        o0, o1 = _flat_guarded(n), _flat_guarded(n)
        g.call("vg_act_bwd_bwd", g.ptr(u), g.ptr(dy), g.ptr(h), g.ptr(o0), g.ptr(o1), n, act, g.stream())
        g.sync()
        ref = R.act_closed(ACT_KIND[act], h64, dy64, u64)
        for buf, name, A in ((o0, "d_dy", ACT_A[act][1]), (o1, "d_h", ACT_A[act][2])):
            X.assert_guard(buf, 1, f"n {n} {name}")
            X.assert_written(buf, 1, f"n {n} {name}")
            # |u|, |dy| < 8 scale the absolute allowance
            _assert_act(buf[0].cpu(), ref[name], A * float((u64.abs() * (dy64.abs() if name == "d_h" else 1)).max()), f"n {n} {name}")


def test_activation_kernels_refuse_bad_arguments():
    g = _u()
    h = torch.zeros(1024, dtype=BF, device="cuda")
    for n, act in ((1024, 0), (1024, 2), (1022, 1), (1021, 3), (0, 1)):
        o0, o1 = _flat_guarded(1024), _flat_guarded(1024)
        rcs = (_rc("vg_act_fwd", g.ptr(h), g.ptr(o0), n, act, g.stream()),
               _rc("vg_act_bwd", g.ptr(h), g.ptr(h), g.ptr(o0), n, act, g.stream()),
               _rc("vg_act_bwd_bwd", g.ptr(h), g.ptr(h), g.ptr(h), g.ptr(o0), g.ptr(o1), n, act, g.stream()))
        g.sync()
        assert all(rc < 0 for rc in rcs), (n, act, rcs)
        for buf in (o0, o1):
            X.assert_guard(buf, 0, f"n {n} act {act}: refused call wrote")


# ------------------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = [128, 256, 384, 512, 640, 768, 896, 1024]


def _ln_run(u, dy, x, mean, rstd, gamma, Rr, E):
    """one launch + the fold of d_gamma; returns guarded d_dy, d_x, part and d_gamma"""
    g = _u()
    parts = _rc("vg_layernorm_bwd_bwd_parts", Rr)
    assert parts == min((Rr + 3) // 4, 2048)
    d_dy, d_x = X.guarded(Rr, E, BF, "cuda"), X.guarded(Rr, E, BF, "cuda")
    part = X.guarded(parts, E, torch.float32, "cuda", guard=16)
    g.call("vg_layernorm_bwd_bwd", g.ptr(u), g.ptr(dy), g.ptr(x), g.ptr(mean), g.ptr(rstd), g.ptr(gamma), g.ptr(d_dy), g.ptr(d_x), g.ptr(part),
           Rr, E, g.stream())
    dgam = X.guarded(1, E, torch.float32, "cuda", guard=1)
    g.call("vg_colsum_f32", g.ptr(part), parts, E, g.ptr(dgam), E, None, 0, None, 0, None, 0, 0, g.stream())
    g.sync()
    return d_dy, d_x, part, dgam, parts


def _ln_case(E, Rr):
    g = _u()
    u64, dy64, x64, gam64 = R.ln_inputs(Rr, E, 1)
    mean64, rstd64 = R.ln_stats(x64)
    mean, rstd = mean64.float(), rstd64.float()
    ref = R.ln_closed(u64, dy64, x64, mean, rstd, gam64)
    dev = [g.dev(t, BF) for t in (u64, dy64, x64)] + [g.dev(mean), g.dev(rstd), g.dev(gam64, torch.float32)]
    d_dy, d_x, part, dgam, parts = _ln_run(*dev, Rr, E)
    what = f"E {E} R {Rr}"
    for buf, rows, n in ((d_dy, Rr, "d_dy"), (d_x, Rr, "d_x"), (part, parts, "part"), (dgam, 1, "d_gamma")):
        X.assert_guard(buf, rows, f"{what} {n}")
        X.assert_written(buf, rows, f"{what} {n}")
    stats = {}
    for buf, n in ((d_dy, "d_dy"), (d_x, "d_x")):
        stats[n] = R.assert_elementwise(buf[:Rr], ref[n], ref["mag_" + n], R.ln_kappa(E), f"{what} {n}")
        if R.ln_fit_runs(Rr, E):
            stats["fit " + n] = R.assert_fit(buf[:Rr], ref[n + "_terms"], R.ln_fit_bound(Rr, E), f"{what} {n}") / R.ln_fit_bound(Rr, E)
    stats["d_gamma"] = R.assert_elementwise(dgam[0], ref["d_gamma"], ref["mag_d_gamma"], R.ln_kappa_gamma(E, Rr), f"{what} d_gamma", rel=0.0)
    print(what, {k: round(v, 3) for k, v in stats.items()}, "(fractions of the bounds)")
    # a second launch is bitwise the same; u * 2^3 scales every output by 2^3, bit for bit (every output is linear in u)
    again = _ln_run(*dev, Rr, E)
    scaled = _ln_run(g.dev(u64 * 8, BF), *dev[1:], Rr, E)
    for i, rows, n in ((0, Rr, "d_dy"), (1, Rr, "d_x"), (3, 1, "d_gamma")):
        a, b, s = (d_dy, d_x, part, dgam)[i], again[i], scaled[i]
        X.assert_bitwise(b[:rows], a[:rows], f"{what} {n}: second launch")
        X.assert_bitwise(s[:rows], (a[:rows].float() * 8).to(a.dtype), f"{what} {n}: u scaled by 8")


@pytest.mark.parametrize("E", LN_WIDTHS)
def test_layernorm_double_backward_against_fp64(E):
    """R = 1, 3, 4, 5 (around one workgroup of four rows), 130, 8192 (every one of the 2048 partial rows in use); at E = 384 and 512
    also 1040, 8193, 8199 and 16 640: the second trip of the grid-stride loop, ragged and full."""
    rows = [1, 3, 4, 5, 130, 8192] + ([1040, 8193, 8199, 16640] if E in (384, 512) else [])
    X.collect(rows, lambda Rr: _ln_case(E, Rr), f"E {E} R ")


def test_layernorm_double_backward_refuses_bad_shapes():
    g = _u()
    for E, Rr in ((64, 8), (192, 8), (1088, 8), (384, 0)):
        t = torch.zeros(8, max(E, 64), dtype=BF, device="cuda")
        f = torch.ones(1088, dtype=torch.float32, device="cuda")
        d_dy, d_x = X.guarded(0, 1088, BF, "cuda", guard=8), X.guarded(0, 1088, BF, "cuda", guard=8)
        part = X.guarded(0, 1088, torch.float32, "cuda", guard=8)
        rc = _rc("vg_layernorm_bwd_bwd", g.ptr(t), g.ptr(t), g.ptr(t), g.ptr(f), g.ptr(f), g.ptr(f), g.ptr(d_dy), g.ptr(d_x), g.ptr(part), Rr, E,
                 g.stream())
        g.sync()
        assert rc == -3, (E, Rr, rc)
        for buf in (d_dy, d_x, part):
            X.assert_guard(buf, 0, f"E {E} R {Rr}: refused call wrote")


# ------------------------------------------------------------------------------------------------------------- attention
def _attn_run(qkv, d_o, lse, uqkv, B, H, S, HE, scale):
    """vg_attention_bwd_bwd on row-layout bf16 device tensors; guarded outputs [B*S, E] and [B*S, 3E]"""
    g = _u()
    E = H * HE
    d_do, d_qkv = X.guarded(B * S, E, BF, "cuda"), X.guarded(B * S, 3 * E, BF, "cuda")
    g.call("vg_attention_bwd_bwd", g.ptr(qkv), g.ptr(d_o), g.ptr(lse), g.ptr(uqkv), g.ptr(d_do), g.ptr(d_qkv), B, H, S, HE, float(scale), g.stream())
    g.sync()
    for buf, n in ((d_do, "d(dO)"), (d_qkv, "d(qkv)")):
        X.assert_guard(buf, B * S, n)
        X.assert_written(buf, B * S, n)
    return d_do[:B * S].cpu(), d_qkv[:B * S].cpu()


def _attn_call(inp, lse, B, H, S, HE, scale):
    """inputs [B, H, S, HE] float64 (bf16-valued), lse [B, H, S] fp32 -> the four outputs as [B, H, S, HE] bf16 (CPU)"""
    g = _u()
    q, k, v, d_o, uq, uk, uv = inp
    E = H * HE
    rows = lambda *ts: g.dev(torch.cat([R.heads_to_rows(t) for t in ts], 1), BF)  # noqa: E731
    d_do, d_qkv = _attn_run(rows(q, k, v), rows(d_o), g.dev(lse.float()), rows(uq, uk, uv), B, H, S, HE, scale)
    hd = lambda t: R.rows_to_heads(t, B, H, S, HE)  # noqa: E731
    return {"d_do": hd(d_do), "d_q": hd(d_qkv[:, :E]), "d_k": hd(d_qkv[:, E:2 * E]), "d_v": hd(d_qkv[:, 2 * E:])}


DESIGNED_SCALE = 1.0 / 16   # CODE^2 / 16 = 256 >= MIN_GAP: every unwanted exp underflows to 0


def _designed(S, HE, kind):
    """AttnProbe q, k (B = 3, H = 2: another probe per image and head) with sparse small-integer v, d_out, u_qkv.  Returns inputs, the
    exact P and the float64 result; for the ties P, H, dS and Sg are asserted to be exact in bf16 (short dyadic numbers), so that the
    kernel's own roundings of them are exact too."""
    B, H = 3, 2
    if kind == "perm":
        p = X.AttnProbe(B, H, S, HE, "perm", None, 11)
    elif kind == "tie2a":
        p = X.AttnProbe(B, H, S, HE, "tie2", (0, S - 1), 12)
    else:
        p = X.AttnProbe(B, H, S, HE, "tie4", (0, S // 3, (2 * S) // 3, S - 1), 13)
    p.check_preconditions([DESIGNED_SCALE])
    gen = X.gen(1000 * S + HE)
    shape = (B, H, S, HE)
    v = X.counting(shape, gen, -4, 4, 0.1)
    d_o, uq, uk, uv = (X.counting(shape, gen, -2, 2, 4.0 / HE) for _ in range(4))
    inp = [p.Q, p.K, v, d_o, uq, uk, uv]
    m, logt = p.lse_exact(DESIGNED_SCALE)
    lse64 = m + logt
    P = p.P()
    ref = R.attn_closed(*inp, lse64, DESIGNED_SCALE)
    assert float((ref["P"] - P).abs().max()) < 1e-12
    for n in ("P", "H", "dS", "Sg"):
        assert float((ref[n] - ref[n].to(BF).double()).abs().max()) < 1e-9, f"designed inputs: {n} is not exact in bf16 at S {S} HE {HE} {kind}"
    ref["P_exact"] = P
    return inp, lse64, ref


@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_double_backward_designed_inputs_every_S(HE):
    """saturated-softmax probes at every S from 1 to 80.  'perm': P is a permutation matrix, so d(dO) = P uV exactly and d(Q) = d(K) =
    d(V) = 0 exactly: bitwise.  'tie2a' / 'tie4': P in {0, 1/2, 1/4}; exp(-ln 2) is 1/2 only after its bf16 rounding and lse = 512 + ln t
    carries an fp32 rounding of 2^-15 relative, so every output is held to one bf16 ulp of rne(fp64) + 4 * 2^-15 * mag (P enters each
    term at most three times; mag is the sum of magnitudes through every cancellation)."""
    def one(case):
        S, kind = case
        if (kind == "tie2a" and S < 2) or (kind == "tie4" and S < 4):
            return
        inp, lse64, ref = _designed(S, HE, kind)
        got = _attn_call(inp, lse64, 3, 2, S, HE, DESIGNED_SCALE)
        for n in R.ATTN_OUTPUTS:
            if kind == "perm":
                want = ref["P_exact"] @ inp[6] if n == "d_do" else torch.zeros_like(ref[n])
                assert float((ref[n] - want).abs().max()) < 1e-9, "the analytic result of the permutation probe"
                X.assert_bitwise(got[n].contiguous(), X.rne(want, BF), f"{kind} {n}")
            else:
                X.assert_ulps(got[n], ref[n], f"{kind} {n}", ulps=1.0, floor=4 * 2.0 ** -15 * ref["mag_" + n])
    X.collect([(S, kind) for S in range(1, 81) for kind in ("perm", "tie2a", "tie4")], one, f"HE {HE} (S, kind) ")


ATTN_S = [1, 15, 16, 17, 32, 33, 48, 64, 65, 67, 68, 79, 80]


def _attn_random(B, H, S, HE, stats):
    inp = R.attn_inputs(B, H, S, HE, 3)
    scale = 1.0 / math.sqrt(HE)
    lse = R.attn_lse(inp[0], inp[1], scale).float()
    ref = R.attn_closed(*inp, lse, scale, bf16_operands=True)
    got = _attn_call(inp, lse, B, H, S, HE, scale)
    for n in R.ATTN_OUTPUTS:
        assert bool(torch.isfinite(got[n].float()).all()), n
        if S == 1 and n != "d_do":
            # one key: P = 1 and d(Q) = d(K) = d(V) = 0 exactly.  The kernel's P is exp(fp32(s q.k) - fp32(lse)) = 1 + e with
            # |e| <= 2 |s q.k| 2^-24 + 2^-21 < 2^-16 for |s q.k| < 100, and every zero above is a difference it multiplies once
            lim = 2.0 ** -16 * ref["mag_" + n]
            assert bool((got[n].double().abs() <= lim + 1e-30).all()), f"{n} at S = 1 is not zero within 2^-16 mag"
            continue
        e = R.rel_rms(got[n], ref[n])
        stats["rms"] = max(stats["rms"], e / R.ATTN_RMS_BOUND)
        assert e <= R.ATTN_RMS_BOUND, f"{n}: relative RMS error {e:.3e} > {R.ATTN_RMS_BOUND:.3e}"
    if S >= R.ATTN_FIT_MIN_S:
        for n in R.ATTN_FIT_OUTPUTS:
            stats["fit"] = max(stats["fit"], R.assert_fit(got[n], ref[n + "_terms"], R.ATTN_FIT_BOUND, n) / R.ATTN_FIT_BOUND)


@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_double_backward_random_inputs(HE):
    """B x H = 2 x 4 at the S on both sides of every 16-row tile, and once 48 x 12 (more workgroups than are resident at once)"""
    stats = {"rms": 0.0, "fit": 0.0}
    X.collect(ATTN_S, lambda S: _attn_random(2, 4, S, HE, stats), f"HE {HE} S ")
    _attn_random(48, 12, 65, HE, stats)
    print(f"HE {HE}: worst relative RMS {stats['rms']:.2f} of its bound, worst fit deviation {stats['fit']:.2f} of its bound")


def test_attention_double_backward_refuses_bad_shapes():
    g = _u()
    for S, HE in ((0, 64), (81, 64), (16, 48)):
        B, H = 1, 2
        E = H * HE
        n = max(S, 1)
        qkv = torch.zeros(B * n, 3 * E, dtype=BF, device="cuda")
        d_o = torch.zeros(B * n, E, dtype=BF, device="cuda")
        lse = torch.zeros(B * H * n, dtype=torch.float32, device="cuda")
        d_do, d_qkv = X.guarded(0, E, BF, "cuda"), X.guarded(0, 3 * E, BF, "cuda")
        rc = _rc("vg_attention_bwd_bwd", g.ptr(qkv), g.ptr(d_o), g.ptr(lse), g.ptr(qkv), g.ptr(d_do), g.ptr(d_qkv), B, H, S, HE, 0.125, g.stream())
        g.sync()
        assert rc < 0, (S, HE, rc)
        X.assert_guard(d_do, 0, f"S {S} HE {HE}: refused call wrote d(dO)")
        X.assert_guard(d_qkv, 0, f"S {S} HE {HE}: refused call wrote d(qkv)")


# ------------------------------------------------------------------------------------------------- the penalty as one call
@pytest.mark.parametrize("geo", ["c2", "c4", "e128", "c2-10-classes", "c2-17-classes", "c2-mlp4"])
def test_penalty_c_call_against_the_float64_oracle(geo):
    """vg_vit_penalty against oracle.step_oracle.gradient_penalty over oracle.vit_oracle.vit_forward in float64 (B = 16, L = 2, dropout
    off; tests/test_second_order_ref_cpu.py checks that the oracle really runs in float64).  The weights are rounded to bf16 first, so
    both sides read the same parameters.  Per parameter tensor: 2^-4 of max|ref| and the projection <got, ref> / <ref, ref> within 2^-6
    of 1; the penalty within 2^-7.  Tensors whose reference gradient is round-off of an exact zero (the key bias: softmax cancels it)
    are held to the buffer's scale and not projected - at most that one per block, and the bias of the last Linear, which no input
    gradient depends on."""
    from oracle import step_oracle as so, vit_oracle as vo
    from test_gp_gpu import _penalty_c_call
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    B, L = 16, 2
    kw = dict(embeddings_dimension=384, classes_count=1, dropout_rate=0.0, batch_size=B, transformer_blocks_count=L)
    dims = dict(image=32, patch=4, embed=384, heads=4, mlp_ratio=2, classes=1)
    if geo == "c4":
        kw.update(embeddings_dimension=512, attention_heads_count=8, patch_size=8, image_size=64)
        dims.update(image=64, patch=8, embed=512, heads=8)
    elif geo == "c2-10-classes":
        kw.update(classes_count=10)
        dims.update(classes=10)
    elif geo == "c2-17-classes":   # Kc > 16: vg_head_bwd_launch(ones, ...) leaves the one-launch kernel for vg_head_bwd_dz_kernel
        kw.update(classes_count=17)
        dims.update(classes=17)
    elif geo == "c2-mlp4":
        kw.update(mlp_ratio=4)
        dims.update(mlp_ratio=4)
    elif geo == "e128":
        kw.update(embeddings_dimension=128, attention_heads_count=4)
        dims.update(embed=128, heads=4)
    torch.manual_seed(3)
    D = ViTDiscriminator(Config(**kw)).cuda().train()
    fl = D.vit._flat
    with torch.no_grad():
        fl.flat.copy_(fl.flat.to(BF).float())
    d = vo.VitDims(layers=L, **dims)
    assert (D.vit._dims.E, D.vit._dims.H, D.vit._dims.L, D.vit._dims.Kc) == (d.embed, d.heads, d.layers, d.classes)
    img = dims["image"]
    gen = torch.Generator().manual_seed(B)
    real = (torch.rand(B, 3, img, img, generator=gen) * 2 - 1).to(BF).float()
    fake = (torch.rand(B, 3, img, img, generator=gen) * 2 - 1).to(BF).float()
    eps = torch.rand(B, 1, 1, 1, generator=gen)
    w = 10.0
    got_pen, got = _penalty_c_call(D, real.cuda(), fake.cuda(), eps.cuda(), w)
    got = got.double().cpu()
    st = {"vit." + k: p.detach().double().cpu().clone().requires_grad_(True) for k, p in D.vit.named_parameters()}
    assert set(st) == set(vo.vit_param_shapes(d))
    pen = so.gradient_penalty(lambda t: vo.vit_forward(st, t, d), real.double(), fake.double(), eps.double())
    assert pen.dtype == F64
    (w * pen).backward()
    ref_pen = float(pen.detach())
    print(f"{geo}: penalty C call {got_pen:.6f}  float64 oracle {ref_pen:.6f}  ({abs(got_pen - ref_pen) / ref_pen / 2.0 ** -7:.2f} of the bound)")
    assert abs(got_pen - ref_pen) <= 2.0 ** -7 * abs(ref_pen)
    gmax = max(float(p.grad.abs().max()) for p in st.values() if p.grad is not None)
    floor = 2.0 ** -10 * gmax
    bad, skipped, worst = [], [], (0.0, 0.0)
    for name, (off, shape) in fl.slots.items():
        n = int(torch.tensor(shape).prod())
        a = got[off:off + n]
        gr = st["vit." + name].grad
        b = torch.zeros(n, dtype=F64) if gr is None else gr.reshape(-1)
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        if not err <= 2.0 ** -4 * scale + floor:
            bad.append((name, "max", err, scale))
        if scale < 1e-9 * gmax:   # float64 round-off of an exact zero: nothing to project on
            skipped.append(name)
            continue
        proj = float((a * b).sum() / (b * b).sum())
        worst = (max(worst[0], err / scale / 2.0 ** -4), max(worst[1], abs(proj - 1) / 2.0 ** -6))
        if not abs(proj - 1) <= 2.0 ** -6:
            bad.append((name, "projection", proj, scale))
    print(f"{geo}: worst max-error {worst[0]:.2f} and projection {worst[1]:.2f} of their bounds; skipped {skipped}")
    assert not bad, bad
    # the key bias of each block, and the last bias, which the input gradient cannot depend on
    assert all(s.endswith("attention.keys.bias") or s == "classifier.fc2.bias" for s in skipped) and len(skipped) <= L + 1, skipped
