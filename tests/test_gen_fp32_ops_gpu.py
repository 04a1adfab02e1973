"""The generator's fp32 operators, each against float64 on the fp32 inputs the kernel read:

  vg_sln_f32_fwd / _bwd against norm_ref.sln_fwd / sln_bwd:  forward |d| <= 1e-5 max|ref| + 1e-4 |ref|;  backward (dh, dw, d lw, d lb)
    |d| <= 1e-3 |ref| + 1e-5 max|ref|;  the scalars d gs, d bs within 1e-4 of the 2-norm of their terms.  R in {1, 255, 256, 257, 192}:
    the edges of the column sums' 256-row chunks; E in {128, 384, 1024}; with and without the broadcast h, gres, and dw accumulate.
  vg_siren_f32_fwd / _dgrad:  Z against the fp64 product at 1e-5 max|ref|;  Y against sin(float64(float32(omega0 * Z_kernel))) within
    1e-6 absolute - 4 x the 2-ulp bound of an accurate sinf on [-1, 1]; the cosine factor of both backward forms the same way; one probe
    with |omega0 z| up to about 500.
  Two runs of every operator are bit-equal.

Inputs are of trained-network size: rows with means up to 2 and standard deviations 0.5 .. 3 (an fp32 two-pass LayerNorm is held to an
elementwise bound where it is well conditioned; the bf16 kernels' degenerate rows are tests/test_norm_gpu.py's, with magnitude bounds)."""
import pytest
import torch

import norm_ref as nr

pytestmark = pytest.mark.gpu
OMEGA = 30.0


def _ratio(got, ref, rel, of_max, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    bound = rel * ref.abs() + of_max * float(ref.abs().max())
    r = float(((got - ref).abs() / (bound + 1e-300)).max())
    assert r <= 1.0, f"{what}: {r:.3f} x the bound (max err {float((got - ref).abs().max()):.3e}, max|ref| {float(ref.abs().max()):.3e})"
    return r


def _sln_inputs(R, E, hb, seed):
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + E + hb)
    rows = hb if hb else R
    f = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    h = f(rows, E) * (0.5 + 2.5 * torch.rand(rows, 1, generator=g)) + 2.0 * (2 * torch.rand(rows, 1, generator=g) - 1)
    w = f(R, E)
    if R >= 4:
        w[R // 2] = 0.0
    lw = 1.0 + 0.3 * f(E)
    lw[3] = lw[E - 2] = 0.0
    return dict(h=h, w=w, lw=lw, lb=0.3 * f(E), gs=torch.tensor([0.7]), bs=torch.tensor([-0.4]), dy=f(R, E), gres=f(R, E), dw0=f(R, E),
                p0=[f(E), f(E), torch.zeros(1), torch.zeros(1)])  # d lw, d lb start from noise (+=); the scalars from 0


def _sln_run(u, t, R, E, hb, use_gres, acc):
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    y, mean, rstd = torch.empty(R, E, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    u.call("vg_sln_f32_fwd", u.ptr(d["h"]), hb, u.ptr(d["w"]), u.ptr(d["lw"]), u.ptr(d["lb"]), u.ptr(d["gs"]), u.ptr(d["bs"]), u.ptr(y), u.ptr(mean),
           u.ptr(rstd), R, E, 1e-5, u.stream())
    from vit_gan_amd import _lib
    part = torch.empty(_lib.lib().vg_sln_f32_bwd_part_floats(R, E), device="cuda")
    dh = torch.empty(R, E, device="cuda")
    dw = d["dw0"].clone()
    pg = [v.cuda().clone() for v in t["p0"]]
    u.call("vg_sln_f32_bwd", u.ptr(d["dy"]), u.ptr(d["h"]), hb, u.ptr(d["w"]), u.ptr(mean), u.ptr(rstd), u.ptr(d["lw"]), u.ptr(d["lb"]), u.ptr(d["gs"]),
           u.ptr(d["bs"]), u.ptr(d["gres"]) if use_gres else None, u.ptr(dh), u.ptr(dw), acc, *(u.ptr(v) for v in pg), u.ptr(part), R, E, u.stream())
    u.sync()
    return [y, mean, rstd, dh, dw] + pg


@pytest.mark.parametrize("E", [128, 384, 1024])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 3 * 64])
def test_sln_f32_vs_float64(R, E):
    import gpu_util as u
    worst = {}
    # (broadcast rows, gres, dw accumulate): 3 * 64 rows are a batch of 3 over a 64-row embedding
    variants = [(0, False, 0), (0, True, 1)] + ([(64, True, 0), (64, False, 1)] if R == 3 * 64 else [])
    for hb, use_gres, acc in variants:
        t = _sln_inputs(R, E, hb, 3)
        got = _sln_run(u, t, R, E, hb, use_gres, acc)
        again = _sln_run(u, t, R, E, hb, use_gres, acc)
        for a, b in zip(got, again):
            assert torch.equal(a, b), "two runs differ"
        y, mean, rstd, dh, dw, dlw, dlb, dgs, dbs = got
        gs, bs = float(t["gs"]), float(t["bs"])
        fw = nr.sln_fwd(t["h"], t["w"], t["lw"], t["lb"], gs, bs, bcast_rows=hb)
        tag = f"R {R} E {E} hb {hb} gres {use_gres} acc {acc}: "
        for k, v in (("y", y), ("mean", mean), ("rstd", rstd)):
            worst[k] = max(worst.get(k, 0.0), _ratio(v, fw[k], 1e-4, 1e-5, tag + k))
        bw = nr.sln_bwd(t["dy"], t["h"], t["w"], fw["mean"], fw["rstd"], t["lw"], t["lb"], gs, bs, gres=t["gres"] if use_gres else None,
                        bcast_rows=hb)
        ref_dw = bw["dw"] + (t["dw0"].double() if acc else 0.0)
        p0 = [v.double() for v in t["p0"]]
        for k, v, ref in (("dh", dh, bw["dh"]), ("dw", dw, ref_dw), ("dlw", dlw, p0[0] + bw["dlw"]), ("dlb", dlb, p0[1] + bw["dlb"])):
            worst[k] = max(worst.get(k, 0.0), _ratio(v, ref, 1e-3, 1e-5, tag + k))
        # the two scalars against the 2-norm of the terms they sum
        hx = t["h"].double().repeat(R // hb, 1) if hb else t["h"].double()
        xh = (hx - fw["mean"].unsqueeze(-1)) * fw["rstd"].unsqueeze(-1)
        dyw = t["dy"].double() * t["w"].double()
        for k, v, ref, terms, start in (("dgs", dgs, bw["dgs"], dyw * (xh * t["lw"].double() + t["lb"].double()), p0[2]), ("dbs", dbs, bw["dbs"], dyw, p0[3])):
            err = abs(float(v.double().cpu() - (start + ref)))
            norm = float(terms.norm()) + 1e-300
            assert err <= 1e-4 * norm, f"{tag}{k}: {err:.3e} against 1e-4 x {norm:.3e}"
            worst[k] = max(worst.get(k, 0.0), err / (1e-4 * norm))
    print(f"R {R} E {E}: worst share of each bound", {k: f"{v:.3f}" for k, v in worst.items()})


def test_sln_f32_without_parameter_sums():
    """dlw = dlb = dgs = dbs = NULL: dh and dw only, bit-equal to the full call's"""
    import gpu_util as u
    R, E = 70, 256
    t = _sln_inputs(R, E, 0, 5)
    full = _sln_run(u, t, R, E, 0, True, 0)
    d = {k: v.cuda() for k, v in t.items() if torch.is_tensor(v)}
    dh, dw = torch.empty(R, E, device="cuda"), torch.empty(R, E, device="cuda")
    u.call("vg_sln_f32_bwd", u.ptr(d["dy"]), u.ptr(d["h"]), 0, u.ptr(d["w"]), u.ptr(full[1]), u.ptr(full[2]), u.ptr(d["lw"]), u.ptr(d["lb"]),
           u.ptr(d["gs"]), u.ptr(d["bs"]), u.ptr(d["gres"]), u.ptr(dh), u.ptr(dw), 0, None, None, None, None, None, R, E, u.stream())
    u.sync()
    assert torch.equal(dh, full[3]) and torch.equal(dw, full[4])


def _siren_case(M, N, K, scale, seed):
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + N * 3 + K)
    X = torch.randn(M, K, generator=g) * scale
    W = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    b = (torch.rand(N, generator=g) * 2 - 1) / K ** 0.5
    dY = torch.randn(M, N, generator=g)
    aux = torch.randn(M, K, generator=g) * scale * 0.6  # the pre-activation of the layer below: the size of Z
    return X, W, b, dY, aux


def _sin_ref(Zk):
    """sin and cos of float64(float32(omega0 * z)): the product formed in fp32, as torch forms it, from the kernel's own z"""
    arg = (torch.tensor(OMEGA, dtype=torch.float32) * Zk.float().cpu()).double()
    return torch.sin(arg), torch.cos(arg), arg


def _siren_check(u, M, N, K, scale, seed):
    X, W, b, dY, aux = (v.cuda() for v in _siren_case(M, N, K, scale, seed))

    def run():
        Y, Z, dX, P, dE = (torch.empty(s, device="cuda") for s in ((M, N), (M, N), (M, K), (M, K), (M, K)))
        u.call("vg_siren_f32_fwd", u.ptr(X), u.ptr(W), u.ptr(b), u.ptr(Y), u.ptr(Z), M, N, K, OMEGA, u.stream())
        u.call("vg_siren_f32_dgrad", u.ptr(dY), u.ptr(W), u.ptr(aux), u.ptr(dX), M, N, K, OMEGA, u.stream())
        u.call("vg_linear_f32_dgrad", u.ptr(dY), u.ptr(W), None, u.ptr(P), M, N, K, 0, u.stream())  # the same product without the factor
        ones = torch.ones(M, K, device="cuda")
        u.call("vg_siren_f32_dgrad", u.ptr(ones), None, u.ptr(aux), u.ptr(dE), M, K, 0, OMEGA, u.stream())  # the elementwise form, dy = 1
        u.sync()
        return Y, Z, dX, P, dE
    out = run()
    for a, b2 in zip(out, run()):
        assert torch.equal(a, b2), "two runs differ"
    Y, Z, dX, P, dE = (v.cpu() for v in out)
    Zref = X.double().cpu() @ W.double().cpu().t() + b.double().cpu()
    top = float(Zref.abs().max())
    ez = float((Z.double() - Zref).abs().max())
    assert ez <= 1e-5 * top, f"Z: {ez:.3e} against 1e-5 x {top:.3e}"
    s, _, arg = _sin_ref(Z)
    es = float((Y.double() - s).abs().max())
    assert es <= 1e-6, f"sin: {es:.3e} at |argument| up to {float(arg.abs().max()):.1f}"
    _, c, arg_a = _sin_ref(aux)
    # elementwise form with dy = 1: dz = fl(omega0 * cosf(.)); one more rounding, 2^-24 relative, of a value of at most omega0
    ee = float((dE.double() / OMEGA - c).abs().max())
    assert ee <= 1e-6, f"cos (elementwise): {ee:.3e}"
    # epilogue form: dX = fl(P * fl(omega0 * cosf(.))) with P the kernel's own product; where |P| is not small the quotient gives the factor
    # back with two roundings of 2^-24 relative
    Pref = dY.double().cpu() @ W.double().cpu()
    _ratio(P, Pref, 1e-3, 1e-5, "dY W")
    big = P.abs() >= 0.1 * float(P.abs().max())
    assert int(big.sum()) >= max(1, P.numel() // 20)
    ec = float(((dX.double() / (OMEGA * P.double()) - c)[big]).abs().max())
    assert ec <= 1e-6, f"cos (epilogue): {ec:.3e}"
    _ratio(dX, Pref * OMEGA * c, 1e-3, 1e-5, "dX")
    return float(arg.abs().max()), float(arg_a.abs().max()), es, ee, ec


@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("N", [96, 256])
@pytest.mark.parametrize("M", [1, 17, 96])
def test_siren_f32(M, N, K):
    import gpu_util as u
    amax, _, es, ee, ec = _siren_check(u, M, N, K, 1.0, 1)
    print(f"M {M} N {N} K {K}: |omega0 z| up to {amax:.1f}; sin {es:.2e}, cos {ee:.2e} / {ec:.2e} (bound 1e-6)")


def test_siren_f32_at_hundreds_of_radians():
    """inputs scaled until |omega0 z| reaches about 500: the argument reduction of the accurate sinf / cosf, not the fast intrinsics'"""
    import gpu_util as u
    amax, aaux, es, ee, ec = _siren_check(u, 96, 256, 768, 10.0, 2)
    assert 300.0 <= amax <= 1000.0 and aaux >= 300.0, (amax, aaux)
    print(f"|omega0 z| up to {amax:.0f} / {aaux:.0f}: sin {es:.2e}, cos {ee:.2e} / {ec:.2e} (bound 1e-6)")
