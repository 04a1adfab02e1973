"""The float64 restatements of the first-order normalisation kernels (tests/norm_ref.py), their bounds and their checkers, on the CPU.

(1) restatement == torch autograd of F.layer_norm in float64, to 1e-12 of each tensor's maximum;
(2) the float32 emulation of every function passes the assertions that tests/test_norm_gpu.py makes, at every width: if a derived
    kappa were too small for the operations the kernel performs, it would show here without a GPU;
(3) the mutation table: every planted mistake, through the same emulation, fails one of those assertions;
(4) the floors of the fits of dx and dh, which the GPU test allows 4 x of;
(5) the return codes of the entry points, host only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import norm_ref as N
from second_order_ref import LN_EPS, fit_terms

F64 = torch.float64
ROWS_SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 130]
ROWS_LARGE = [8191, 8192, 8193, 16640]


def _close(a, b, what, rel=1e-12):
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-300, f"{what}: {err:.3e} > {rel:g} * {scale:.3e}"


# ------------------------------------------------------------------------------------------------ (1) restatement == autograd
@pytest.mark.parametrize("E", [128, 384, 1024])
@pytest.mark.parametrize("with_gres", [False, True])
def test_layernorm_restatement_equals_autograd(E, with_gres):
    R = 24
    inp = N.norm_inputs(R, E, 3)
    x = inp["x"].clone().requires_grad_(True)
    gam, bet = inp["gamma"].clone().requires_grad_(True), inp["beta"].clone().requires_grad_(True)
    y = F.layer_norm(x, (E,), gam, bet, LN_EPS)
    y.backward(inp["dy"])
    f = N.ln_fwd(inp["x"], inp["gamma"], inp["beta"])
    b = N.ln_bwd(inp["dy"], inp["x"], f["mean"], f["rstd"], inp["gamma"], inp["gres"] if with_gres else None)
    _close(f["y"], y.detach(), "y")
    _close(f["mean"], inp["x"].mean(-1), "mean")
    _close(f["rstd"], 1.0 / torch.sqrt(inp["x"].var(-1, unbiased=False) + LN_EPS), "rstd")
    _close(b["dx"], x.grad + (inp["gres"] if with_gres else 0.0), "dx")
    _close(sum(b["dx_terms"]), x.grad, "sum of the three terms")
    _close(b["dgamma"], gam.grad, "dgamma")
    _close(b["dbeta"], bet.grad, "dbeta")
    assert len(b["dx_terms"]) == 3
    for n in ("y",):
        assert bool((f["mag_" + n] >= f[n].abs() * (1 - 1e-9)).all())
    for n in ("dx", "dgamma", "dbeta"):
        assert bool((b["mag_" + n] >= b[n].abs() * (1 - 1e-9)).all()), n


@pytest.mark.parametrize("E", [128, 384, 1024])
@pytest.mark.parametrize("T,with_gres", [(0, False), (0, True), (8, False), (8, True), (7, True)])
def test_sln_restatement_equals_autograd(E, T, with_gres):
    """T = 7: R = 24 is no multiple of the broadcast rows"""
    R = 24
    inp = N.norm_inputs(R, E, 4, T)
    rows = torch.arange(R) % T if T else torch.arange(R)
    hx = inp["h"][rows].clone().requires_grad_(True)   # an expanded leaf: the gradient per row, before any sum over the batch
    w = inp["w"].clone().requires_grad_(True)
    lw, lb = inp["lw"].clone().requires_grad_(True), inp["lb"].clone().requires_grad_(True)
    sc = torch.tensor([inp["gs"], inp["bs"]], dtype=F64, requires_grad=True)
    y = w * (sc[0] * F.layer_norm(hx, (E,), lw, lb, LN_EPS) + sc[1])
    y.backward(inp["dy"])
    f = N.sln_fwd(inp["h"], inp["w"], inp["lw"], inp["lb"], inp["gs"], inp["bs"], LN_EPS, T)
    b = N.sln_bwd(inp["dy"], inp["h"], inp["w"], f["mean"], f["rstd"], inp["lw"], inp["lb"], inp["gs"], inp["bs"],
                  inp["gres"] if with_gres else None, T)
    _close(f["y"], y.detach(), "y")
    _close(f["mean"], hx.detach().mean(-1), "mean")
    _close(b["dh"], hx.grad + (inp["gres"] if with_gres else 0.0), "dh")
    for n, g in (("dw", w.grad), ("dlw", lw.grad), ("dlb", lb.grad), ("dgs", sc.grad[0]), ("dbs", sc.grad[1])):
        _close(b[n], g, n)
        assert bool((b["mag_" + n] >= b[n].abs() * (1 - 1e-9)).all()), n
    assert bool((f["mag_y"] >= f["y"].abs() * (1 - 1e-9)).all()) and bool((b["mag_dh"] >= b["dh"].abs() * (1 - 1e-9)).all())


def test_kappas_count_what_their_docstrings_say():
    for E in N.WIDTHS:
        nv = E // 128
        assert N.kappa_stat(E) == 8 * nv + 6 and N.kappa_var(E) == 8 * nv + 11
        assert N.kappa_fwd(E) == 16 * nv + 19 + 2 * N.RSQRT_ULPS and N.kappa_fwd(E, True) == N.kappa_fwd(E) + 3
        assert N.kappa_dx(E) == 4 * nv + 16 and N.kappa_dx(E, True) == 4 * nv + 18
    assert [N.bwd_parts(R) for R in (1, 16, 17, 8192, 8193, 16640)] == [1, 1, 2, 512, 512, 512]
    assert [N.bwd_trips(R) for R in (1, 8, 9, 16, 17, 4096, 4097, 8192, 8193, 16640)] == [1, 1, 2, 2, 2, 2, 2, 2, 3, 5]
    assert N.kappa_colsums(384, 16640) == 3 + 5 + 1 + 2 + 32 + 16 and N.kappa_colsums(384, 1, True) == 5 + 1 + 1 + 2 + 1 + 16
    assert N.kappa_colsums(384, 16640, True, scalar=True) == 6 + 4 * 3 * 5 + 6 + 2 + 48
    assert N.kappa_colsum_bf16(16640) == 32 + 8 + 5 + 16 and N.kappa_dw() == 8
    assert set(N.MUTANTS) == {"unbiased_var", "eps_outside_sqrt", "one_pass_var", "drop_c1", "drop_c2", "c2_without_invE", "dgamma_without_xhat",
                              "dbeta_of_g", "gres_twice", "sln_dw_without_bs", "sln_dgs_without_lb", "sln_dy_eff_without_gs", "bcast_off_by_one"}


# --------------------------------------------------------------------------------------------- (2) the emulation is accepted
def _bcast_rows(R, seed):
    """SLN cases of the emulation: odd seeds broadcast h (T = 16 divides 1040; T = 5 does not divide 17), even seeds do not"""
    return 0 if seed % 2 == 0 else (16 if R == 1040 else 5)


@pytest.mark.parametrize("E", N.WIDTHS)
def test_float32_emulation_passes_the_gpu_assertions(E):
    """R = 17 and 1040, 16 seeds: LayerNorm and SLN, forward and backward, with gres and without"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    stats = {}

    def one(case):
        R, seed = case
        inp = N.norm_inputs(R, E, seed)
        refs = N.ln_refs(inp)
        failed = N.run_assertions(N.ln_assertions(N.ln_emulated(inp, refs), refs, inp, R, E), stats)
        T = _bcast_rows(R, seed)
        inp = N.norm_inputs(R, E, seed, T)
        refs = N.sln_refs(inp, T)
        failed += N.run_assertions(N.sln_assertions(N.sln_emulated(inp, refs, T), refs, inp, R, E), stats)
        assert not failed, "\n".join(failed)
    X.collect([(R, seed) for R in (17, 1040) for seed in range(16)], one, f"E {E} (R, seed) ")
    print(f"E {E}: worst err / limit of the float32 emulation:", {k: round(v, 3) for k, v in stats.items()})


@pytest.mark.parametrize("R,N_", [(2080, 384), (257, 264), (9, 8)])
def test_float32_emulation_of_colsum_bf16_passes(R, N_):
    g = X.gen(R + N_)
    x = torch.randn(R, N_, generator=g, dtype=F64).to(X.BF).double()
    worst = N.assert_elementwise(N.colsum_bf16_f32(x), x.sum(0), x.abs().sum(0), N.kappa_colsum_bf16(R), "colsum_bf16", rel=0.0)
    ints = X.counting((R, N_), g, -4, 4)
    X.assert_bitwise(N.colsum_bf16_f32(ints), X.rne(ints.sum(0), torch.float32), "colsum_bf16 of integers")
    print(f"R {R} N {N_}: worst err / limit {worst:.3f}")


# ------------------------------------------------------------------------------------------------------- (3) mutation table
def test_mutation_table():
    """E = 384, R = 1040: every mutant of N.MUTANTS through the float32 emulation must fail an assertion of the GPU test; one_pass_var
    must fail on the rows with mean 8 and std 2^-5 taken alone."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    R, E, T = 1040, 384, 16
    ln_inp = N.norm_inputs(R, E, 1)
    ln_ref = N.ln_refs(ln_inp)
    sln = {t: (N.norm_inputs(R, E, 1, t),) for t in (0, T)}
    sln = {t: (i[0], N.sln_refs(i[0], t)) for t, i in sln.items()}
    caught = {}

    def one(mut):
        fam = N.MUTANTS[mut]
        failed = []
        if fam in ("fwd", "bwd"):
            failed += N.run_assertions(N.ln_assertions(N.ln_emulated(ln_inp, ln_ref, mut), ln_ref, ln_inp, R, E))
        else:
            t = T if fam == "bcast" else 0
            inp, refs = sln[t]
            failed += N.run_assertions(N.sln_assertions(N.sln_emulated(inp, refs, t, mut), refs, inp, R, E))
        caught[mut] = [f.split(":")[0] for f in failed]
        assert failed, "passes every assertion"
    X.collect(list(N.MUTANTS), one, "mutant ")
    for mut, names in caught.items():
        print(f"{mut}: caught by {names}")
    # the unmutated emulation passes the very same lists
    assert N.run_assertions(N.ln_assertions(N.ln_emulated(ln_inp, ln_ref), ln_ref, ln_inp, R, E)) == []
    for t, (inp, refs) in sln.items():
        assert N.run_assertions(N.sln_assertions(N.sln_emulated(inp, refs, t), refs, inp, R, E)) == []
    # one_pass_var on the tight rows alone
    rows = N.tight_rows(R)
    assert len(rows) >= R // 8 - 1 and float((ln_inp["x"][rows].mean(-1) - 8).abs().max()) < 0.1
    got = N.ln_emulated(ln_inp, ln_ref, "one_pass_var")["f"]
    failed = N.run_assertions(N.fwd_assertions(got, ln_ref["f"], E, rows=rows))
    assert any(f.startswith("rstd") for f in failed), f"one_pass_var passes on the rows with mean 8: {failed}"
    print("one_pass_var on the mean-8 rows alone:", [f.split(":")[0] for f in failed])


# --------------------------------------------------------------------------------------------------------- (4) fit floors
def test_fit_floors():
    """floor of |c - 1| of fit_terms on rne(sum(terms), bf16), reference against reference: worst of 16 seeds at every width, dx of the
    LayerNorm and dh of the SLN.  The GPU test allows N.fit_bound = 4 x the recorded floor.  At most the zero row of w (and a
    constant row, where its exact gradient vanishes) drops out of a fit."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for E in N.WIDTHS:
        R = N.FIT_ROWS[E]
        assert N.ln_fit_runs(R, E) and not N.ln_fit_runs(R - 1, E)
        floor = 0.0
        for seed in range(16):
            inp = N.norm_inputs(R, E, seed)
            mean, rstd = N.ln_stats(inp["x"])
            mean, rstd = mean.float(), rstd.float()
            for terms in (N.ln_bwd(inp["dy"], inp["x"], mean, rstd, inp["gamma"])["dx_terms"],
                          N.sln_bwd(inp["dy"], inp["h"], inp["w"], mean, rstd, inp["lw"], inp["lb"], inp["gs"], inp["bs"])["dh_terms"]):
                assert N.fit_dropped_rows(terms) <= 2
                floor = max(floor, float((fit_terms(sum(terms).float().to(X.BF), terms) - 1).abs().max()))
        print(f"E {E} R {R}: fit floor {floor:.2e}  bound {N.fit_bound(E):.2e}")
        assert 4 * floor <= N.fit_bound(E) <= 8 * floor, (E, R, floor)


# --------------------------------------------------------------------------------------------------------- (5) return codes
def test_return_codes_without_gpu():
    """nothing is launched: every call fails its validation first; the pointers are dummies that are never dereferenced"""
    from vit_gan_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)

    def fwd(E=384, R=8, xs=None, ys=None, null=None):
        a = [p, xs or E, p, p, p, ys or E, p, p, R, E, 1e-5, None]
        if null is not None:
            a[null] = None
        return lib.vg_layernorm_fwd(*a)

    def bwd(E=384, R=8, null=None):
        a = [p, p, p, p, p, p, p, p, R, E, None]
        if null is not None:
            a[null] = None
        return lib.vg_layernorm_bwd(*a)

    def sfwd(E=384, R=8, null=None):
        a = [p, 0, p, p, p, p, p, p, p, p, R, E, 1e-5, None]
        if null is not None:
            a[null] = None
        return lib.vg_sln_fwd(*a)

    def sbwd(E=384, R=8, null=None):
        a = [p, p, 0, p, p, p, p, p, p, p, p, p, p, 0, p, R, E, None]
        if null is not None:
            a[null] = None
        return lib.vg_sln_bwd(*a)

    for f in (fwd, bwd, sfwd, sbwd):
        for E in (64, 192, 1152):
            assert f(E=E) == -3, (f.__name__, E)
        assert f(R=0) == -3, f.__name__
    assert fwd(xs=4) == -3 and fwd(ys=12) == -3
    for f, required in ((fwd, (0, 2, 3, 4, 6, 7)), (bwd, (0, 1, 2, 3, 4, 6, 7)), (sfwd, (0, 2, 3, 4, 5, 6, 7, 8, 9)),
                        (sbwd, (0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14))):
        for i in required:
            assert f(null=i) == -1, (f.__name__, i)
    assert lib.vg_colsum_bf16(p, 12, 8, 12, p, p, 0, None) == -3 and lib.vg_colsum_bf16(p, 100, 8, 96, p, p, 0, None) == -3
    assert lib.vg_colsum_bf16(p, 96, 0, 96, p, p, 0, None) == -3
    for i in (0, 4, 5):
        a = [p, 96, 8, 96, p, p, 0, None]
        a[i] = None
        assert lib.vg_colsum_bf16(*a) == -1, i
    assert lib.vg_colsum_f32(p, 0, 16, p, 16, None, 0, None, 0, None, 0, 0, None) == -1
    assert lib.vg_colsum_f32(p, 4, 0, p, 16, None, 0, None, 0, None, 0, 0, None) == -1
    assert lib.vg_colsum_f32(None, 4, 16, p, 16, None, 0, None, 0, None, 0, 0, None) == -1
    for R in ROWS_SMALL + ROWS_LARGE:
        assert lib.vg_layernorm_bwd_parts(R) == min(-(-R // 16), 512) == N.bwd_parts(R), R
    for R in (1, 7, 8, 9, 255, 256, 257, 16641):
        assert lib.vg_colsum_bf16_parts(R) == -(-R // 256) == N.colsum_bf16_parts(R), R
