"""The float64 references of the second-order kernels (tests/second_order_ref.py) and their checkers, on the CPU.

(1) closed form == torch autograd's double backward, to 1e-10, for the activations, LayerNorm and attention;
(2) the floors of the two statistical checks (fit_terms, relative RMS), measured from the reference alone on 16 seeds: the GPU tests
    allow 4 x these, and the hard-coded bounds of second_order_ref are asserted to be no looser than that;
(3) the mutation table: simulated kernel outputs (a defective closed form, rounded to bf16) must be rejected by a checker at every
    shape, the unmutated one accepted;
(4) the float64 penalty oracle that tests/test_second_order_gpu.py compares vg_vit_penalty with."""
import math

import pytest
import torch

import second_order_ref as R
from exact_util import BF, collect

F64 = torch.float64
LN_WIDTHS = [128, 256, 384, 512, 640, 768, 896, 1024]
LN_FIT_SHAPES = [(E, 8192) for E in LN_WIDTHS] + [(384, 1040), (512, 1040)]
ATTN_S = [1, 15, 16, 17, 32, 33, 48, 64, 65, 67, 68, 79, 80]


def _close(a, b, what, rel=1e-10):
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-300, f"{what}: {err:.3e} > {rel:g} * {scale:.3e}"


def bf(t):
    return t.float().to(BF)


# ------------------------------------------------------------------------------------------------ (1) closed form == autograd
@pytest.mark.parametrize("kind", ["gelu", "tanh"])
def test_activation_closed_form_equals_autograd(kind):
    g = torch.Generator().manual_seed(1)
    h = (torch.randn(4096, generator=g, dtype=F64) * 2.5).to(BF).double()
    dy, u = (torch.randn(4096, generator=g, dtype=F64).to(BF).double() for _ in range(2))
    a, c = R.act_autograd(kind, h, dy, u), R.act_closed(kind, h, dy, u)
    for n in ("d_dy", "d_h"):
        _close(c[n], a[n], f"{kind} {n}")
        assert bool((c["mag_" + n] >= c[n].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("kind", ["gelu", "tanh"])
def test_activation_reference_is_finite_and_saturates_on_every_bf16(kind):
    h = _all_finite_bf16().double()
    f, d1, d2, _, _ = R.act_funcs(kind, h)
    assert all(bool(torch.isfinite(t).all()) for t in (f, d1, d2))
    big = h.abs() >= 40
    assert float(d2[big].abs().max()) < 1e-30
    assert float((d1[big & (h > 0)] - (1.0 if kind == "gelu" else 0.0)).abs().max()) < 1e-30 and float(d1[big & (h < 0)].abs().max()) < 1e-30


def _all_finite_bf16():
    b = torch.arange(65536, dtype=torch.int32)
    b = b[(b & 0x7F80) != 0x7F80]
    assert b.numel() == 65280
    return b.to(torch.int16).view(BF)


@pytest.mark.parametrize("E", [128, 384, 1024])
def test_layernorm_closed_form_equals_autograd(E):
    u, dy, x, gam = R.ln_inputs(12, E, 3)
    mean, rstd = R.ln_stats(x)
    a, c = R.ln_autograd(u, dy, x, gam), R.ln_closed(u, dy, x, mean, rstd, gam)
    for n in ("d_dy", "d_x", "d_gamma"):
        _close(c[n], a[n], f"E {E} {n}")
        assert bool((c["mag_" + n] >= c[n].abs() * (1 - 1e-9)).all()), n
    assert len(c["d_x_terms"]) == 4 and len(c["d_dy_terms"]) == 3


@pytest.mark.parametrize("S,HE", [(1, 32), (17, 32), (65, 64), (80, 96)])
def test_attention_closed_form_equals_autograd(S, HE):
    inp = R.attn_inputs(2, 3, S, HE, 5)
    scale = 1.0 / math.sqrt(HE)
    lse = R.attn_lse(inp[0], inp[1], scale)
    a, c = R.attn_autograd(*inp, scale), R.attn_closed(*inp, lse, scale)
    for n in R.ATTN_OUTPUTS:
        if S == 1 and n != "d_do":
            assert float(a[n].abs().max()) < 1e-12 and float(c[n].abs().max()) < 1e-12   # one key: P = 1, everything else cancels
            continue
        _close(c[n], a[n], f"S {S} HE {HE} {n}")
        assert bool((c["mag_" + n] >= c[n].abs() * (1 - 1e-9)).all()), n
    # the bf16-operand variant is the same function up to the four roundings
    v = R.attn_closed(*inp, lse, scale, bf16_operands=True)
    for n in R.ATTN_OUTPUTS:
        if S > 1:
            assert R.rel_rms(v[n], c[n]) < 2.0 ** -7, n


# ------------------------------------------------------------------------------------------------------------ checkers bite
def test_checkers_reject_what_they_must():
    ref = torch.tensor([1.0, -2.0, 0.0, 4.0], dtype=F64)
    mag = ref.abs() + 1.0
    R.assert_elementwise(bf(ref), ref, mag, 10)
    for bad in (torch.tensor([1.0, -2.0, float("nan"), 4.0]), torch.tensor([1.0, -2.0, 1e-5, 4.0]), torch.tensor([1.01, -2.0, 0.0, 4.0])):
        with pytest.raises(AssertionError):
            R.assert_elementwise(bad, ref, mag, 10)
    g = torch.Generator().manual_seed(0)
    t = [torch.randn(64, 32, generator=g, dtype=F64) for _ in range(3)]
    c = R.fit_terms(t[0] + t[1] + 0.5 * t[2], t)
    assert float((c - torch.tensor([1.0, 1.0, 0.5], dtype=F64)).abs().max()) < 1e-12
    with pytest.raises(AssertionError):
        R.assert_fit(t[0] + t[1] + 0.99 * t[2], t, 1e-3)


# ------------------------------------------------------------------------------------------------------- (2) LayerNorm floors
def _ln_case(Rr, E, seed, mut=None):
    u, dy, x, gam = R.ln_inputs(Rr, E, seed)
    mean, rstd = R.ln_stats(x)
    mean, rstd = mean.float(), rstd.float()   # what kernel and reference are both handed
    return R.ln_closed(u, dy, x, mean, rstd, gam, mut=mut)


def test_layernorm_fit_floor():
    """floor of |c - 1| when rne(sum(terms), bf16) is fitted on the terms: largest of 16 seeds per shape.  The bound of the GPU test is
    R.ln_fit_bound = 4 x floor (hard-coded there, held here), and the 1/(E-1) mutant must sit at >= 10 x the floor."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for E, Rr in LN_FIT_SHAPES:
        assert R.ln_fit_runs(Rr, E)
        floor = 0.0
        for seed in range(16):
            ref = _ln_case(Rr, E, seed)
            for n in ("d_x", "d_dy"):
                floor = max(floor, float((R.fit_terms(bf(ref[n]), ref[n + "_terms"]) - 1).abs().max()))
        mutant = _ln_case(Rr, E, 0, "invE")
        dev = float((R.fit_terms(bf(mutant["d_x"]), _ln_case(Rr, E, 0)["d_x_terms"]) - 1).abs().max())
        print(f"E {E} R {Rr}: fit floor {floor:.2e}  bound {R.ln_fit_bound(Rr, E):.2e}  1/(E-1) mutant {dev:.2e} = {dev / floor:.0f} x floor")
        assert 4 * floor <= R.ln_fit_bound(Rr, E) <= 8 * floor, (E, Rr, floor)
        assert dev >= 10 * floor, (E, Rr, dev, floor)
    assert not R.ln_fit_runs(130, 384) and not R.ln_fit_runs(1040, 1024)


def _ln_checks(got, ref, Rr, E, with_fit):
    """the checks of the GPU test on d_dy / d_x / d_gamma; returns the names of the checks that failed"""
    failed = []
    for n in ("d_dy", "d_x"):
        try:
            R.assert_elementwise(got[n], ref[n], ref["mag_" + n], R.ln_kappa(E), n)
        except AssertionError:
            failed.append("elementwise " + n)
        if with_fit:
            try:
                R.assert_fit(got[n], ref[n + "_terms"], R.ln_fit_bound(Rr, E), n)
            except AssertionError:
                failed.append("fit " + n)
    return failed


@pytest.mark.parametrize("E,Rr", LN_FIT_SHAPES + [(E, Rr) for E in (128, 384, 1024) for Rr in (1, 5, 130)])
def test_layernorm_mutation_table(E, Rr):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with_fit = R.ln_fit_runs(Rr, E)
    ref = _ln_case(Rr, E, 1)
    sim = lambda r: {n: bf(r[n]) for n in ("d_dy", "d_x")}  # noqa: E731
    assert _ln_checks(sim(ref), ref, Rr, E, with_fit) == [], "the unmutated reference, rounded, must pass every check"
    survivors = []
    for mut in (R.LN_MUTANTS if with_fit else R.LN_GROSS):
        if not _ln_checks(sim(_ln_case(Rr, E, 1, mut)), ref, Rr, E, with_fit):
            survivors.append(mut)
    assert not survivors, f"E {E} R {Rr}: mutants {survivors} pass every check"


# ------------------------------------------------------------------------------------------------------- (2) attention floors
def _attn_case(S, HE, seed, B=2, H=4):
    inp = R.attn_inputs(B, H, S, HE, seed)
    scale = 1.0 / math.sqrt(HE)
    lse = R.attn_lse(inp[0], inp[1], scale).float()
    return inp, lse, scale, R.attn_closed(*inp, lse, scale, bf16_operands=True)


def test_attention_floors():
    """reference against reference: the float32 evaluation of the bf16-operand variant (output rounded to bf16) against its float64
    evaluation, worst of 16 seeds over every tested S: relative RMS per output and |c - 1| of the two-term fits.  The GPU test's bounds
    (R.ATTN_RMS_BOUND, R.ATTN_FIT_BOUND) are 4 x these."""
    for HE in (32, 64, 96):
        rms, fit = 0.0, 0.0
        for S in ATTN_S:
            for seed in range(16):
                inp, lse, scale, ref = _attn_case(S, HE, seed)
                got = R.attn_simulated(inp, lse, scale)
                for n in R.ATTN_OUTPUTS:
                    if S == 1 and n != "d_do":
                        continue
                    rms = max(rms, R.rel_rms(got[n], ref[n]))
                if S >= R.ATTN_FIT_MIN_S:
                    for n in R.ATTN_FIT_OUTPUTS:
                        fit = max(fit, float((R.fit_terms(got[n], ref[n + "_terms"]) - 1).abs().max()))
        print(f"HE {HE}: relative RMS floor {rms:.2e} (bound {R.ATTN_RMS_BOUND:.2e})  fit floor {fit:.2e} (bound {R.ATTN_FIT_BOUND:.2e})")
        assert 4 * rms <= R.ATTN_RMS_BOUND and 4 * fit <= R.ATTN_FIT_BOUND
    assert R.ATTN_RMS_BOUND <= 2.0 ** -6 and R.ATTN_FIT_BOUND <= 2.0 ** -5


def attn_checks(got, ref, S):
    failed = []
    for n in R.ATTN_OUTPUTS:
        if S == 1 and n != "d_do":
            continue
        if not R.rel_rms(got[n], ref[n]) <= R.ATTN_RMS_BOUND:
            failed.append("rms " + n)
    if S >= R.ATTN_FIT_MIN_S:
        for n in R.ATTN_FIT_OUTPUTS:
            try:
                R.assert_fit(got[n], ref[n + "_terms"], R.ATTN_FIT_BOUND, n)
            except AssertionError:
                failed.append("fit " + n)
    return failed


@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_mutation_table(HE):
    def one(S):
        inp, lse, scale, ref = _attn_case(S, HE, 2)
        assert attn_checks(R.attn_simulated(inp, lse, scale), ref, S) == [], "the unmutated simulation must pass"
        survivors = [m for m in R.ATTN_MUTANTS if not attn_checks(R.attn_simulated(inp, lse, scale, mut=m), ref, S)]
        # one key: no score gradient exists (dS = Sg = H = 0), so scale, gam and the lse row cannot matter; the mask mutant must still die
        if S == 1:
            survivors = [m for m in survivors if m == "mask_off_by_one"]
        assert not survivors, f"mutants {survivors} pass every check"
    collect(ATTN_S, one, f"HE {HE} S ")


# ---------------------------------------------------------------------------------------------------- (4) the penalty oracle
def test_penalty_oracle_runs_in_float64_and_agrees_with_float32():
    from oracle import step_oracle as so, vit_oracle as vo
    d = vo.VitDims(image=16, patch=4, embed=128, heads=4, layers=2, mlp_ratio=2, classes=1)
    torch.manual_seed(0)
    st = vo.init_vit_state(d, 5)
    for k in st:   # biases and LayerNorm parameters away from their initial 0 / 1, so that every tensor has a gradient
        if k.endswith("bias") or ".norm" in k:
            st[k] = st[k] + 0.05 * torch.randn(st[k].shape)
    g = torch.Generator().manual_seed(1)
    real, fake = (torch.rand(4, 3, 16, 16, generator=g) * 2 - 1 for _ in range(2))
    eps = torch.rand(4, 1, 1, 1, generator=g)
    out = {}
    for dt in (torch.float32, F64):
        s = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in st.items()}
        pen = so.gradient_penalty(lambda t: vo.vit_forward(s, t, d), real.to(dt), fake.to(dt), eps.to(dt))
        assert pen.dtype == dt
        pen.backward()
        assert all(p.grad is None or p.grad.dtype == dt for p in s.values())
        out[dt] = (float(pen.detach()), {k: p.grad.double() for k, p in s.items() if p.grad is not None})
    assert abs(out[torch.float32][0] - out[F64][0]) <= 1e-5 * abs(out[F64][0])
    gmax = max(float(v.abs().max()) for v in out[F64][1].values())
    for k, v in out[F64][1].items():
        assert float((out[torch.float32][1][k] - v).abs().max()) <= 1e-5 * gmax, k
