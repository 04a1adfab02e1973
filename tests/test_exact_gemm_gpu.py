"""The GEMM family on exact inputs, bit for bit (tests/exact_util.py).

Counting regime: small integers whose every partial sum is exact in fp32, so each output must equal the fp64 result rounded
once to its dtype, whatever the kernel's summation order; one dropped, doubled or misplaced product is an integer error of at
least 1.  Each shape table names the kernel its shapes reach (exact_util.fwd_target / dgrad_target / wgrad_target mirror the
dispatch of csrc/gemm.hip, gemm_wr.hip and gemm_tn.hip).  Every output has guard rows of sentinel behind it, inside the same
allocation; only shapes the C ABI accepts are launched.
"""
import math

import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CUDA = "cuda"


def _check_out(buf, rows, want, what):
    X.assert_written(buf, rows, what)
    X.assert_bitwise(buf[:rows], want, what)
    X.assert_guard(buf, rows, what)


# ------------------------------------------------------------------------------------------------------- vg_linear_fwd
def _fwd_inputs(M, N, K, seed, br, wide=False):
    g = X.gen(seed, CUDA)
    if wide:  # results beyond 256: the bf16 output must be the round-to-nearest-even of the exact fp32 sum
        lim = 16 if K <= 96 else 4
        A, W = X.counting((M, K), g, -lim, lim), X.counting((N, K), g, -lim, lim)
    else:
        dens = 1.0 if K <= 96 else 0.5
        A, W = X.counting((M, K), g, -1, 1, dens), X.counting((N, K), g, -1, 1, dens)
    bias = X.counting((N,), g, -8, 8) if br else None
    res = X.counting((M, N), g, -8, 8) if br else None
    return A, W, bias, res


def _run_fwd(A, W, bias, res, act=0, pre=None):
    u = X.gpu()
    M, K = A.shape
    N = W.shape[0]
    dA, dW = A.to(BF), W.to(BF)
    db = None if bias is None else bias.float()
    dr = None if res is None else res.to(BF)
    C = X.guarded(M, N, BF, CUDA)
    P = X.guarded(M, N, BF if pre == "bf16" else F32, CUDA) if pre else None
    u.call("vg_linear_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), u.ptr(dr), u.ptr(C),
           u.ptr(P if pre == "bf16" else None), u.ptr(P if pre == "f32" else None), M, N, K, act, 0.0, u.stream())
    u.sync()
    return C, P


def _fwd_one(M, N, K, br, pre, wide=False):
    A, W, bias, res = _fwd_inputs(M, N, K, M * 7 + N * 3 + K + br, br, wide)
    pre64 = X.check_exact_gemm(A, W.t(), [] if bias is None else [bias.expand(M, N)], out_dtype=F32 if wide else BF,
                               what="pre")
    y = X.check_exact_gemm(A, W.t(), [] if bias is None else [bias.expand(M, N), res], out_dtype=F32 if wide else BF)
    C, P = _run_fwd(A, W, bias, res, 0, pre)
    tgt = X.fwd_target(M, N, K, 0, pre, bool(br))
    _check_out(C, M, X.rne(y, BF), f"C [{tgt}]")
    if pre:
        _check_out(P, M, X.rne(pre64, BF if pre == "bf16" else F32), f"pre_{pre} [{tgt}]")


# (bias + residual, pre-activation output): plain and bias + residual without a second output run on wr where the shape
# allows (its NONE and NONE + RES instances); an fp32 pre-activation, or a bf16 one next to a residual, moves them to a tiled kernel
FWD_VARIANTS = ((0, None), (1, None), (1, "f32"), (1, "bf16"))


@pytest.mark.parametrize("shape", X.FWD_SHAPES, ids=lambda s: f"N{s[1]}-K{s[2]}-M{s[0][0]}x{len(s[0])}")
def test_linear_fwd_counting(shape):
    """plain; bias + residual; bias + residual with the fp32 pre-activation; with the bf16 pre-activation"""
    Ms, N, K = shape
    X.collect([(M, br, pre) for M in Ms for br, pre in FWD_VARIANTS], lambda c: _fwd_one(c[0], N, K, c[1], c[2]))


WIDE_SHAPES = [(X.M_RESIDUES, 136, 48), ([4100], 768, 48), ([1024, 1120, 16640], 384, 384)]


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=lambda s: f"N{s[1]}-K{s[2]}")
def test_linear_fwd_rounds_to_nearest_even(shape):
    """exact integer sums up to a few thousand: the bf16 outputs are their round-to-nearest-even, bit for bit
    (tiled128 / tiled256; the last shape's launches without a pre-activation output reach wr)"""
    Ms, N, K = shape
    X.collect([(M, br, pre) for M in Ms for br, pre in FWD_VARIANTS], lambda c: _fwd_one(c[0], N, K, c[1], c[2], wide=True))


# ----------------------------------------------------------------------------------------------------- vg_linear_dgrad
def _dgrad_one(M, N, K, mode):
    u = X.gpu()
    g = X.gen(M * 5 + N + K * 11 + mode, CUDA)
    dens = 1.0 if N <= 200 else 0.5
    dY, W = X.counting((M, N), g, -1, 1, dens), X.counting((N, K), g, -1, 1, dens)
    y = X.check_exact_gemm(dY, W, out_dtype=BF)
    Z = None
    if mode == 7:  # dX *= Z, Z small integers: still exact, still representable (asserted)
        Z = X.counting((M, K), g, -2, 2)
        y = y * Z
        assert torch.equal(y, y.to(BF).double())
    dX = X.guarded(M, K, BF, CUDA)
    dZ = None if Z is None else Z.to(BF)
    a, b = dY.to(BF), W.to(BF)  # held until the kernel has run: a bare temporary's memory could be reused before it
    u.call("vg_linear_dgrad", u.ptr(a), u.ptr(b), u.ptr(dX), M, N, K, mode, u.ptr(dZ), None, 0.0, u.stream())
    u.sync()
    _check_out(dX, M, X.rne(y, BF), f"dX mode {mode} [{X.dgrad_target(M, N, K)}]")


@pytest.mark.parametrize("shape", X.DGRAD_SHAPES, ids=lambda s: f"N{s[1]}-K{s[2]}-M{s[0][0]}x{len(s[0])}")
@pytest.mark.parametrize("mode", [0, 7])
def test_linear_dgrad_counting(shape, mode):
    Ms, N, K = shape
    X.collect(Ms, lambda M: _dgrad_one(M, N, K, mode))


# ----------------------------------------------------------------------------------------------------- vg_linear_wgrad
def _wgrad_inputs(M, N, K, seed):
    g = X.gen(seed, CUDA)
    dens = 1.0 if M <= 64 else (0.5 if M <= 4096 else 0.25)
    return X.counting((M, N), g, -1, 1, dens), X.counting((M, K), g, -1, 1, dens)


def _wgrad_run(dY, Xa, splits, accumulate, dW0=None):
    u = X.gpu()
    M, N = dY.shape
    K = Xa.shape[1]
    L = u._lib.lib()
    ns = L.vg_linear_wgrad_slab_floats(N, K, splits)
    assert ns == splits * N * K
    slab = torch.empty(ns, dtype=F32, device=CUDA)
    dW = X.guarded(N, K, F32, CUDA)
    if dW0 is not None:
        dW[:N] = dW0.float()
    a, b = dY.to(BF), Xa.to(BF)
    u.call("vg_linear_wgrad", u.ptr(a), u.ptr(b), u.ptr(dW), u.ptr(slab), ns, M, N, K, splits, accumulate,
           u.stream())
    u.sync()
    return dW


# (M, N, K): tiled_tn (N, K not multiples of 128 / 384), tn384 (K % 384 == 0), tn512 (K % 512 == 0)
WGRAD_SPLIT_SHAPES = [(1000, 136, 200), (77, 8, 24), (2080, 128, 384), (2048, 128, 512)]


@pytest.mark.parametrize("shape", WGRAD_SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_wgrad_every_split(shape):
    """splits 1 .. 64 (the launcher drops empty slices: ragged last slices at most of them), then accumulate = 1 on top of
    an integer-valued dW"""
    M, N, K = shape
    dY, Xa = _wgrad_inputs(M, N, K, M + N + K)
    y = X.check_exact_gemm(dY.t(), Xa, out_dtype=F32)
    tgt = X.wgrad_target(M, N, K)

    def one(splits):
        _check_out(_wgrad_run(dY, Xa, splits, 0), N, X.rne(y, F32), f"dW splits {splits} [{tgt}]")
    X.collect(list(range(1, 65)), one)
    dW0 = X.counting((N, K), X.gen(3, CUDA), -1000, 1000)
    for splits in (1, 5):
        _check_out(_wgrad_run(dY, Xa, splits, 1, dW0), N, X.rne(y + dW0, F32), f"dW accumulate splits {splits} [{tgt}]")


# the step's weight gradients (M = B * S of C2): QKV, out-proj, fc1, fc2
@pytest.mark.parametrize("M", [16640, 33280])
def test_linear_wgrad_step_shapes(M):
    def one(c):
        N, K, splits = c
        dY, Xa = _wgrad_inputs(M, N, K, N + K + M)
        y = X.check_exact_gemm(dY.t(), Xa, out_dtype=F32)
        _check_out(_wgrad_run(dY, Xa, splits, 0), N, X.rne(y, F32), f"dW [{X.wgrad_target(M, N, K)}]")
    X.collect([(1152, 384, 8), (384, 384, 16), (1536, 384, 4), (384, 1536, 4), (384, 1536, 64)], one)


@pytest.mark.parametrize("M", [1040, 16640])
def test_linear_wgrad_group(M):
    """a block's four weight gradients as one grouped launch and one fold, regions tiling the destination exactly"""
    u = X.gpu()
    shapes = [(1152, 384), (384, 384), (1536, 384), (384, 1536)]
    ins = [_wgrad_inputs(M, N, K, 17 * j + M) for j, (N, K) in enumerate(shapes)]
    offs, at = [], 0
    for N, K in shapes:
        offs.append(at)
        at += N * K
    region = at
    want = torch.cat([X.check_exact_gemm(dY.t(), Xa, out_dtype=F32).reshape(-1) for dY, Xa in ins])
    import ctypes as C
    n = len(shapes)
    dYs = [dY.to(BF) for dY, _ in ins]
    Xs = [Xa.to(BF) for _, Xa in ins]
    P = C.c_void_p * n
    for splits, acc in ((1, 0), (4, 0), (4, 1)):
        slab = torch.empty(splits * region, dtype=F32, device=CUDA)
        dst = X.guarded(region // 384, 384, F32, CUDA)
        base = X.counting((region // 384, 384), X.gen(splits, CUDA), -50, 50) if acc else None
        if acc:
            dst[:region // 384] = base.float()
        u.call("vg_linear_wgrad_group", n, P(*[t.data_ptr() for t in dYs]), P(*[t.data_ptr() for t in Xs]),
               (C.c_int * n)(*[s[0] for s in shapes]), (C.c_int * n)(*[s[1] for s in shapes]), (C.c_longlong * n)(*offs),
               M, splits, u.ptr(slab), slab.numel(), u.ptr(dst), region, acc, u.stream())
        u.sync()
        w = want if not acc else want + base.reshape(-1)
        _check_out(dst, region // 384, X.rne(w, F32).reshape(-1, 384), f"group splits {splits} acc {acc}")


# ---------------------------------------------------------------------------------------- vg_linear_ln_fwd (full rows)
def row_call(E, name, *args):
    """a full-row entry point at width E: the plain name at 384, the `_e` form (which takes the width) otherwise"""
    u = X.gpu()
    if E == 384:
        u.call(name, *args)
    else:
        u.call(name + "_e", E, *args)


def _pack(E, W, K, transposed=False):
    """the packed stage images of W: [E, K] (forward), or transposed [K, E] (the input gradient dX = dY W)"""
    u = X.gpu()
    L = u._lib.lib()
    n = L.vg_row_pack_elems(K) if E == 384 else L.vg_row_pack_elems_e(E, K)
    assert n == E * K
    Wp = torch.empty(n, dtype=BF, device=CUDA)
    dW = W.to(BF)
    row_call(E, "vg_row_pack_weight", u.ptr(dW), W.shape[1], K, 1 if transposed else 0, u.ptr(Wp), u.stream())
    return Wp


MEAN_TOL = 2.0 ** -21  # of max|Y| over the row: the sum of exact integers is exact, then one multiply by fp32(1/E)
RSTD_TOL = 2.0 ** -16  # relative: fp32 sum of E squared deviations, eps added by fma, rsqrtf
YN_FLOOR = 2.0 ** -14  # of the magnitudes the fp32 arithmetic of Yn rounds relative to: its share where the terms cancel


def plain_yn(gam, bet):
    """z = (y - mean) rstd -> (Yn, its fp32 floor) of the plain LayerNorm"""
    def yn_of(z):
        zg = z * gam
        return zg + bet, YN_FLOOR * (zg.abs() + bet.abs())
    return yn_of


def check_row_fwd(y, Y, Yn, mean, rstd, M, yn_of):
    """the outputs of a full-row forward against the exact sum y (fp64): Y bitwise, mean / rstd against the fp64 statistics of y,
    Yn within one bf16 ulp of yn_of((y - mean) rstd) plus the fp32 arithmetic's share; nothing unwritten, no guard row touched"""
    _check_out(Y, M, X.rne(y, BF), "Y")
    for t, w in ((Yn, "Yn"), (mean, "mean"), (rstd, "rstd")):
        X.assert_written(t, M, w)
        X.assert_guard(t, M, w)
    mu = y.mean(1)
    var = ((y - mu[:, None]) ** 2).mean(1)
    rs = 1.0 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=F32)))
    em = (mean[:M, 0].double() - mu).abs()
    assert bool((em <= MEAN_TOL * y.abs().amax(1)).all()), f"mean off by {float(em.max())}"
    er = ((rstd[:M, 0].double() - rs) / rs).abs()
    assert bool((er <= RSTD_TOL).all()), f"rstd off by {float(er.max())} relative"
    yn, floor = yn_of((y - mu[:, None]) * rs[:, None])
    # one bf16 ulp of the exact value, plus the fp32 arithmetic's share where the terms cancel
    X.assert_ulps(Yn[:M], yn, "Yn", 1.0, floor=floor)


@pytest.mark.parametrize("E", [384, 512])
@pytest.mark.parametrize("K", [384, 1536])
def test_linear_ln_fwd_counting(E, K):
    """Y = res + A W^T + bias bitwise; mean / rstd against fp64 statistics of that Y; Yn within one bf16 ulp.
    units = M / 16 from 1 to 40 (every split of up to 40 units over workgroups of 1 or 2: tiles of 1 and 2 m-tiles), then the
    step's M = 16 640 (tiles of 4 and 5 m-tiles).  Every other tile height, the dropout and the other epilogues of this kernel:
    tests/test_exact_row_gpu.py."""
    u = X.gpu()
    g = X.gen(E + K, CUDA)
    dens = 0.5
    W = X.counting((E, K), g, -1, 1, dens)
    Wp = _pack(E, W, K)
    bias = X.counting((E,), g, -8, 8)
    gam = 1.0 + X.dyadic((E,), g, 16, 4)
    bet = X.dyadic((E,), g, 16, 8)
    dbias, dg, dbt = bias.float(), gam.float(), bet.float()

    def one(c):
        M, with_res = c
        gg = X.gen(100003 + M * 3 + with_res, CUDA)  # a seed apart from the weights': A must not repeat W
        A = X.counting((M, K), gg, -1, 1, dens)
        res = X.counting((M, E), gg, -8, 8) if with_res else None
        y = X.check_exact_gemm(A, W.t(), [bias.expand(M, E)] + ([res] if with_res else []), out_dtype=BF)
        Y, Yn = X.guarded(M, E, BF, CUDA), X.guarded(M, E, BF, CUDA)
        mean, rstd = X.guarded(M, 1, F32, CUDA), X.guarded(M, 1, F32, CUDA)
        dA, dr = A.to(BF), (res.to(BF) if with_res else None)
        row_call(E, "vg_linear_ln_fwd", u.ptr(dA), u.ptr(Wp), u.ptr(dbias), u.ptr(dr), u.ptr(Y), u.ptr(Yn),
                 u.ptr(mean), u.ptr(rstd), u.ptr(dg), u.ptr(dbt), M, K, 1e-5, 0.0, 0, 0, None, u.stream())
        u.sync()
        check_row_fwd(y, Y, Yn, mean, rstd, M, plain_yn(gam, bet))

    X.collect([(16 * un, r) for un in range(1, 41) for r in (0, 1)] + [(16640, 1), (16640, 0)], one)


# ----------------------------------------------------------------------------------------------------------- fp32 GEMMs
F32_M, F32_N, F32_K = [1, 3, 17, 64, 130], [1, 5, 31, 64, 129], [1, 3, 7, 13, 64, 67, 130]


def test_linear_f32_fwd_dgrad_counting():
    """vg_linear_f32_fwd (+ bias + residual) and vg_linear_f32_dgrad: integer fp32 inputs, any M, N, K >= 1, bitwise"""
    u = X.gpu()

    def one(c):
        M, N, K = c
        g = X.gen(M * 1000 + N * 10 + K, CUDA)
        A, W = X.counting((M, K), g, -8, 8), X.counting((N, K), g, -8, 8)
        bias, res = X.counting((N,), g, -99, 99), X.counting((M, N), g, -99, 99)
        y = X.check_exact_gemm(A, W.t(), [bias.expand(M, N), res], out_dtype=F32)
        Y = X.guarded(M, N, F32, CUDA)
        fA, fW, fb, fr = A.float(), W.float(), bias.float(), res.float()
        u.call("vg_linear_f32_fwd", u.ptr(fA), u.ptr(fW), u.ptr(fb), u.ptr(fr), u.ptr(Y), None,
               M, N, K, 0, 0.0, 0, 0, None, u.stream())
        dY = X.counting((M, N), g, -8, 8)
        dx = X.check_exact_gemm(dY, W, out_dtype=F32)
        dX = X.guarded(M, K, F32, CUDA)
        fdY = dY.float()
        u.call("vg_linear_f32_dgrad", u.ptr(fdY), u.ptr(fW), None, u.ptr(dX), M, N, K, 0, u.stream())
        u.sync()
        _check_out(Y, M, X.rne(y, F32), "f32 fwd")
        _check_out(dX, M, X.rne(dx, F32), "f32 dgrad")

    X.collect([(M, N, K) for M in F32_M for N in F32_N for K in F32_K], one)


def test_linear_f32_wgrad_counting():
    """vg_linear_f32_wgrad: dW += dY^T X and db += colsum(dY) on integer-valued dW / db, bitwise"""
    u = X.gpu()
    L = u._lib.lib()

    def one(c):
        M, N, K = c
        g = X.gen(M * 1000 + N * 10 + K + 1, CUDA)
        dY, Xa = X.counting((M, N), g, -8, 8), X.counting((M, K), g, -8, 8)
        dW0, db0 = X.counting((N, K), g, -999, 999), X.counting((N,), g, -999, 999)
        w = X.check_exact_gemm(dY.t(), Xa, [dW0], out_dtype=F32)
        b = dY.sum(0) + db0
        ns = L.vg_linear_f32_wgrad_slab_floats(M, N, K)
        assert ns > 0
        slab = torch.empty(ns, dtype=F32, device=CUDA)
        dW = X.guarded(N, K, F32, CUDA)
        dW[:N] = dW0.float()
        db = X.guarded(N, 1, F32, CUDA)
        db[:N, 0] = db0.float()
        fdY, fX = dY.float(), Xa.float()
        u.call("vg_linear_f32_wgrad", u.ptr(fdY), u.ptr(fX), u.ptr(dW), u.ptr(db), u.ptr(slab), ns, M, N, K,
               u.stream())
        u.sync()
        _check_out(dW, N, X.rne(w, F32), "f32 dW")
        _check_out(db, N, X.rne(b, F32)[:, None], "f32 db")

    X.collect([(M, N, K) for M in F32_M + [1000, 4099] for N in F32_N for K in (1, 7, 64, 130)], one)


# ----------------------------------------------------------------------------------------- dyadic regime: epilogues
def _gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


GELU_RANGE = 3.5  # |pre| bound of the GELU probes.  The kernel's Phi is 0.5 + 0.5 erf(x / sqrt 2) with the Abramowitz-Stegun
                  # polynomial for erf (vg_common.h vg_phi_e, documented there): an ABSOLUTE error of ~1.5e-7, which below
                  # x = -3.5 exceeds half a bf16 ulp of the tiny x * Phi(x).  A documented approximation, not a defect.


def _dyadic_inputs(M, N, K, seed):
    """A = i/8, W = j/16, bias = k/64: pre-activations on the 1/128 grid, exact in fp32, |pre| <= GELU_RANGE (asserted)"""
    g = X.gen(seed, CUDA)
    wl = 4 if K <= 96 else 2
    A, W = X.dyadic((M, K), g, 8, 8, 0.5), X.dyadic((N, K), g, 16, wl, 0.5)
    bias = X.dyadic((N,), g, 64, 32)
    pre = X.check_exact_gemm(A, W.t(), [bias.expand(M, N)], out_dtype=F32, what="pre")
    assert float(pre.abs().max()) <= GELU_RANGE, float(pre.abs().max())
    return A, W, bias, pre


# (M list, N, K, act, pre): tiled128 / tiled256 (GELU only: tanh is not a light epilogue) / wr (GELU with a bf16
# pre-activation, tanh with none)
ACT_SHAPES = [(X.M_RESIDUES, 136, 96, 1, "f32"), (X.M_RESIDUES, 136, 96, 3, "f32"), ([4100], 768, 96, 1, "f32"),
              ([1024, 1120], 256, 384, 1, "bf16"), ([1024, 1120, 288], 256, 384, 3, None), ([33, 257], 256, 384, 3, "bf16")]


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: f"act{s[3]}-N{s[1]}-K{s[2]}-{s[4]}")
def test_linear_fwd_activation_dyadic(shape):
    """act 1 (GELU) and 3 (tanh): the pre-activation bitwise, the output within one bf16 ulp of the fp64 function of it"""
    Ms, N, K, act, pre = shape
    f = _gelu64 if act == 1 else torch.tanh

    def one(M):
        A, W, bias, p64 = _dyadic_inputs(M, N, K, M + N + K + act)
        C, P = _run_fwd(A, W, bias, None, act, pre)
        tgt = X.fwd_target(M, N, K, act, pre)
        X.assert_written(C, M, "C")
        X.assert_guard(C, M, "C")
        X.assert_ulps(C[:M], f(p64), f"act {act} [{tgt}]")
        if pre:
            _check_out(P, M, X.rne(p64, BF if pre == "bf16" else F32), f"pre [{tgt}]")
    X.collect(Ms, one)


GELU_SHAPES = [(X.M_RESIDUES, 136, 96), ([4100], 768, 96), ([256, 1024, 1120], 256, 384), ([16640], 1536, 384)]


@pytest.mark.parametrize("shape", GELU_SHAPES, ids=lambda s: f"N{s[1]}-K{s[2]}")
def test_linear_gelu_fwd_byte_codes(shape):
    """vg_linear_gelu_fwd: C within one bf16 ulp of gelu(pre), and the byte code exactly round(200 gelu'(pre)) + 27 - off by
    one only where 200 gelu'(pre) lies within 1e-4 of a rounding boundary"""
    u = X.gpu()
    Ms, N, K = shape

    def one(M):
        A, W, bias, p64 = _dyadic_inputs(M, N, K, 3 * M + N + K)
        C = X.guarded(M, N, BF, CUDA)
        D = X.guarded(M, N, torch.uint8, CUDA)
        dA, dW, db = A.to(BF), W.to(BF), bias.float()
        u.call("vg_linear_gelu_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), u.ptr(C), u.ptr(D), M, N, K,
               u.stream())
        u.sync()
        tgt = X.fwd_target(M, N, K, 1, "bf16")
        X.assert_written(C, M, "C")
        X.assert_guard(C, M, "C")
        X.assert_guard(D, M, "dcode")
        X.assert_ulps(C[:M], _gelu64(p64), f"gelu [{tgt}]")
        t = 200.0 * _gelu_grad64(p64)
        want = torch.round(t) + 27
        got = D[:M].double()
        near = ((t - torch.floor(t)) - 0.5).abs() < 1e-4
        bad = (got != want) & ~(near & ((got - want).abs() <= 1))
        n = int(bad.sum())
        if n:
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"dcode [{tgt}]: {n} codes wrong; first at {i}: got {int(got[i])} want {int(want[i])} "
                                 f"(pre {float(p64[i])})")
    X.collect(Ms, one)
