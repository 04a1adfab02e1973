"""The full-row kernel (csrc/gemm_row.hip) on exact inputs, at every tile height it is instantiated for and through all four
epilogues the C ABI reaches: vg_linear_ln_fwd, vg_linear_sln_fwd, vg_linear_dgrad_ln_bwd, vg_linear_dgrad_sln_bwd (+ `_e`).

Row counts: exact_util.ROW_M, which tests/test_exact_probes_cpu.py proves to reach tiles of 1..9 m-tiles at E = 384 and 1..6 at
E = 512, alone and several to a workgroup, under the dispatch as exact_util.row_tiles mirrors it.  K cycles over 128 / 192 / 320
(4, 6 and 10 stages of the 4-slot operand ring); 16, 48 and one tall row count run at all three.

GEMM operands are counting-regime integers (the product is an integer that bf16 holds exactly), every other operand is an integer
or a dyadic fraction, and dropout runs at p = 0.5, whose kept factor is exactly 2: the sums the kernel stores are then known bit for
bit, and a lost, doubled or misplaced row changes an integer.  What the kernel may round (the normalised rows, dx) is held to one
bf16 ulp of the fp64 value plus the stated share of its fp32 arithmetic.  The column sums are checked PER WORKGROUP (the rows of
each from row_tiles), never as a total.  The dropout mask comes from tests/drop_ref.py, not from another kernel.  Every output
has guard rows of sentinel behind it.  The gradient-penalty epilogue has no C entry point and is not reached from here.
"""
import ctypes as C
import functools

import pytest
import torch

import drop_ref
import exact_util as X
import test_exact_gemm_gpu as G

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CUDA = "cuda"
DROP_P, SEED, SITE = 0.5, 20240607, 3
T = 32  # rows of the fp32 residual table and of the broadcast h
GS, BS = X.RowBwdProbe.GS, X.RowBwdProbe.BS


@pytest.fixture(params=[384, 512])
def E(request):
    return request.param


@functools.lru_cache(maxsize=None)
def _keep_flat():
    """drop_ref.mask addresses an element by its flat index, so mask(p, seed, site, None, M * E) is a prefix of the mask of the
    largest probe (tests/test_exact_probes_cpu.py): drawn once, on the host, for every case of this module"""
    keep, scale = drop_ref.mask(DROP_P, SEED, SITE, None, max(X.ROW_M[512]) * 512)
    assert float(scale) == 2.0
    return torch.from_numpy(keep).to(CUDA)


def _keep(M, E):
    return _keep_flat()[:M * E].view(M, E)


def _variants(vs, fn):
    """fn(v) for every variant of one case; the first failing one names itself"""
    for v in vs:
        try:
            fn(v)
        except AssertionError as e:
            raise AssertionError(f"[{v}] {e}") from None


def _scalars():
    sc = torch.tensor([GS, BS], dtype=F32, device=CUDA)
    return sc, C.c_void_p(sc.data_ptr()), C.c_void_p(sc.data_ptr() + 4)


def _fwd_weights(E, K, sln):
    g = X.gen(E * 7 + K + 31 * sln, CUDA)
    W = X.counting((E, K), g, -1, 1, 0.5)
    return W, G._pack(E, W, K), X.counting((E,), g, -8, 8), 1.0 + X.dyadic((E,), g, 16, 4), X.dyadic((E,), g, 16, 8)


def _fwd_sum(A, W, bias, res, keep):
    """res + drop(A W^T + bias) in fp64, exact in bf16 (asserted); keep None: no dropout"""
    M, E = A.shape[0], W.shape[0]
    y = X.check_exact_gemm(A, W.t(), [bias.expand(M, E)], out_dtype=BF, what="A W^T + bias")
    if keep is not None:
        y = y * (2.0 * keep)
    y = y + res
    assert torch.equal(y, y.to(BF).double()), f"Y not exactly representable in bf16 (max |y| {float(y.abs().max())})"
    return y


# ------------------------------------------------------------------------------------------------------ forward epilogues
def test_linear_ln_fwd_every_height(E):
    """Y = res + drop(A W^T + bias) bitwise, with and without dropout; mean, rstd and Yn as test_linear_ln_fwd_counting holds them"""
    u = X.gpu()
    wts = {K: _fwd_weights(E, K, 0) for K in X.ROW_K}

    def one(c):
        M, K = c
        W, Wp, bias, gam, bet = wts[K]
        g = X.gen(100003 + M * 3 + K, CUDA)
        A, res = X.counting((M, K), g, -1, 1, 0.5), X.counting((M, E), g, -8, 8)
        dA, dr, db, dg, dbt = A.to(BF), res.to(BF), bias.float(), gam.float(), bet.float()

        def run(drop):
            y = _fwd_sum(A, W, bias, res, _keep(M, E) if drop else None)
            Y, Yn = X.guarded(M, E, BF, CUDA), X.guarded(M, E, BF, CUDA)
            mean, rstd = X.guarded(M, 1, F32, CUDA), X.guarded(M, 1, F32, CUDA)
            G.row_call(E, "vg_linear_ln_fwd", u.ptr(dA), u.ptr(Wp), u.ptr(db), u.ptr(dr), u.ptr(Y), u.ptr(Yn), u.ptr(mean), u.ptr(rstd),
                       u.ptr(dg), u.ptr(dbt), M, K, 1e-5, drop, SEED, SITE, None, u.stream())
            u.sync()
            G.check_row_fwd(y, Y, Yn, mean, rstd, M, G.plain_yn(gam, bet))
        _variants([DROP_P, 0.0], run)

    X.collect(X.row_cases(E), one)


@pytest.mark.parametrize("table", [False, True], ids=["res_bf16", "res_table"])
def test_linear_sln_fwd_every_height(E, table):
    """the self-modulated form: Y bitwise (residual a bf16 tensor, or an fp32 table of 32 rows broadcast over the batch), mean and
    rstd as above, Yn within one bf16 ulp of wmod (gs (LN(y) lw + lb) + bs) in fp64 from the exact Y"""
    u = X.gpu()
    wts = {K: _fwd_weights(E, K, 1) for K in X.ROW_K}
    sc, p_gs, p_bs = _scalars()
    tab = X.counting((T, E), X.gen(E + 5, CUDA), -8, 8)
    dtab = tab.float()

    def one(c):
        M, K = c
        W, Wp, bias, lw, lb = wts[K]
        g = X.gen(200003 + M * 3 + K + table, CUDA)
        A = X.counting((M, K), g, -1, 1, 0.5)
        res = tab.repeat(-(-M // T), 1)[:M] if table else X.counting((M, E), g, -8, 8)
        wmod = X.dyadic((M, E), g, 4, 8)
        dA, dr, db, dlw, dlb, dwm = A.to(BF), res.to(BF), bias.float(), lw.float(), lb.float(), wmod.to(BF)

        def yn_of(z):
            zl = z * lw
            return wmod * (GS * (zl + lb) + BS), G.YN_FLOOR * wmod.abs() * (abs(GS) * (zl.abs() + lb.abs()) + abs(BS))

        def run(drop):
            y = _fwd_sum(A, W, bias, res, _keep(M, E) if drop else None)
            Y, Yn = X.guarded(M, E, BF, CUDA), X.guarded(M, E, BF, CUDA)
            mean, rstd = X.guarded(M, 1, F32, CUDA), X.guarded(M, 1, F32, CUDA)
            G.row_call(E, "vg_linear_sln_fwd", u.ptr(dA), u.ptr(Wp), u.ptr(db), None if table else u.ptr(dr), u.ptr(dtab) if table else None, T,
                       u.ptr(Y), u.ptr(Yn), u.ptr(mean), u.ptr(rstd), u.ptr(dwm), u.ptr(dlw), u.ptr(dlb), p_gs, p_bs, M, K, 1e-5, drop,
                       SEED, SITE, None, u.stream())
            u.sync()
            G.check_row_fwd(y, Y, Yn, mean, rstd, M, yn_of)
        _variants([DROP_P, 0.0], run)

    X.collect(X.row_cases(E), one)


# ----------------------------------------------------------------------------------------------------- backward epilogues
def _check_bwd(p, E, rows, owner, with_gres, drop, dx, dxm, part, used):
    """what both backward epilogues share: dx (dh), dxm (dhm), the three column sums per workgroup, guards"""
    M, nwg = p.M, rows.numel()
    for t, n, w in ((dx, M, "dx"), (dxm, M, "dxm"), (part, nwg, "part")):
        if t is not None:
            X.assert_written(t[:, :used] if t is part else t, n, w)
            X.assert_guard(t, n, w)
    if used < part.shape[1]:  # the self-modulated form's partial rows are 64 wide behind 3 E and carry two values there
        assert bool((X.bits(part[:nwg, used:]) == X.F32_SENTINEL).all()), "part: written behind d gs | d bs"
    X.assert_bitwise(part[:nwg, 0:E], X.rne(X.per_workgroup(p.t["t_gamma"], owner, nwg), F32), "d gamma per workgroup")
    X.assert_bitwise(part[:nwg, E:2 * E], X.rne(X.per_workgroup(p.t["t_beta"], owner, nwg), F32), "d beta per workgroup")
    ref, floor = p.dx(with_gres)
    X.assert_ulps(dx[:M], ref, "dx", 1.0, floor=floor)
    stored = dx[:M]
    if drop:
        twice = (2.0 * dx[:M].float()).to(BF)  # one exact multiply of the kernel's own dx
        X.assert_bitwise(dxm[:M], torch.where(_keep(M, E), twice, torch.zeros_like(twice)), "dxm")
        stored = dxm[:M]
    X.assert_colsum(part[:nwg, 2 * E:3 * E], stored, owner, rows, "colsum per workgroup")


def test_linear_dgrad_ln_bwd_every_height(E):
    """d gamma and d beta per workgroup bitwise; dx within one bf16 ulp (+ 2^-20 of its fp32 terms) of fp64; dxm bitwise from the
    kernel's own dx and the host's mask; colsum per workgroup inside the fp32 summation bound of the stored rows: with and without
    dxm, with gres and with gres = NULL.  dx does not depend on whether the dropped copy is asked for."""
    u = X.gpu()
    L = u._lib.lib()

    def one(c):
        M, K = c
        p = X.RowBwdProbe(M, K, E, X.gen(300007 + M * 3 + K, CUDA))
        rows, owner = X.row_owner(M, E, CUDA)
        nwg = rows.numel()
        assert nwg == L.vg_row_parts(M)
        WpT = G._pack(E, p.W, K, transposed=True)
        ddY, dxin, dgres, dmu, drs, dgam = p.dY.to(BF), p.x.to(BF), p.gres.to(BF), p.mean.float(), p.rstd.float(), p.gamma.float()
        seen = {}

        def run(v):
            drop, with_gres = v
            dx, dxm = X.guarded(M, E, BF, CUDA), (X.guarded(M, E, BF, CUDA) if drop else None)
            part = X.guarded(nwg, 3 * E, F32, CUDA, guard=1)
            G.row_call(E, "vg_linear_dgrad_ln_bwd", u.ptr(ddY), u.ptr(WpT), u.ptr(dxin), u.ptr(dmu), u.ptr(drs), u.ptr(dgam),
                       u.ptr(dgres) if with_gres else None, u.ptr(dx), u.ptr(dxm), u.ptr(part), M, K, DROP_P if drop else 0.0, SEED, SITE,
                       None, u.stream())
            u.sync()
            _check_bwd(p, E, rows, owner, with_gres, drop, dx, dxm, part, 3 * E)
            if with_gres in seen:
                X.assert_bitwise(dx[:M], seen[with_gres], "dx with and without dxm")
            seen[with_gres] = dx[:M]
        _variants([(d, r) for d in (1, 0) for r in (1, 0)], run)

    X.collect(X.row_cases(E), one)


@pytest.mark.parametrize("bcast", [0, T], ids=["h_rows", "h_bcast"])
def test_linear_dgrad_sln_bwd_every_height(E, bcast):
    """the self-modulated form: dw_acc bitwise (dw_accumulate 0, and 1 on an integer-valued dw_acc), d lw / d lb and d gs / d bs per
    workgroup bitwise, dh / dhm / colsum as for the plain LayerNorm"""
    u = X.gpu()
    L = u._lib.lib()
    sc, p_gs, p_bs = _scalars()
    PW = 3 * E + 64

    def one(c):
        M, K = c
        p = X.RowBwdProbe(M, K, E, X.gen(400009 + M * 3 + K + bcast, CUDA), sln=True, bcast=bcast)
        rows, owner = X.row_owner(M, E, CUDA)
        nwg = rows.numel()
        assert nwg == L.vg_row_parts(M)
        p.check_scalar_budget(owner, nwg)
        WpT = G._pack(E, p.W, K, transposed=True)
        ddY, dh_in, dgres, dmu, drs = p.dY.to(BF), p.x.to(BF), p.gres.to(BF), p.mean.float(), p.rstd.float()
        dlw, dlb, dwm = p.gamma.float(), p.lb.float(), p.wmod.to(BF)
        dw0 = X.counting((M, E), X.gen(M + 9, CUDA), -1000, 1000)
        want_gs = X.rne(X.per_workgroup(p.t["t_gs"], owner, nwg).sum(1), F32)
        want_bs = X.rne(X.per_workgroup(p.t["t_bs"], owner, nwg).sum(1), F32)

        def run(v):
            drop, acc, with_gres = v
            dh, dhm = X.guarded(M, E, BF, CUDA), (X.guarded(M, E, BF, CUDA) if drop else None)
            dwa = X.guarded(M, E, F32, CUDA)
            if acc:
                dwa[:M] = dw0.float()
            part = X.guarded(nwg, PW, F32, CUDA, guard=1)
            G.row_call(E, "vg_linear_dgrad_sln_bwd", u.ptr(ddY), u.ptr(WpT), u.ptr(dh_in), bcast, u.ptr(dwm), u.ptr(dmu), u.ptr(drs), u.ptr(dlw),
                       u.ptr(dlb), p_gs, p_bs, u.ptr(dgres) if with_gres else None, u.ptr(dh), u.ptr(dhm), u.ptr(dwa), acc, u.ptr(part), M, K,
                       DROP_P if drop else 0.0, SEED, SITE, None, u.stream())
            u.sync()
            X.assert_written(dwa, M, "dw_acc")
            X.assert_guard(dwa, M, "dw_acc")
            X.assert_bitwise(dwa[:M], X.rne(X.assert_f32_exact(p.t["dw"] + dw0 if acc else p.t["dw"], "dw_acc"), F32), "dw_acc")
            X.assert_bitwise(part[:nwg, 3 * E], want_gs, "d gs per workgroup")
            X.assert_bitwise(part[:nwg, 3 * E + 1], want_bs, "d bs per workgroup")
            _check_bwd(p, E, rows, owner, with_gres, drop, dh, dhm, part, 3 * E + 2)
        _variants([(1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1)], run)

    X.collect(X.row_cases(E), one)


# ------------------------------------------------------------------------------------------------ tile-height independence
HEAD = 4096  # 256 units over 128 workgroups: tiles of 2 m-tiles
TALLER = {384: [12288, 24576, 28672], 512: [12288, 24576]}  # the same rows as the head of tiles of 3, 6 (and 7) m-tiles


@pytest.mark.parametrize("sln", [False, True], ids=["ln", "sln"])
def test_rows_do_not_depend_on_the_tile_height(E, sln):
    """test_row_gpu.py::test_rows_do_not_depend_on_the_tile_they_land_in at the heights it never saw (it runs 2, 4-5 and 8-9): the first
    4096 rows as a problem of their own and as the head of taller problems give bit-identical Y, Yn, mean, rstd, dx and dxm
    (and d w), through the plain and the self-modulated epilogues.  Random bf16 inputs."""
    u = X.gpu()
    L = u._lib.lib()
    K, Mbig = 192, max(TALLER[E])
    for M in [HEAD] + TALLER[E]:
        assert {h for _, t in X.row_tiles(M, E) for h in t} == {2 if M == HEAD else M // 4096}, M
    g = X.gen(11 + E, CUDA)
    rnd = lambda *s: torch.randn(*s, generator=g, device=CUDA)  # noqa: E731
    A = rnd(Mbig, K).to(BF)
    Wp = G._pack(E, rnd(E, K) / K ** 0.5, K)
    WpT = G._pack(E, rnd(K, E) / K ** 0.5, K, transposed=True)
    R, Xin, wmod = rnd(Mbig, E).to(BF), (rnd(Mbig, E) * 1.5 + 0.3).to(BF), rnd(Mbig, E).to(BF)
    gam, bet, b = 1.0 + 0.2 * rnd(E), 0.1 * rnd(E), 0.1 * rnd(E)
    mu = Xin.float().mean(1).contiguous()
    rs = (1.0 / torch.sqrt(Xin.float().var(1, unbiased=False) + 1e-5)).contiguous()
    sc, p_gs, p_bs = _scalars()
    outs = []
    for M in [HEAD] + TALLER[E]:
        Y, Yn, dx, dxm = (torch.empty(M, E, dtype=BF, device=CUDA) for _ in range(4))
        mean, rstd = torch.empty(M, device=CUDA), torch.empty(M, device=CUDA)
        dwa = torch.empty(M, E, device=CUDA)
        part = torch.empty(L.vg_row_parts(M), 3 * E + 64, device=CUDA)
        if sln:
            G.row_call(E, "vg_linear_sln_fwd", u.ptr(A), u.ptr(Wp), u.ptr(b), u.ptr(R), None, 0, u.ptr(Y), u.ptr(Yn), u.ptr(mean), u.ptr(rstd),
                       u.ptr(wmod), u.ptr(gam), u.ptr(bet), p_gs, p_bs, M, K, 1e-5, 0.1, 3, 1, None, u.stream())
            G.row_call(E, "vg_linear_dgrad_sln_bwd", u.ptr(A), u.ptr(WpT), u.ptr(Xin), 0, u.ptr(wmod), u.ptr(mu), u.ptr(rs), u.ptr(gam), u.ptr(bet),
                       p_gs, p_bs, u.ptr(R), u.ptr(dx), u.ptr(dxm), u.ptr(dwa), 0, u.ptr(part), M, K, 0.1, 3, 1, None, u.stream())
        else:
            G.row_call(E, "vg_linear_ln_fwd", u.ptr(A), u.ptr(Wp), u.ptr(b), u.ptr(R), u.ptr(Y), u.ptr(Yn), u.ptr(mean), u.ptr(rstd), u.ptr(gam),
                       u.ptr(bet), M, K, 1e-5, 0.1, 3, 1, None, u.stream())
            G.row_call(E, "vg_linear_dgrad_ln_bwd", u.ptr(A), u.ptr(WpT), u.ptr(Xin), u.ptr(mu), u.ptr(rs), u.ptr(gam), u.ptr(R), u.ptr(dx),
                       u.ptr(dxm), u.ptr(part), M, K, 0.1, 3, 1, None, u.stream())
        u.sync()
        outs.append([t[:HEAD].clone() for t in (Y, Yn, mean, rstd, dx, dxm) + ((dwa,) if sln else ())])
    assert bool(torch.isfinite(outs[0][0].float()).all()) and float(outs[0][4].float().abs().max()) > 0
    for M, other in zip(TALLER[E], outs[1:]):
        for name, a_, b_ in zip(("Y", "Yn", "mean", "rstd", "dx", "dxm", "dw_acc"), outs[0], other):
            assert torch.equal(a_, b_), f"{name} of the first {HEAD} rows differs between M = {HEAD} and M = {M}"
