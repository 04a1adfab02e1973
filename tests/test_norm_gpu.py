"""The bf16 first-order normalisation kernels of csrc/norm.hip through the C ABI against the float64 restatements of tests/norm_ref.py.

vg_layernorm_fwd / _bwd at every width of NV_SWITCH, at row counts on both sides of one workgroup pass (8 rows), of one partial row
(16) and of the grid cap (512 partial rows: 8192), and at the engine's own 16 640 rows; vg_sln_fwd / _bwd with h broadcast and not, dw
overwritten and accumulated; vg_colsum_f32 and vg_colsum_bf16 on integers, where every order of summation is exact, bit for bit.
Every output lives in a buffer with sentinel rows behind it and must be written in full and nowhere else.  The bounds are derived in
norm_ref (kappa_*, rstd_rel_bound) and checked there against a float32 emulation (tests/test_norm_ref_cpu.py); nothing here is tuned
to what the GPU returns.  Each test prints the worst err / limit per output as a record."""
import ctypes as C

import pytest
import torch

import exact_util as X
import norm_ref as N
from exact_util import BF

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ROWS_SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 130]
ROWS_LARGE = [8191, 8192, 8193, 16640]
EPS = 1e-5


def _u():
    return X.gpu()


def _lib():
    from vit_gan_amd import _lib
    return _lib.lib()


def _off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


def _vec(n, guard=1):
    """n fp32 of sentinel as row 0 of a guarded buffer"""
    return X.guarded(1, n, F32, "cuda", guard=guard)


def _whole(buf, rows, what):
    X.assert_guard(buf, rows, what)
    X.assert_written(buf, rows, what)


def _show(what, stats):
    print(what, {k: round(v, 3) for k, v in stats.items()}, "(worst err / limit)")


# --------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_fwd_run(x, gamma, beta, R, E, strided=False):
    """contiguous, or x as the middle third of [R, 3E] (xs = 3E) and y as the first half of a guarded [R, 2E] (ys = 2E)"""
    g = _u()
    mean, rstd = _vec(R), _vec(R)
    if strided:
        xb = torch.full((R, 3 * E), 777.0, dtype=BF, device="cuda")
        xb[:, E:2 * E] = x
        y = X.guarded(R, 2 * E, BF, "cuda")
        g.call("vg_layernorm_fwd", _off(xb, 2 * E), 3 * E, g.ptr(gamma), g.ptr(beta), g.ptr(y), 2 * E, g.ptr(mean), g.ptr(rstd), R, E, EPS, g.stream())
        g.sync()
        X.assert_guard(y[:, E:], 0, f"E {E} R {R}: the half of the strided y that is not the kernel's")
        yv = y[:, :E]
    else:
        yv = y = X.guarded(R, E, BF, "cuda")
        g.call("vg_layernorm_fwd", g.ptr(x), E, g.ptr(gamma), g.ptr(beta), g.ptr(y), E, g.ptr(mean), g.ptr(rstd), R, E, EPS, g.stream())
        g.sync()
    for buf, rows, n in ((yv, R, "y"), (mean, 1, "mean"), (rstd, 1, "rstd")):
        _whole(buf, rows, f"E {E} R {R} fwd {n}{' (strided)' if strided else ''}")
    return {"y": yv[:R].contiguous(), "mean": mean[0], "rstd": rstd[0]}


def _ln_bwd_run(dy, x, mean, rstd, gamma, gres, R, E):
    """vg_layernorm_bwd then the fold of its three segments; every partial row must be written"""
    g = _u()
    parts = _lib().vg_layernorm_bwd_parts(R)
    assert parts == N.bwd_parts(R)
    dx = X.guarded(R, E, BF, "cuda")
    part = X.guarded(parts, 3 * E, F32, "cuda", guard=16)
    g.call("vg_layernorm_bwd", g.ptr(dy), g.ptr(x), g.ptr(mean), g.ptr(rstd), g.ptr(gamma), g.ptr(gres), g.ptr(dx), g.ptr(part), R, E, g.stream())
    dg, db, cs = _vec(E), _vec(E), _vec(E)
    g.call("vg_colsum_f32", g.ptr(part), parts, 3 * E, g.ptr(dg), E, g.ptr(db), E, g.ptr(cs), E, None, 0, 0, g.stream())
    g.sync()
    for buf, rows, n in ((dx, R, "dx"), (part, parts, "part"), (dg, 1, "dgamma"), (db, 1, "dbeta"), (cs, 1, "colsum(dx)")):
        _whole(buf, rows, f"E {E} R {R} bwd {n}{'' if gres is None else ' (gres)'}")
    return {"dx": dx[:R], "dgamma": dg[0], "dbeta": db[0], "dxsum": cs[0], "part": part[:parts]}


def _trip_groups(R):
    """rows of three different trips of the backward's grid-stride loop (a pass of the 512 workgroups covers 4096 rows)"""
    return [("rows 0-7", slice(0, 8)), ("rows 4096-4103", slice(4096, 4104)), ("last 9 rows", slice(R - 9, R))]


def _ln_case(E, R, stats, strided=False):
    g = _u()
    what = f"E {E} R {R}"
    inp = N.norm_inputs(R, E, 1)
    refs = N.ln_refs(inp, EPS)
    x, dy, gres = (g.dev(inp[n], BF) for n in ("x", "dy", "gres"))
    gamma, beta = g.dev(inp["gamma"], F32), g.dev(inp["beta"], F32)
    mean, rstd = g.dev(refs["mean"]), g.dev(refs["rstd"])   # the fp32 roundings of the float64 statistics, not the forward's output
    got = {"f": _ln_fwd_run(x, gamma, beta, R, E), "bg": _ln_bwd_run(dy, x, mean, rstd, gamma, gres, R, E),
           "b0": _ln_bwd_run(dy, x, mean, rstd, gamma, None, R, E)}
    failed = N.run_assertions(N.ln_assertions(got, refs, inp, R, E, EPS, what), stats)
    if R in (8193, 16640):
        for name, rows in _trip_groups(R):
            for key in ("bg", "b0"):
                failed += N.run_assertions([(f"{name} {n}", f) for n, f in N.bwd_assertions(got[key], refs[key], R, E, rows=rows, what=f"{what} {name}")], stats)
    assert not failed, "\n".join(failed)
    # a second launch is the first, bit for bit, down to the partial rows
    again = _ln_bwd_run(dy, x, mean, rstd, gamma, gres, R, E)
    for n in ("dx", "part", "dgamma", "dbeta", "dxsum"):
        X.assert_bitwise(again[n].contiguous(), got["bg"][n].contiguous(), f"{what} {n}: second launch")
    if strided:
        fs = _ln_fwd_run(x, gamma, beta, R, E, strided=True)
        for n in ("y", "mean", "rstd"):
            X.assert_bitwise(fs[n].contiguous(), got["f"][n].contiguous(), f"{what} {n}: strided against contiguous")


@pytest.mark.parametrize("E", N.WIDTHS)
def test_layernorm_small_row_counts(E):
    """R on both sides of one workgroup pass of the backward (8 rows: the second trip starts at R = 9 with one workgroup), of one
    partial row (16) and of the forward's 16 rows a workgroup; at E = 384 and 768 also with strides"""
    stats = {}
    X.collect(ROWS_SMALL, lambda R: _ln_case(E, R, stats, strided=E in (384, 768)), f"E {E} R ")
    _show(f"LayerNorm E {E}:", stats)


@pytest.mark.parametrize("R", ROWS_LARGE)
@pytest.mark.parametrize("E", [128, 384, 768, 1024])
def test_layernorm_at_the_grid_cap(E, R):
    """R around 8192 (the cap of 512 partial rows; at 8193 the row stride is 8 * 512 and a third trip starts) and the engine's 16 640;
    at 8193 and 16 640 rows of three different trips are also held on their own, so that a miss confined to one trip is named"""
    stats = {}
    _ln_case(E, R, stats, strided=E in (384, 768) and R == 8193)
    _show(f"LayerNorm E {E} R {R}:", stats)


# --------------------------------------------------------------------------------------------------------------------- SLN
def _sln_fwd_run(h, T, w, lw, lb, sc, R, E):
    g = _u()
    y, mean, rstd = X.guarded(R, E, BF, "cuda"), _vec(R), _vec(R)
    g.call("vg_sln_fwd", g.ptr(h), T, g.ptr(w), g.ptr(lw), g.ptr(lb), g.ptr(sc), _off(sc, 4), g.ptr(y), g.ptr(mean), g.ptr(rstd), R, E, EPS, g.stream())
    g.sync()
    for buf, rows, n in ((y, R, "y"), (mean, 1, "mean"), (rstd, 1, "rstd")):
        _whole(buf, rows, f"E {E} R {R} T {T} sln fwd {n}")
    return {"y": y[:R], "mean": mean[0], "rstd": rstd[0]}


def _sln_bwd_run(dy, h, T, w, mean, rstd, lw, lb, sc, gres, R, E, dw_start=None):
    """vg_sln_bwd and the fold of its four segments (n3 = 2: d gs, d bs).  dw_start: dw_accumulate = 1 from that fp32 tensor, else 0
    from the sentinel."""
    g = _u()
    parts, PW = _lib().vg_layernorm_bwd_parts(R), 3 * E + 64
    assert parts == N.bwd_parts(R)
    dh, dw = X.guarded(R, E, BF, "cuda"), X.guarded(R, E, F32, "cuda")
    if dw_start is not None:
        dw[:R] = g.dev(dw_start, F32)
    part = X.guarded(parts, PW, F32, "cuda", guard=16)
    g.call("vg_sln_bwd", g.ptr(dy), g.ptr(h), T, g.ptr(w), g.ptr(mean), g.ptr(rstd), g.ptr(lw), g.ptr(lb), g.ptr(sc), _off(sc, 4), g.ptr(gres),
           g.ptr(dh), g.ptr(dw), 0 if dw_start is None else 1, g.ptr(part), R, E, g.stream())
    dlw, dlb, cs, dsc = _vec(E), _vec(E), _vec(E), _vec(64)
    g.call("vg_colsum_f32", g.ptr(part), parts, PW, g.ptr(dlw), E, g.ptr(dlb), E, g.ptr(cs), E, g.ptr(dsc), 2, 0, g.stream())
    g.sync()
    what = f"E {E} R {R} T {T} sln bwd"
    for buf, rows, n in ((dh, R, "dh"), (dw, R, "dw"), (part[:, :3 * E + 2], parts, "part"), (dlw, 1, "dlw"), (dlb, 1, "dlb"), (cs, 1, "colsum(dh)"),
                         (dsc[:, :2], 1, "d gs, d bs")):
        _whole(buf, rows, f"{what} {n}")
    X.assert_guard(part[:, 3 * E + 2:], parts, f"{what}: guard rows behind the unspecified columns of part")
    X.assert_guard(dsc[:, 2:], 0, f"{what}: the fold of n3 = 2 wrote past 2 elements")
    out = {"dh": dh[:R], "dw": dw[:R], "dlw": dlw[0], "dlb": dlb[0], "dxsum": cs[0], "dgs": dsc[0, 0], "dbs": dsc[0, 1], "part": part[:parts, :3 * E + 2]}
    if dw_start is not None:
        out["dw_start"] = dw_start
    return out


def _sln_case(E, R, T, stats):
    g = _u()
    what = f"E {E} R {R} T {T}"
    inp = N.norm_inputs(R, E, 2, T)
    refs = N.sln_refs(inp, T, EPS)
    h, w, dy, gres = (g.dev(inp[n], BF) for n in ("h", "w", "dy", "gres"))
    lw, lb = g.dev(inp["lw"], F32), g.dev(inp["lb"], F32)
    sc = g.dev(torch.tensor([inp["gs"], inp["bs"]], dtype=F64), F32)
    mean, rstd = g.dev(refs["mean"]), g.dev(refs["rstd"])
    start = torch.randn(R, E, generator=X.gen(R + E), dtype=F32).double()
    a = (dy, h, T, w, mean, rstd, lw, lb, sc)
    got = {"f": _sln_fwd_run(h, T, w, lw, lb, sc, R, E), "bg": _sln_bwd_run(*a, gres, R, E, dw_start=start), "b0": _sln_bwd_run(*a, None, R, E)}
    failed = N.run_assertions(N.sln_assertions(got, refs, inp, R, E, what), stats)
    if R == 8193:
        for name, rows in _trip_groups(R):
            for key in ("bg", "b0"):
                failed += N.run_assertions([(f"{name} {n}", f) for n, f in N.bwd_assertions(got[key], refs[key], R, E, sln=True, rows=rows,
                                                                                            what=f"{what} {name}")], stats)
    assert not failed, "\n".join(failed)
    again = _sln_bwd_run(*a, gres, R, E, dw_start=start)
    for n in ("dh", "dw", "part", "dlw", "dlb", "dxsum", "dgs", "dbs"):
        X.assert_bitwise(torch.atleast_1d(again[n]).contiguous(), torch.atleast_1d(got["bg"][n]).contiguous(), f"{what} {n}: second launch")


# (R, T): h broadcast over B = 3 images at T = 1, 17, 32; R = 40 is no multiple of T = 17; T = 0: h has R rows
SLN_SMALL = [(3, 1), (51, 17), (96, 32), (40, 17), (34, 0), (96, 0)]


@pytest.mark.parametrize("E", [128, 384, 512, 1024])
def test_sln_small_row_counts(E):
    stats = {}
    X.collect(SLN_SMALL, lambda c: _sln_case(E, c[0], c[1], stats), f"E {E} (R, T) ")
    _show(f"SLN E {E}:", stats)


@pytest.mark.parametrize("E", [128, 384, 512, 1024])
def test_sln_past_the_grid_cap(E):
    stats = {}
    _sln_case(E, 8193, 0, stats)
    _show(f"SLN E {E} R 8193:", stats)


# ----------------------------------------------------------------------------------------------------------- vg_colsum_f32
def _segment_sets(width):
    q = width // 4
    four = [q, q, q, width - 3 * q]
    return {"one": ([width, 0, 0, 0], ()), "four": (four, ()), "null second": (four, (1,)), "short": ([width // 2, width // 4, 0, 0], ())}


@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_f32_on_integers(accumulate):
    """integer partials with |v| <= 64 and rows * 64 < 2^24: every order of summation is exact, so the fold must give the float64 sum
    bit for bit.  A NULL segment's columns are skipped without shifting the later ones; columns past the last segment are ignored."""
    g = _u()

    def one(case):
        rows, width = case
        gen = X.gen(rows * 4099 + width)
        part64 = X.counting((rows, width), gen, -64, 64)
        assert rows * 64 < X.EXACT_LIMIT
        part = g.dev(part64, F32)
        want = part64.sum(0)
        for name, (sizes, null) in _segment_sets(width).items():
            start64 = [X.counting((max(n, 1),), gen, -64, 64) for n in sizes]
            dst = [_vec(max(n, 1)) for n in sizes]
            if accumulate:
                for d, s in zip(dst, start64):
                    d[0] = g.dev(s, F32)
            args = []
            for k, (d, n) in enumerate(zip(dst, sizes)):
                args += [None if k in null else g.ptr(d), n]
            g.call("vg_colsum_f32", g.ptr(part), rows, width, *args, accumulate, g.stream())
            g.sync()
            off = 0
            for k, (d, n, s) in enumerate(zip(dst, sizes, start64)):
                what = f"segments '{name}' segment {k} (n {n})"
                X.assert_guard(d, 1, what)
                if k in null or n == 0:   # must stay as it was: the sentinel, or the integers it started from
                    if accumulate:
                        X.assert_bitwise(d[0].cpu(), X.rne(s, F32), what + ": a segment that must stay untouched")
                    else:
                        X.assert_guard(d, 0, what + ": a segment that must stay untouched")
                else:
                    X.assert_written(d, 1, what)
                    X.assert_bitwise(d[0].cpu(), X.rne(want[off:off + n] + (s if accumulate else 0.0), F32), what)
                off += n
    X.collect([(rows, width) for rows in (1, 15, 16, 17, 512, 513) for width in (1, 16, 17, 1216, 3072)], one, "(rows, width) ")


# ---------------------------------------------------------------------------------------------------------- vg_colsum_bf16
def _colsum_bf16_run(x, R, N_, ld3, accumulate, start=None):
    """x [R, N] bf16 on the device; ld3: X is the middle third of a [R, 3N] buffer whose outer thirds hold 1000"""
    g = _u()
    parts = _lib().vg_colsum_bf16_parts(R)
    assert parts == N.colsum_bf16_parts(R)
    ws, dst = X.guarded(parts, N_, F32, "cuda", guard=4), _vec(N_)
    if accumulate:
        dst[0] = start
    if ld3:
        xb = torch.full((R, 3 * N_), 1000.0, dtype=BF, device="cuda")
        xb[:, N_:2 * N_] = x
        g.call("vg_colsum_bf16", _off(xb, 2 * N_), 3 * N_, R, N_, g.ptr(ws), g.ptr(dst), accumulate, g.stream())
    else:
        g.call("vg_colsum_bf16", g.ptr(x), N_, R, N_, g.ptr(ws), g.ptr(dst), accumulate, g.stream())
    g.sync()
    what = f"R {R} N {N_} ld {'3N' if ld3 else 'N'} accumulate {accumulate}"
    _whole(ws, parts, what + " part_ws")
    X.assert_guard(dst, 1, what + " dst")
    if not accumulate:
        X.assert_written(dst, 1, what + " dst")
    return dst[0], what


@pytest.mark.parametrize("N_", [8, 248, 256, 264, 1152])
def test_colsum_bf16_on_integers(N_):
    """integers in [-4, 4]: exact in any order (R * 4 < 2^24), so the result is the float64 sum bit for bit.  R on both sides of 8 (the
    row lanes of a workgroup) and of 256 (its rows); N on both sides of 256 (its columns); ld = N and ld = 3N."""
    def one(case):
        R, ld3, accumulate = case
        gen = X.gen(R * 31 + N_, "cuda")
        x64 = X.counting((R, N_), gen, -4, 4)
        start64 = X.counting((N_,), gen, -64, 64)
        got, what = _colsum_bf16_run(x64.to(BF), R, N_, ld3, accumulate, start64.float())
        want = x64.sum(0) + (start64 if accumulate else 0.0)
        X.assert_bitwise(got, X.rne(want, F32), what)
    X.collect([(R, ld3, acc) for R in (1, 7, 8, 9, 255, 256, 257, 16641) for ld3 in (False, True) for acc in (0, 1)], one, f"N {N_} (R, ld 3N, accumulate) ")


@pytest.mark.parametrize("R,N_", [(16640, 1152), (2080, 384)])
def test_colsum_bf16_random(R, N_):
    """N(0, 1) inputs at the engine's shapes: within kappa_colsum_bf16 * 2^-24 * sum_r |x| of the float64 sum"""
    x64 = torch.randn(R, N_, generator=X.gen(R + N_), dtype=F64).to(BF).double()
    got, what = _colsum_bf16_run(_u().dev(x64, BF), R, N_, False, 0)
    worst = N.assert_elementwise(got, x64.sum(0), x64.abs().sum(0), N.kappa_colsum_bf16(R), what, rel=0.0)
    print(f"vg_colsum_bf16 {what}: worst err / limit {worst:.3f}")
