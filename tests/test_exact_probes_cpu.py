"""The exact probes of test_exact_gemm_gpu.py / test_exact_attention_gpu.py / test_exact_row_gpu.py, checked without a GPU: every
probe family meets its preconditions at the shapes the GPU tests use, the constructed expectations equal the fp64 torch result
of the same operation, the shape tables reach every kernel of the dispatch (and, for the full-row kernel, every tile height it is
instantiated for), and each checker rejects simulated kernel defects."""
import math

import pytest
import torch

import exact_util as X

BF, F32 = torch.bfloat16, torch.float32
S_SAMPLE = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 48, 79, 80, 81, 96, 97, 128, 129, 161, 193, 197, 225, 255, 256]
KINDS = [("perm", None), ("tie2", "first_last"), ("tie2", "pair"), ("tie2", "tiles"), ("tie4", None), ("sum", None)]


def _probe(S, HE, kind, where, seed=0):
    if kind == "tie2" and S >= 2:
        a = 32 * ((S - 1) // 32)
        ties = {"first_last": (0, S - 1), "pair": (a, a + 1) if a + 1 < S else (a - 1, a),
                "tiles": (max(S - 17, 0), S - 1)}[where]
        if ties[0] == ties[1]:
            return None
        return X.AttnProbe(2, 2, S, HE, "tie2", ties, seed)
    if kind == "tie4":
        if S < 4:
            return None
        return X.AttnProbe(2, 2, S, HE, "tie4", (0, S // 3, (2 * S) // 3, S - 1), seed)
    if kind == "tie2":
        return None
    return X.AttnProbe(2, 2, S, HE, kind, None, seed)


def _torch_attention(p, scale, drop=None, mask_last=False):
    """fp64 torch: O = softmax(scale Q K^T) V and, by autograd, dQ / dK / dV for p.dO; `drop` = (q, k) pairs removed from the
    softmax, mask_last = key S - 1 masked out (simulated kernel defects)"""
    Q = p.Q.clone().requires_grad_(True)
    K = p.K.clone().requires_grad_(True)
    V = p.V.clone().requires_grad_(True)
    s = (Q @ K.transpose(-1, -2)) * scale
    if drop is not None:
        s = s.clone()
        for q, k in drop:
            s[:, :, q, k] = -math.inf
    if mask_last:
        s = s.clone()
        s[..., -1] = -math.inf
    P = torch.softmax(s, -1)
    O = P @ V
    O.backward(p.dO)
    return P.detach(), O.detach(), Q.grad, K.grad, V.grad, torch.logsumexp(s.detach(), -1)


@pytest.mark.parametrize("HE", [32, 64, 96])
@pytest.mark.parametrize("kind,where", KINDS)
def test_attention_probes_are_exact(HE, kind, where):
    for S in S_SAMPLE:
        p = _probe(S, HE, kind, where)
        if p is None:
            continue
        scales = [1 / 8, 1 / 16, 1 / math.sqrt(HE), 1 / math.sqrt(128)]
        p.check_preconditions(scales)
        for scale in (1 / 8, 1 / 16):
            P, O, dQ, dK, dV, lse = _torch_attention(p, scale)
            assert float((P - p.P()).abs().max()) < 1e-40, (S, "softmax is not saturated")
            assert float((O - p.forward()).abs().max()) < 1e-30
            eQ, eK, eV, dS = p.backward(scale)
            for a, b in ((dQ, eQ), (dK, eK), (dV, eV)):
                assert float((a - b).abs().max()) < 1e-25
            m, logt = p.lse_exact(scale)
            assert float((lse - (m + logt)).abs().max()) < 1e-9
            # every expected value is exact in fp32 (the kernels' accumulators), so the bf16 outputs are ONE rounding of it
            for t in (p.forward(), eQ, eK, eV):
                assert torch.equal(X.rne(t, F32).double(), t)
            assert torch.equal(X.rne(p.forward(), BF).double(), p.forward())  # O itself is exact in bf16
        if kind == "perm":
            assert bool((p.forward() == p.V.gather(2, p.P().argmax(-1, keepdim=True).expand(-1, -1, -1, HE))).all())
            assert float(p.backward(1 / 8)[0].abs().max()) == 0.0 and float(p.backward(1 / 8)[1].abs().max()) == 0.0
        if kind in ("tie2", "tie4"):  # the CLS row sits on the tie
            assert bool((p.ties_per_query()[:, :, 0] == (2 if kind == "tie2" else 4)).all())
        if kind == "sum" and S >= 8:
            assert float(p.backward(1 / 16)[0].abs().max()) > 0, "sum probe has no nonzero dQ"


def test_preconditions_reject_an_unintended_tie():
    """a key code duplicated where no tie was designed is caught before any launch"""
    p = X.AttnProbe(2, 2, 40, 32, "perm", None, 4)
    p.check_preconditions([1 / 8])
    p.K[1, 0, 7] = p.K[1, 0, 20]  # keys 7 and 20 now share a code: the queries on it see an undesigned 2-way tie
    q7 = int(p.designed[1, 0, :, 7].nonzero()[0])
    p.Q[1, 0, q7] = p.K[1, 0, 20]
    with pytest.raises(AssertionError, match="against the design"):
        p.check_preconditions([1 / 8])
    t = X.AttnProbe(2, 2, 40, 32, "tie2", (3, 30), 4)
    t.check_preconditions([1 / 8])
    t.designed[0, 1, 0, 30] = False  # the tie is real but no longer the designed one
    with pytest.raises(AssertionError, match="against the design"):
        t.check_preconditions([1 / 8])


def test_attention_probe_codes_fit():
    """enough 2-subsets of the head dims for 256 distinct keys, and c = 64 keeps the gap >= 110 at every scale in use
    (c = 32 would not at 1/16, 1/sqrt(96) or 1/sqrt(128))"""
    assert 32 * 31 // 2 >= 256
    for scale in (1 / 8, 1 / 16, 1 / math.sqrt(32), 1 / math.sqrt(64), 1 / math.sqrt(96), 1 / math.sqrt(128)):
        assert X.CODE ** 2 * scale >= X.MIN_GAP
    assert min(32.0 ** 2 * s for s in (1 / 16, 1 / math.sqrt(96), 1 / math.sqrt(128))) < X.MIN_GAP
    assert torch.exp(torch.tensor(-X.MIN_GAP, dtype=F32)) == 0.0


def test_attention_checkers_reject_defects():
    S, HE, scale = 97, 32, 1 / 8
    p = X.AttnProbe(2, 2, S, HE, "perm", None, 5)
    want = X.rne(p.flat(p.forward()), BF)
    X.assert_bitwise(want.clone(), want, "identity")
    # one dropped (query, key) pair: the target of query 10
    k = int(p.P()[0, 0, 10].argmax())
    O = _torch_attention(p, scale, drop=[(10, k)])[1]
    with pytest.raises(AssertionError):
        X.assert_bitwise(X.rne(p.flat(O).float().double(), BF), want, "drop")
    # a key mask off by one at S - 1
    O = _torch_attention(p, scale, mask_last=True)[1]
    with pytest.raises(AssertionError):
        X.assert_bitwise(X.rne(p.flat(O).float().double(), BF), want, "mask")
    # a tie with one of its keys dropped: O = V_a instead of (V_a + V_b) / 2
    t = X.AttnProbe(2, 2, S, HE, "tie2", (0, S - 1), 5)
    wt = X.rne(t.flat(t.forward()), BF)
    qs = (t.P()[0, 0, :, S - 1] > 0).nonzero()[:, 0].tolist()
    O = _torch_attention(t, scale, drop=[(q, S - 1) for q in qs])[1]
    with pytest.raises(AssertionError):
        X.assert_bitwise(X.rne(t.flat(O).float().double(), BF), wt, "tie drop")


def _bad_lse_raises(p, scale, lse):
    import test_exact_attention_gpu as A
    with pytest.raises(AssertionError):
        A._check_lse(lse, p, scale, "lse")


def test_lse_checker():
    import test_exact_attention_gpu as A
    p = X.AttnProbe(2, 2, 40, 32, "tie2", (0, 39), 1)
    m, logt = p.lse_exact(1 / 8)
    good = (m + logt).float()
    A._check_lse(good, p, 1 / 8, "lse")
    bump = good.clone()
    bump[0, 0, 5] = torch.nextafter(torch.nextafter(bump[0, 0, 5], torch.tensor(1e9)), torch.tensor(1e9))
    _bad_lse_raises(p, 1 / 8, bump)


# ------------------------------------------------------------------------------------------------------------- GEMMs
def test_shape_tables_reach_every_kernel():
    fwd = {X.fwd_target(M, N, K) for Ms, N, K in X.FWD_SHAPES for M in Ms}
    fwd |= {X.fwd_target(M, N, K, 0, "f32", True) for Ms, N, K in X.FWD_SHAPES for M in Ms}
    import test_exact_gemm_gpu as G
    for act, want in ((1, {"tiled128", "tiled256", "wr"}), (3, {"tiled128", "wr"})):  # tanh is never on 256-row tiles
        assert {X.fwd_target(M, N, K, a, pre) for Ms, N, K, a, pre in G.ACT_SHAPES if a == act for M in Ms} == want
    assert {X.fwd_target(M, N, K, 1, "bf16") for Ms, N, K in G.GELU_SHAPES for M in Ms} == {"tiled128", "tiled256", "wr"}
    assert {X.fwd_target(M, N, K, 0, p, True) for Ms, N, K in G.WIDE_SHAPES for M in Ms for p in ("f32", "bf16")} >= {
        "tiled128", "tiled256"}
    assert "wr" in {X.fwd_target(M, N, K) for Ms, N, K in G.WIDE_SHAPES for M in Ms}
    # the residual epilogue of wr (bias + residual, no pre-activation output) in both counting tests
    assert (1, None) in G.FWD_VARIANTS
    assert "wr" in {X.fwd_target(M, N, K, 0, None, True) for Ms, N, K in X.FWD_SHAPES for M in Ms}
    assert "wr" in {X.fwd_target(M, N, K, 0, None, True) for Ms, N, K in G.WIDE_SHAPES for M in Ms}
    assert fwd == {"tiled128", "tiled256", "wr"}
    assert {X.dgrad_target(M, N, K) for Ms, N, K in X.DGRAD_SHAPES for M in Ms} == {"tiled128", "tiled256", "wr"}
    assert {X.wgrad_target(*s) for s in G.WGRAD_SPLIT_SHAPES} == {"tiled_tn", "tn384", "tn512"}
    runs = set()
    for Ms, N, K in X.FWD_SHAPES:
        for M in Ms:
            if X.fwd_target(M, N, K) == "wr":
                runs |= X.wr_runs(M, N)
    assert {r for _, r in runs} == {0, 1, 2, 3}, runs
    assert {0, 1} <= {nf for nf, _ in runs} and max(nf for nf, _ in runs) >= 2, runs
    # every M residue class around the 16 / 32 / 128 / 256 boundaries
    for b in (16, 32, 128, 256):
        assert {b - 1, b, b + 1} <= set(X.M_RESIDUES)
    assert any(N % 128 for _, N, _ in X.FWD_SHAPES) and {48, 96, 384, 768, 1536} <= {K for _, _, K in X.FWD_SHAPES}
    assert {K % 32 for _, _, K in X.FWD_SHAPES} == {0, 8, 16, 24}  # every K tail of a 32-deep k-step


@pytest.mark.parametrize("K", [48, 96, 384, 768, 1536])
def test_counting_regime_preconditions(K):
    """the generators of test_exact_gemm_gpu.py: |y| <= 256 (bf16-exact), every partial sum < 2^24"""
    g = X.gen(K)
    dens = 1.0 if K <= 96 else 0.5
    A, W = X.counting((1040, K), g, -1, 1, dens), X.counting((256, K), g, -1, 1, dens)
    bias, res = X.counting((256,), g, -8, 8), X.counting((1040, 256), g, -8, 8)
    y = X.check_exact_gemm(A, W.t(), [bias.expand(1040, 256), res])
    assert float(y.abs().max()) <= 256
    # the wgrad regime at the step's M
    g = X.gen(K + 1)
    dY, Xa = X.counting((33280, 8), g, -1, 1, 0.25), X.counting((33280, K), g, -1, 1, 0.25)
    X.check_exact_gemm(dY.t(), Xa, out_dtype=F32)


def test_gemm_checker_rejects_defects():
    g = X.gen(11)
    M, N, K = 64, 136, 96
    A, W = X.counting((M, K), g), X.counting((N, K), g)
    y = X.check_exact_gemm(A, W.t())
    want = X.rne(y, BF)
    # one dropped product
    m, n = 17, 100
    k = int((A[m] * W[n]).ne(0).nonzero()[0])
    bad = y.clone()
    bad[m, n] -= A[m, k] * W[n, k]
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_bitwise(X.rne(bad, BF), want, "drop")
    # two swapped rows
    assert not torch.equal(y[3], y[40])
    bad = y.clone()
    bad[[3, 40]] = y[[40, 3]]
    with pytest.raises(AssertionError):
        X.assert_bitwise(X.rne(bad, BF), want, "swap")
    # truncation instead of round-to-nearest-even (the wide regime: results beyond 256)
    Aw, Ww = X.counting((M, 48), g, -16, 16), X.counting((N, 48), g, -16, 16)
    yw = X.check_exact_gemm(Aw, Ww.t(), out_dtype=F32)
    trunc = (yw.float().view(torch.int32) & ~0xFFFF).view(F32).to(BF)
    with pytest.raises(AssertionError):
        X.assert_bitwise(trunc, X.rne(yw, BF), "trunc")
    # a write into a guard row, and an element never written
    buf = X.guarded(M, N, BF, "cpu")
    buf[:M] = want
    X.assert_guard(buf, M, "guard")
    X.assert_written(buf, M, "written")
    buf[M + 3, 5] = 0.0
    with pytest.raises(AssertionError, match="guard"):
        X.assert_guard(buf, M, "guard")
    buf = X.guarded(M, N, F32, "cpu")
    buf[:M - 1] = y[:M - 1].float()
    with pytest.raises(AssertionError, match="never written"):
        X.assert_written(buf, M, "written")
    # one bf16 ulp: passes at 1 ulp, fails at 2
    ref = torch.tensor([1.0 + 2 ** -9, -3.0, 1e-3], dtype=torch.float64)
    X.assert_ulps(ref.to(BF), ref, "ulp")
    with pytest.raises(AssertionError):
        X.assert_ulps((ref * (1 + 2 ** -6)).to(BF), ref, "ulp")


def test_rne_refuses_double_rounding():
    with pytest.raises(AssertionError):
        X.rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), BF)
    assert X.rne(torch.tensor([257.0, 259.0, 261.0]), BF).tolist() == [256.0, 260.0, 260.0]


# ------------------------------------------------------------------------------------ the full-row kernel's probes
def _lib():
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib
    return _lib.lib()


def _heights(M, E):
    return {h for _, t in X.row_tiles(M, E) for h in t}


@pytest.mark.parametrize("E", [384, 512])
def test_row_tiles_mirror_the_dispatch(E):
    """exact_util.row_tiles against the library's own workgroup count (vg_row_parts is host-only), at every row count a row test
    uses and at every M up to 1280 units: a change of RW_MINUNITS or of the deal fails here, it does not silently shrink coverage"""
    import test_exact_row_gpu as R
    L = _lib()
    Ms = set(X.ROW_M[E]) | {M for M, _ in X.row_cases(E)} | {R.HEAD} | set(R.TALLER[E]) | {16 * un for un in range(1, 1281)}
    Ms |= {1040, 2080, 2096, 4160, 16640, 33280, 66560}
    for M in sorted(Ms):
        tiles = X.row_tiles(M, E)
        assert len(tiles) == L.vg_row_parts(M), M
        assert all(1 <= h <= X.ROW_MAXMT[E] for _, t in tiles for h in t), M
        at = 0
        for first, t in tiles:  # the workgroups tile the rows without gap or overlap
            assert first == at and t, M
            at += 16 * sum(t)
        assert at == M
    rows, owner = X.row_owner(43008, E)
    assert int(rows.sum()) == 43008 and owner.tolist() == sorted(owner.tolist()) and int(owner[-1]) == 255
    assert L.vg_row_parts(8) == 0 and L.vg_row_parts(130) == 0


def test_row_probe_counts_reach_every_height():
    """ROW_M runs every instantiation of the tile body (MT = 1..9 at E = 384, 1..6 at E = 512), alone and as one of several tiles of
    a workgroup; the older row tests, by the same mirror, do not (what their docstrings now say)"""
    for E, top in ((384, 9), (512, 6)):
        assert set().union(*[_heights(M, E) for M in X.ROW_M[E]]) == set(range(1, top + 1)), E
        assert any(len(t) >= 2 for M in X.ROW_M[E] for _, t in X.row_tiles(M, E)), E
        assert any(len(t) >= 3 for _, t in X.row_tiles(66560, 512))
        tall = X.row_tiles(X.ROW_TALL[E], E)
        assert any(len(t) >= 2 for _, t in tall) and top in _heights(X.ROW_TALL[E], E)
        for h in range(1, top + 1):  # 4096 h rows: that height and no other
            assert _heights(4096 * h, E) == {h if h > 1 else 2}, (E, h)
    assert {tuple(t) for _, t in X.row_tiles(38912, 384)} == {(8, 2), (9,)}
    assert {tuple(t) for _, t in X.row_tiles(43008, 384)} == {(8, 2), (8, 3)}
    assert {tuple(t) for _, t in X.row_tiles(66560, 384)} == {(8, 8), (8, 9)}
    assert {tuple(t) for _, t in X.row_tiles(26624, 512)} == {(4, 3), (6,)}
    assert {tuple(t) for _, t in X.row_tiles(43008, 512)} == {(5, 5), (6, 5)}
    assert {tuple(t) for _, t in X.row_tiles(66560, 512)} == {(6, 5, 5), (6, 6, 5)}
    # what the older tests reach: tests/test_row_gpu.py SHAPES / SLN_SHAPES and test_exact_gemm_gpu.py::test_linear_ln_fwd_counting
    shapes = [16, 48, 1040, 2080, 2096, 4160, 16640, 33280, 66560]
    assert set().union(*[_heights(M, 384) for M in shapes]) == {1, 2, 4, 5, 8, 9}
    assert set().union(*[_heights(M, 512) for M in shapes]) == {1, 2, 4, 5, 6}
    for E in (384, 512):
        assert set().union(*[_heights(M, E) for M in (64, 96, 1024, 2048, 8192)]) == {2}
        assert set().union(*[_heights(16 * un, E) for un in range(1, 41)], _heights(16640, E)) == {1, 2, 4, 5}


@pytest.mark.parametrize("E", [384, 512])
def test_row_cases_cover_the_k_loop(E):
    cases = X.row_cases(E)
    assert len(cases) == len(set(cases)) and {M for M, _ in cases} == set(X.ROW_M[E])
    assert X.ROW_K == (128, 192, 320) and [K // 32 for K in X.ROW_K] == [4, 6, 10]  # the ring, a wrap, a wrap that is no multiple of 4
    for M in (16, 48, X.ROW_TALL[E]):
        assert {K for m, K in cases if m == M} == set(X.ROW_K)
    for K in X.ROW_K:  # every K meets tall tiles as well
        assert max(max(_heights(M, E)) for M, k in cases if k == K) == X.ROW_MAXMT[E]
    assert max(M for M, _ in cases) == 66560 and max(K for _, K in cases) == 320


def test_row_probe_dropout_mask():
    """p = 0.5 keeps with the factor exactly 2, and the mask of M * E elements is a prefix of a longer one (elements are addressed by
    their flat index), which is what lets test_exact_row_gpu.py draw it once"""
    import drop_ref
    import test_exact_row_gpu as R
    big, scale = drop_ref.mask(R.DROP_P, R.SEED, R.SITE, None, 48 * 512)
    assert float(scale) == 2.0 and drop_ref.threshold(R.DROP_P) == 128
    for n in (16 * 384, 16 * 512, 48 * 384):
        assert (drop_ref.mask(R.DROP_P, R.SEED, R.SITE, None, n)[0] == big[:n]).all()
    assert 0.45 < big.mean() < 0.55


def _ln(x, eps=0.0):
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    return (x - mu) * rs, rs[:, 0]


@pytest.mark.parametrize("sln", [False, True])
def test_row_bwd_terms_are_the_autograd_gradients(sln):
    """exact_util.row_bwd_terms, the reference of the backward probes, against fp64 autograd of the same operation (with the true
    statistics of x, where the formula IS the gradient)"""
    g = X.gen(3 + sln)
    M, E = 48, 384
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x, d, gres = r(M, E).requires_grad_(True), r(M, E), r(M, E)
    gam, lb, wmod = (1 + 0.2 * r(E)).requires_grad_(True), r(E).requires_grad_(True), r(M, E).requires_grad_(True)
    gs, bs = torch.tensor(0.7, dtype=torch.float64, requires_grad=True), torch.tensor(-0.3, dtype=torch.float64, requires_grad=True)
    h, rs = _ln(x)
    y = wmod * (gs * (h * gam + lb) + bs) if sln else h * gam + lb
    (y * d).sum().backward()
    sl = dict(lb=lb.detach(), wmod=wmod.detach(), gs=float(gs.detach()), bs=float(bs.detach())) if sln else {}
    t = X.row_bwd_terms(d, h.detach(), rs.detach(), gam.detach(), gres, **sl)

    def close(a, b, what):
        assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), what
    close(t["dx"], x.grad + gres, "dx")
    close(t["t_gamma"].sum(0), gam.grad, "d gamma")
    close(t["t_beta"].sum(0), lb.grad, "d beta")
    assert bool((t["dx_mag"] >= t["dx"].abs() * (1 - 1e-12)).all())
    if sln:
        close(t["dw"], wmod.grad, "d w")
        close(t["t_gs"].sum(), gs.grad, "d gs")
        close(t["t_bs"].sum(), bs.grad, "d bs")


@pytest.mark.parametrize("E,sln,bcast", [(384, False, 0), (512, True, 0), (512, True, 32)])
def test_row_bwd_probe_ranges_stay_exact(E, sln, bcast):
    """the ranges of RowBwdProbe keep every product exact in fp32 and every sum of them exact.  Run at a quarter of the largest M of
    the GPU test (at its largest K) against a quarter of the 2^24 budget: the column sums of |terms| over all rows grow with M, so
    the full 66 560 rows stay inside it; there the probe asserts the full budget itself, on the data it launches.  A workgroup's
    share of the column sums is a 256th of this; its d gs / d bs sum over rows AND columns does not grow with M and keeps a factor
    of 2 here, at the tallest workgroups of any M (17 units)."""
    M, K = 16640, 320
    p = X.RowBwdProbe(M, K, E, X.gen(E + sln + bcast), sln=sln, bcast=bcast, limit=X.EXACT_LIMIT / 4)
    assert float(p.d.abs().max()) <= 256 and set(p.rstd.unique().tolist()) == {0.5, 1.0} and set(p.mean.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert X.grid_of(p.h) == 0.5 and float(p.h.abs().max()) == 5.0
    if sln:
        rows, owner = X.row_owner(4 * M, E)  # the workgroups of the largest M: 272 rows each at the most
        assert int(rows.max()) == 272
        p.check_scalar_budget(owner[:M], int(owner[M - 1]) + 1, X.EXACT_LIMIT / 2)


def test_row_checkers_reject_defects():
    """the per-workgroup checks of test_exact_row_gpu.py against simulated defects, from the reference tensors alone: a row lost
    from one workgroup's column sums, a row counted twice, a dx element two bf16 ulps off, a dxm that ignores the mask"""
    M, K, E = 2096, 128, 384
    p = X.RowBwdProbe(M, K, E, X.gen(5))
    rows, owner = X.row_owner(M, E)
    nwg = rows.numel()
    assert set(rows.tolist()) == {16, 32}
    want = X.rne(X.per_workgroup(p.t["t_gamma"], owner, nwg), F32)
    X.assert_bitwise(want.clone(), want, "identity")
    r = int((p.t["t_gamma"].abs().sum(1) > 0).nonzero()[7])
    for sign in (-1.0, 1.0):  # lost, doubled
        bad = X.per_workgroup(p.t["t_gamma"], owner, nwg)
        bad[owner[r]] += sign * p.t["t_gamma"][r]
        with pytest.raises(AssertionError, match="differ"):
            X.assert_bitwise(X.rne(bad, F32), want, "d gamma")
    ref, floor = p.dx(True)
    dx = ref.to(BF)
    X.assert_ulps(dx, ref, "dx", 1.0, floor=floor)
    part = X.per_workgroup(dx, owner, nwg).float()
    X.assert_colsum(part, dx, owner, rows, "colsum")
    for sign in (-1.0, 1.0):
        bad = part.clone()
        bad[owner[r]] += sign * dx[r].float()
        with pytest.raises(AssertionError, match="summation bound"):
            X.assert_colsum(bad, dx, owner, rows, "colsum")
    i = tuple(int(v) for v in (ref.abs() > 1).nonzero()[3])
    off = dx.clone()
    off[i] = float(dx[i]) + 2 * float(X.bf16_ulp(ref[i]))
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_ulps(off, ref, "dx", 1.0, floor=floor)
    with pytest.raises(AssertionError):  # a statistic read from the neighbouring row
        q = X.row_bwd_terms(p.d, (p.x - p.mean.roll(1)[:, None]) * p.rstd[:, None], p.rstd, p.gamma, p.gres)
        X.assert_ulps(q["dx"].to(BF), ref, "dx", 1.0, floor=floor)


def test_row_bwd_partial_rows_are_not_optional_at_the_c_abi():
    """csrc/gemm_row.hip's launcher takes part == nullptr as "input gradient only" (the engine's pass of the generator through D);
    the C entry points do not offer that form: a null `part` is refused on the host, before any launch"""
    import ctypes as C
    L = _lib()
    p = C.c_void_p(4096)  # never dereferenced
    assert L.vg_linear_dgrad_ln_bwd(p, p, p, p, p, p, None, p, None, None, 32, 384, 0.0, 0, 0, None, None) == -1
    assert L.vg_linear_dgrad_ln_bwd_e(512, p, p, p, p, p, p, None, p, None, None, 32, 384, 0.0, 0, 0, None, None) == -1
    assert L.vg_linear_dgrad_sln_bwd(p, p, p, 0, p, p, p, p, p, p, p, None, p, None, p, 0, None, 32, 384, 0.0, 0, 0, None, None) == -1
