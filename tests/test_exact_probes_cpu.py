"""The exact probes of test_exact_gemm_gpu.py / test_exact_attention_gpu.py, checked without a GPU: every probe family
meets its preconditions at the shapes the GPU tests use, the constructed expectations equal the fp64 torch result of the
same operation, the shape tables reach every kernel of the dispatch, and each checker rejects simulated kernel defects."""
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
