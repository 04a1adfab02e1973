"""Precision / recall / density / coverage and KID on the GPU: vg_knn_radii, vg_ball_counts and vg_poly_kernel_sum held to int64
arithmetic on integer features - radii, counts and minima EXACT, ties included, which is what tells ``<=`` from ``<`` and the k-th from
the (k +- 1)-th - and to the Gram-identity bound 4 (d + 2) 2^-53 (|a|^2 + |b|^2) on normal ones (one set offset by a mean of 100), with
the counts exactly those of tests/manifold_ref.py (test_manifold_cpu.py shows every comparison of these cases sits 1000 bounds from
flipping); duplicates at distance exactly 0.0; bit-equal reruns and invariance under a permutation of the centres; the kernel sum
exact on integers and inside the worst-case accumulation bound elsewhere; every refusal with the outputs untouched; the evaluator
against the restatement on its own features; the trainer's header line and epoch fields.
Every test here fails on the parent commit: no exports, no functions, no keywords."""
import os
import re

import numpy as np
import pytest
import torch

import gpu_util as u
import manifold_ref as mf

pytestmark = pytest.mark.gpu

GUARD = -7.25
PAD = 64  # guard words in front of and behind every output


def _guarded(n, dtype):
    buf = torch.full((2 * PAD + n,), GUARD if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _intact(buf, n):
    fill = GUARD if buf.dtype.is_floating_point else -7
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def _ws(nq, nc, k):
    from vit_gan_amd import _lib
    nbytes = _lib.lib().vg_pair_ws_bytes(nq, nc, k)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def _dev(x, pad=16):
    """a numpy [n, d] set as fp32 on the device with row stride d + pad; the padding columns would wreck any sum they entered"""
    x = np.asarray(x)
    wide = torch.full((x.shape[0], x.shape[1] + pad), 1e30, dtype=torch.float32)
    wide[:, :x.shape[1]] = torch.from_numpy(x.astype(np.float32))
    view = wide.cuda()[:, :x.shape[1]]
    assert view.stride(0) == x.shape[1] + pad
    return view


def _radii(xd, k):
    n, d = xd.shape
    buf, rad2 = _guarded(n, torch.float64)
    u.call("vg_knn_radii", u.ptr(xd), xd.stride(0), n, d, k, u.ptr(rad2), u.ptr(_ws(n, n, k)), u.stream())
    u.sync()
    assert _intact(buf, n), "a guard word around rad2 was written"
    return rad2.cpu().numpy().copy()


def _balls(qd, cd, rad2_c):
    nq, d = qd.shape
    nc = cd.shape[0]
    bc, count = _guarded(nq, torch.int32)
    bm, min_d2 = _guarded(nq, torch.float64)
    rd = torch.from_numpy(np.asarray(rad2_c, dtype=np.float64)).cuda()
    u.call("vg_ball_counts", u.ptr(qd), qd.stride(0), nq, u.ptr(cd), cd.stride(0), nc, d, u.ptr(rd), u.ptr(count), u.ptr(min_d2),
           u.ptr(_ws(nq, nc, 0)), u.stream())
    u.sync()
    assert _intact(bc, nq) and _intact(bm, nq), "a guard word around count / min_d2 was written"
    return count.cpu().numpy().copy(), min_d2.cpu().numpy().copy()


def _ksum(qd, cd, skip):
    nq, d = qd.shape
    nc = cd.shape[0]
    buf, out = _guarded(1, torch.float64)
    u.call("vg_poly_kernel_sum", u.ptr(qd), qd.stride(0), nq, u.ptr(cd), cd.stride(0), nc, d, int(skip), u.ptr(out), u.ptr(_ws(nq, nc, 0)),
           u.stream())
    u.sync()
    assert _intact(buf, 1), "a guard word around the sum was written"
    return float(out.cpu()[0])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


# ------------------------------------------------------------------------------------------------------ integer features: exact
# the launcher's paths (csrc/pairwise.hip, pair_plan): centre tiles go in groups of 4 (64 rows), and a launch takes
# min(groups, ceil(2048 / query tiles), 64) column splits.  n <= 64: one group, ONE split, the kernel stores rad2 itself;
# n = 100: 2 groups -> 2 splits and the merge launch;  n = 257: 5 groups -> 5 splits and the merge launch, the last split a
# single row of the last tile.
NS = (None, 16, 17, 33, 100, 257)  # None: k + 1, the smallest legal set


@pytest.mark.parametrize("d", [16, 48, 384])
def test_knn_radii_are_exact_on_integers(d):
    seen = 0
    for k in (1, 3, 5, 8):
        for n in NS:
            n = k + 1 if n is None else n
            # values in [-2, 2]: neighbours tie all the time at d = 16; three exact copies of row 0 besides
            x = mf.integer_set(n, d, seed=1000 * d + 10 * n + k, lo=-2, hi=2, copies=min(3, n - 2))
            want = mf.radii(x, k)
            got = _radii(_dev(x), k)
            bad = np.argwhere(got != want.astype(np.float64))
            assert bad.size == 0, (d, n, k, bad[:4].ravel().tolist(), got[bad[:4].ravel()], want[bad[:4].ravel()])
            seen += 1
    assert seen == 4 * len(NS)


# (nq, nc): nq != nc on both sides of the 16-row tile edge and of the 64-row group edge.  nc <= 64: one split, stored by the kernel;
# (100, 257): 5 splits + merge;  (5, 300): 5 splits + merge with a single query tile;  (257, 100): 2 splits + merge
BALL_SHAPES = [(15, 17), (17, 15), (16, 16), (33, 64), (64, 65), (65, 63), (100, 257), (5, 300), (257, 100)]


@pytest.mark.parametrize("d", [16, 384])
def test_ball_counts_are_exact_on_integers(d):
    for nq, nc in BALL_SHAPES:
        c = mf.integer_set(nc, d, seed=7 * nq + nc + d, lo=-2, hi=2, copies=3)
        q = mf.integer_set(nq, d, seed=11 * nq + nc + d, lo=-2, hi=2)
        q[-1] = c[0]  # a query ON a centre (and on its three copies): distance 0 against radius 0 when k <= 3
        q[0] = c[1]
        for k in (3, 5):
            rad = mf.radii(c, k)
            assert rad[0] == 0 if k <= 3 else rad[0] > 0
            want_c, want_m = mf.ball_counts(q, c, rad)
            got_c, got_m = _balls(_dev(q), _dev(c), rad)
            assert np.array_equal(got_c.astype(np.int64), want_c), (d, nq, nc, k, np.argwhere(got_c != want_c)[:4].ravel().tolist())
            assert np.array_equal(got_m, want_m.astype(np.float64)), (d, nq, nc, k)
            if k == 3:  # the criterion has teeth: a strict comparison loses the query that sits on a centre of radius 0
                assert not np.array_equal((mf.d2(q, c) < rad[None, :]).sum(1), want_c)


# -------------------------------------------------------------------------------------------------------- normal features: bound
@pytest.mark.parametrize("name", sorted(mf.NORMAL_CASES))
def test_normal_features_within_the_gram_bound_and_counts_equal(name):
    nq, nc, d, k, mean, _ = mf.NORMAL_CASES[name]
    q, c = mf.normal_case(name)
    qd, cd = _dev(q), _dev(c)
    for x, xd in ((q, qd), (c, cd)):
        # the k-th smallest is 1-Lipschitz in the sup norm of its row: |rad2 - ref| <= max_j bound_ij
        want, lim = mf.radii(x, k), mf.gram_bound(x, x).max(1)
        got = _radii(xd, k)
        err = np.abs(got - want)
        print(f"{name} n={len(x)}: rad2 worst err/limit {float((err / lim).max()):.3e}, |rad2| {float(want.max()):.3e}")
        assert (err <= lim).all()
    rad = mf.radii(c, k)
    assert mf.margin(q, c, rad) > mf.margin_needed(d)  # held by the seeds: test_manifold_cpu.py
    want_c, want_m = mf.ball_counts(q, c, rad)
    got_c, got_m = _balls(qd, cd, rad)
    lim = mf.gram_bound(q, c)[np.arange(nq), mf.d2(q, c).argmin(1)]
    print(f"{name}: min_d2 worst err/limit {float((np.abs(got_m - want_m) / lim).max()):.3e}; counts {int(want_c.sum())} of {nq * nc}")
    assert (np.abs(got_m - want_m) <= mf.gram_bound(q, c).max(1)).all()
    assert np.array_equal(got_c.astype(np.int64), want_c)
    assert 0 < want_c.sum() < nq * nc
    if mean:  # fp32 products would be off by ~1e-7 |a|^2 ~ 0.05 d here, far outside: this is fp64 throughout
        assert float(np.abs(got_m - want_m).max()) < 1e-6 * float(want_m.min())


# ------------------------------------------------------------------------------------------------------------------ duplicates
@pytest.mark.parametrize("mean", [0.0, 100.0])
def test_bit_equal_rows_are_at_distance_exactly_zero(mean):
    n, d, k = 70, 384, 3
    g = np.random.default_rng(8)
    x = (mean + g.standard_normal((n, d))).astype(np.float32)
    x[[20, 45, 69]] = x[3]  # four bit-equal rows across three tiles and two groups: each has k = 3 neighbours at 0
    x[17] = x[5]            # a pair: its nearest neighbour at 0, its 3rd elsewhere
    xd = _dev(x)
    rad = _radii(xd, k)
    assert all(rad[i] == 0.0 and not np.signbit(rad[i]) for i in (3, 20, 45, 69)), rad[[3, 20, 45, 69]]
    assert rad[5] > 0 and rad[17] == rad[5]
    r1 = _radii(xd, 1)
    assert r1[5] == 0.0 and r1[17] == 0.0 and (np.delete(r1, [3, 5, 17, 20, 45, 69]) > 0).all()
    # queries that ARE centres: min_d2 exactly 0.0, and a centre of radius 0 counts its own copy (inclusive comparison)
    q = x[[3, 5, 9]]
    zero = np.zeros(n)
    cnt, mn = _balls(_dev(q), xd, zero)
    assert mn.tolist() == [0.0, 0.0, 0.0] and cnt.tolist() == [4, 2, 1]
    cnt, _ = _balls(_dev(q), xd, rad)
    want, _ = mf.ball_counts(q, x, mf.radii(x, k))
    assert np.array_equal(cnt.astype(np.int64), want) and cnt[0] >= 4


# ----------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_are_bit_equal_and_centre_order_does_not_matter():
    q, c = mf.normal_case("unit-48")  # 100 x 257: five splits and the merge launch
    nq, nc, d, k, _, _ = mf.NORMAL_CASES["unit-48"]
    qd, cd = _dev(q), _dev(c)
    rad = _radii(cd, k)
    assert np.array_equal(_bits(rad), _bits(_radii(cd, k)))
    cnt, mn = _balls(qd, cd, rad)
    cnt2, mn2 = _balls(qd, cd, rad)
    assert np.array_equal(cnt, cnt2) and np.array_equal(_bits(mn), _bits(mn2))
    for skip in (0, 1):
        assert _ksum(qd, cd, skip) == _ksum(qd, cd, skip) and _ksum(cd, cd, skip) == _ksum(cd, cd, skip)
    perm = np.random.default_rng(9).permutation(nc)
    cp = _dev(c[perm])
    radp = _radii(cp, k)
    assert np.array_equal(_bits(radp), _bits(rad[perm])), "a radius depends on where its row and its neighbours sit"
    cntp, mnp = _balls(qd, cp, rad[perm])
    assert np.array_equal(cntp, cnt) and np.array_equal(_bits(mnp), _bits(mn))
    # and the two sides of a pair see the same distance: d2(q_i, c_j) as a query's minimum and as a centre's
    _, mn_c = _balls(cd, qd, np.zeros(nq))
    full = mf.d2(q, c)
    i = int(full.min(1).argmin())
    j = int(full[i].argmin())
    if int(full[:, j].argmin()) == i:
        assert mn[i] == mn_c[j]


# ------------------------------------------------------------------------------------------------------------------ kernel sum
@pytest.mark.parametrize("d", [16, 64])
def test_kernel_sum_is_exact_on_integers(d):
    """entries in [-2, 2], d a power of two: t = q.c / d + 1 has at most 6 fraction bits and |t| <= 5, t^3 at most 18 and |t^3| <= 125,
    the sum of up to 257 * 257 of them stays below 2^24 with 18 fraction bits: every term, partial and total is exact in fp64"""
    for nq, nc in ((33, 100), (100, 257), (257, 257), (16, 16)):
        q, c = mf.integer_set(nq, d, seed=nq + d, lo=-2, hi=2), mf.integer_set(nc, d, seed=nc + d + 1, lo=-2, hi=2)
        qd, cd = _dev(q), _dev(c)
        for skip in (0, 1):
            num, den = mf.kernel_sum_int(q, c, skip)
            assert _ksum(qd, cd, skip) == num / den, (d, nq, nc, skip)
        # skip_diagonal leaves out exactly the i == j terms (min(nq, nc) of them)
        diag = sum(int(q[i] @ c[i] + d) ** 3 for i in range(min(nq, nc)))
        assert _ksum(qd, cd, 0) - _ksum(qd, cd, 1) == diag / d ** 3


@pytest.mark.parametrize("name", sorted(mf.NORMAL_CASES))
def test_kernel_sum_within_the_accumulation_bound(name):
    q, c = mf.normal_case(name)
    qd, cd = _dev(q), _dev(c)
    for a, ad, b, bd, skip in ((q, qd, c, cd, 0), (c, cd, c, cd, 1), (q, qd, q, qd, 1), (c, cd, q, qd, 0)):
        got, want, lim = _ksum(ad, bd, skip), mf.kernel_sum(a, b, skip), mf.kernel_sum_bound(a, b)
        print(f"{name} {len(a)} x {len(b)} skip={skip}: {got!r} vs {want!r}, err/limit {abs(got - want) / lim:.3e}")
        assert abs(got - want) <= lim
        if skip:
            assert abs((_ksum(ad, bd, 0) - got) - float(np.trace(mf.kappa(a, b)))) <= lim


# ---------------------------------------------------------------------------------------------------------------- return codes
def test_refusals_leave_the_outputs_untouched():
    from vit_gan_amd import _lib
    lib = _lib.lib()
    n, d = 40, 32
    x = torch.randn(n, d, device="cuda")
    ws = _ws(n, n, 8)
    br, rad2 = _guarded(n, torch.float64)
    bc, count = _guarded(n, torch.int32)
    bm, min_d2 = _guarded(n, torch.float64)
    bs, out = _guarded(1, torch.float64)
    rad2.fill_(3.5), count.fill_(35), min_d2.fill_(3.5), out.fill_(3.5)
    rc = torch.zeros(n, dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    knn = lambda X=x, ld=d, n_=n, d_=d, k=3, r=rad2, w=ws: lib.vg_knn_radii(P(X), ld, n_, d_, k, P(r), P(w), u.stream())  # noqa: E731
    ball = lambda Q=x, ldq=d, nq=n, Cn=x, ldc=d, nc=n, d_=d, r=rc, c=count, m=min_d2, w=ws: lib.vg_ball_counts(  # noqa: E731
        P(Q), ldq, nq, P(Cn), ldc, nc, d_, P(r), P(c), P(m), P(w), u.stream())
    ksum = lambda Q=x, ldq=d, nq=n, Cn=x, ldc=d, nc=n, d_=d, o=out, w=ws: lib.vg_poly_kernel_sum(  # noqa: E731
        P(Q), ldq, nq, P(Cn), ldc, nc, d_, 0, P(o), P(w), u.stream())
    assert knn(X=None) == knn(r=None) == knn(w=None) == knn(n_=0) == knn(n_=-2) == -1
    assert ball(Q=None) == ball(Cn=None) == ball(r=None) == ball(c=None) == ball(m=None) == ball(w=None) == ball(nq=0) == ball(nc=0) == -1
    assert ksum(Q=None) == ksum(Cn=None) == ksum(o=None) == ksum(w=None) == ksum(nq=0) == ksum(nc=-1) == -1
    for bad in (0, 8, 24, 2064, 4096, -16):
        assert knn(d_=bad, ld=8192) == ball(d_=bad, ldq=8192, ldc=8192) == ksum(d_=bad, ldq=8192, ldc=8192) == -2, bad
    assert knn(ld=d - 1) == ball(ldq=d - 1) == ball(ldc=d - 1) == ksum(ldq=d - 1) == ksum(ldc=d - 1) == -2
    assert knn(k=0) == knn(k=9) == knn(k=-1) == knn(k=3, n_=3) == knn(k=8, n_=8) == -3
    assert lib.vg_pair_ws_bytes(0, 4, 1) == lib.vg_pair_ws_bytes(4, 0, 1) == lib.vg_pair_ws_bytes(4, 4, 9) == lib.vg_pair_ws_bytes(4, 4, -1) == -1
    u.sync()
    for buf, view, fill in ((br, rad2, 3.5), (bc, count, 35), (bm, min_d2, 3.5), (bs, out, 3.5)):
        assert _intact(buf, view.numel()) and bool((view == fill).all()), "a refused call wrote to an output"
    assert knn() == ball() == ksum() == 0  # and the same arguments, legal, run
    u.sync()
    assert bool((rad2 > 0).all()) and bool((count >= 1).all()) and bool((min_d2 == 0).all())


# --------------------------------------------------------------------------------------------------------------- the Python API
def test_python_api_on_device_tensors():
    from vit_gan_amd import metrics as M
    q, c = mf.normal_case("offset100-48")
    k = mf.NORMAL_CASES["offset100-48"][3]
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    rad = M.knn_radii(cd, k)
    assert rad.dtype == torch.float64 and rad.is_cuda and np.array_equal(rad.cpu().numpy(), _radii(_dev(c), k))  # ld does not matter
    cnt, mn = M.ball_counts(qd, cd, rad)
    assert cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy().astype(np.int64), mf.ball_counts(q, c, mf.radii(c, k))[0])
    assert M.prdc(cd, qd, k) == mf.prdc(c, q, k)
    got, want = M.kid(cd, qd), mf.kid(c, q)
    assert abs(got - want) <= mf.kid_bound(c, q), (got, want)
    assert float(M.poly_kernel_sum(qd, cd, True)) == _ksum(_dev(q), _dev(c), 1)
    # bf16 rows are widened; a transposed view is made contiguous
    xb = torch.from_numpy(q).to(torch.bfloat16)
    assert torch.equal(M.knn_radii(xb.cuda(), k), M.knn_radii(xb.float().cuda(), k))
    with pytest.raises(ValueError):
        M.ball_counts(qd, cd.cpu(), rad)


# ------------------------------------------------------------------------------------------------------------------- evaluator
class _Stub(torch.nn.Module):
    """latent -> image by one fixed map; counts its calls"""

    def __init__(self, gain):
        super().__init__()
        self.latent, self.calls = 8, 0
        self.w = torch.nn.Parameter((torch.randn(8, 3 * 8 * 8, generator=torch.Generator().manual_seed(2)) * gain).cuda())

    def forward(self, z):
        self.calls += 1
        return torch.tanh(z @ self.w).reshape(-1, 3, 8, 8)


class _Projection:
    """images [n, 3, 8, 8] -> [n, 32] fp32 on the device; counts its calls"""

    def __init__(self):
        self.p = torch.randn(192, 32, generator=torch.Generator().manual_seed(3)).cuda()
        self.calls = 0

    def __call__(self, x):
        self.calls += 1
        return x.reshape(x.shape[0], -1) @ self.p


def _check_against_restatement(ev, k):
    real, fake = ev.bank["feats"].cpu().numpy(), ev.fake_feats.cpu().numpy()
    d = real.shape[1]
    need, worst = mf.margin_needed(d), mf.case_margin(real, fake, k)
    print(f"margin {worst:.3e}, needed {need:.3e}")
    assert worst > need  # the features are the run's own: the precondition of exact ratios, checked where they are known
    want = mf.prdc(real, fake, k)
    for key in ("precision", "recall", "density", "coverage"):
        assert ev.last[key] == want[key], (key, ev.last[key], want[key])
    assert abs(ev.last["kid"] - mf.kid(real, fake)) <= mf.kid_bound(real, fake)
    print({key: ev.last[key] for key in ("precision", "recall", "density", "coverage", "kid")})
    return want


def test_evaluator_with_a_callable_against_the_restatement(tmp_path):
    from vit_gan_amd.data import DeviceDataset
    from vit_gan_amd.metrics import FrechetDistance
    images = torch.randint(0, 256, (150, 3, 8, 8), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    ds = DeviceDataset(images, None, layout="nchw", device="cuda")
    f_on, f_off, G = _Projection(), _Projection(), _Stub(0.4)
    on = FrechetDistance(f_on, n_fake=70, batch=32, seed=7, manifold_k=3, kid=True, bank_real=40).fit_real(ds)
    off = FrechetDistance(f_off, n_fake=70, batch=32, seed=7).fit_real(ds)
    assert f_on.calls == f_off.calls == 5  # the bank is rows of the one pass over the 150 images
    picks = torch.tensor([(j * 150) // 40 for j in range(40)])
    whole = torch.cat([f_on(ds.decode(torch.arange(lo, min(lo + 32, 150)))) for lo in range(0, 150, 32)])  # the same batches
    assert torch.equal(on.bank["feats"], whole[picks.cuda()]) and on.bank["k"] == 3 and on.bank["rad2"].shape == (40,)
    f_on.calls = f_off.calls = 0
    d_on, calls = on(G), G.calls
    d_off = off(G)
    assert (f_on.calls, calls) == (f_off.calls, G.calls - calls) == (3, 3)  # launch for launch today's evaluation
    assert d_on == d_off and off.bank is None and off.fake_feats is None
    assert set(off.last) == {"distance", "mean_term", "trace_term", "n_real", "n_fake"}
    assert all(on.last[key] == off.last[key] for key in off.last)
    assert set(on.last) == set(off.last) | {"precision", "recall", "density", "coverage", "kid", "manifold_k", "n_real_bank"}
    assert (on.last["manifold_k"], on.last["n_real_bank"]) == (3, 40) and on.fake_feats.shape == (70, 32)
    want = _check_against_restatement(on, 3)
    assert 0 < want["precision"] and 0 < want["coverage"]
    # the statistics file: same arrays with the options off, the bank under new keys with them on; it round-trips
    p_on, p_off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    on.save_real(p_on), off.save_real(p_off)
    with np.load(p_on) as a, np.load(p_off) as b:
        assert set(b.files) == {"mean", "cov", "n", "d", "tag", "lut"} and set(a.files) == set(b.files) | {"bank_feats", "bank_k", "bank_rad2", "bank_self_sum"}
        assert all(np.array_equal(a[key], b[key]) for key in b.files)
    again = FrechetDistance(f_on, n_fake=70, batch=32, seed=7, manifold_k=3, kid=True, tag=on.tag).load_real(p_on)
    assert again(G) == d_on and again.last == on.last
    other_k = FrechetDistance(f_on, n_fake=70, batch=32, seed=7, manifold_k=5, tag=on.tag).load_real(p_on)  # radii recomputed at its k
    other_k(G)
    assert other_k.last["density"] == mf.prdc(on.bank["feats"].cpu().numpy(), on.fake_feats.cpu().numpy(), 5)["density"]
    assert other_k.last["kid"] != other_k.last["kid"]
    assert FrechetDistance(f_off, n_fake=70, batch=32, seed=7, tag=on.tag).load_real(p_on)(G) == d_on  # a bank nobody asked for is no harm
    for kw, name in (({"manifold_k": 3}, "manifold_k"), ({"kid": True}, "kid")):
        with pytest.raises(ValueError, match=name):
            FrechetDistance(f_on, n_fake=70, tag=on.tag, **kw).load_real(p_off)


def test_evaluator_on_a_frozen_vit_against_the_restatement():
    from vit_gan_amd.data import DeviceDataset
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.metrics import FrechetDistance
    dims = dict(n_channels=3, embed_dim=128, n_layers=2, n_attention_heads=4, forward_mul=2, image_size=32, patch_size=4)
    images = torch.randint(0, 256, (120, 3, 32, 32), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    ds = DeviceDataset(images, None, device="cuda")
    ev = FrechetDistance.random_vit(dims, seed=5, latent_seed=3, n_fake=96, batch=32, manifold_k=3, kid=True, bank_real=100).fit_real(ds)
    plain = FrechetDistance.random_vit(dims, seed=5, latent_seed=3, n_fake=96, batch=32).fit_real(ds)
    torch.manual_seed(0)
    G = SirenGenerator(embed=128, layers=1, siren_hidden=256, dropout=0.0).cuda().train()
    dist = ev(G)
    assert dist == plain(G) and G.training and ev.last["n_real_bank"] == 100
    _check_against_restatement(ev, 3)
    first = dict(ev.last)
    assert ev(G) == dist and ev.last == first  # bit for bit again


# --------------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_reports_the_manifold_metrics(tmp_path):
    from vit_gan_amd.data import DeviceDataset
    from vit_gan_amd.training import train_model
    cfg = {"epochs": 1, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}
    images = torch.randint(0, 256, (20, 3, 32, 32), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)
    ds = DeviceDataset(images, None, device="cuda")  # 20 images, batch 8: one epoch of two steps
    out = train_model(cfg, dataset=ds, output_base=str(tmp_path), fid="random-vit", fid_samples=32, manifold_k=3, kid=True)
    log = open(os.path.join(out["dirs"].save, "training.log")).read()
    assert "Exception" not in log
    assert re.search(r"Manifold metrics: 20 real feature rows kept; precision / recall / density / coverage with k = 3; KID", log), log
    m = re.search(r"Epoch \[0/1\] \| Disc Loss: \S+, Gen Loss: \S+ \| FID: (\S+) \| P: (\S+) R: (\S+) D: (\S+) C: (\S+) \| KID: (\S+)\n", log)
    assert m, log
    vals = [float(v) for v in m.groups()]
    assert all(np.isfinite(vals)) and all(0.0 <= v <= 1.0 for v in (vals[1], vals[2], vals[4])) and vals[3] >= 0.0
    (d_loss, g_loss, q), = out["history"]
    assert set(q) == {"precision", "recall", "density", "coverage", "kid"} and all(np.isfinite(list(q.values())))
    assert q == {key: out["fid"].last[key] for key in q} and abs(q["precision"] - vals[1]) <= 5.1e-5
    with np.load(os.path.join(out["dirs"].save, "real_stats.npz")) as z:
        assert z["bank_feats"].shape == (20, 128) and int(z["bank_k"]) == 3
