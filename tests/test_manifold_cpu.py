"""Precision / recall / density / coverage and KID without a GPU: the restatement (tests/manifold_ref.py) and the CPU path of the
Python API on configurations whose answers are known in closed form; the two against each other; the criterion the GPU tests apply
(exact radii / counts / minima, the Gram bound) REJECTING seven planted defects, each implemented here and never in product code; the
margins that make exact counts a fair demand of the GPU; the caller's errors of the new functions, evaluator options and trainer
options; the new symbols in the header and the binding.  Every test here fails on the parent commit: no functions, no keywords, no
exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import manifold_ref as mf
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib
from vit_gan_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_pair_ws_bytes", "vg_knn_radii", "vg_ball_counts", "vg_poly_kernel_sum")


def _t(x):
    return torch.from_numpy(np.asarray(x).astype(np.float32))


def _api_prdc(real, fake, k):
    return M.prdc(_t(real), _t(fake), k)


# -------------------------------------------------------------------------------------------------------------------- analytic
def _line(n, step=1, at=0, d=16):
    x = np.zeros((n, d), dtype=np.int64)
    x[:, 3] = at + step * np.arange(n)
    return x


def test_points_on_a_line_have_known_radii():
    """x_i = i e_3 in d = 16: the k-th neighbour of an interior point is ceil(k / 2) away, of the end point k away"""
    n = 12
    x = _line(n)
    for k in (1, 2, 3, 4, 5, 8):
        want = np.array([sorted(abs(i - j) for j in range(n) if j != i)[k - 1] ** 2 for i in range(n)])
        assert want[0] == k * k and want[5] == ((k + 1) // 2) ** 2
        assert np.array_equal(mf.radii(x, k), want)
        got = M.knn_radii(_t(x), k)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want.astype(np.float64))


def test_fakes_on_one_of_two_clusters():
    """reals at 0, 2, .. on a line and the same shifted far away; fakes at the odd points of the first cluster, k = 2: every fake is
    1 from a real whose radius is at least 2 (precision 1), every real of the first cluster 1 from a fake of radius at least 2, none of
    the second (recall 1/2, coverage 1/2); each fake lies in the balls of the reals within their radius - 2 (4 at the ends)"""
    m, k = 10, 2
    near, far = _line(m, 2), _line(m, 2)
    far[:, 7] = 1000
    real, fake = np.concatenate([near, far]), _line(m, 2, at=1)
    for got in (mf.prdc(real, fake, k), _api_prdc(real, fake, k)):
        assert got["precision"] == 1.0 and got["recall"] == 0.5 and got["coverage"] == 0.5
        # fake 2i + 1: reals 2i and 2i + 2 (radius 2) at 1; real 0 (radius 4) reaches 1 and 3, real 2m - 2 (radius 4) 2m - 1 and 2m - 5
        assert got["density"] == (2 * m - 1 + 2) / (k * m)


def test_identical_sets():
    """generic points against themselves: each is in its own ball and in those of the k points it is among the k nearest of...
    counted from the balls' side, ball j holds j and its k nearest: sum = n (k + 1), density (k + 1) / k; precision, recall and
    coverage are 1.  The unbiased MMD^2 of a sample against ITSELF is 2 / n^2 (S_off / (n - 1) - S_diag), not 0 (the cross term
    keeps the diagonal); it is exactly 0 where every row is the same row, whatever the row."""
    g = np.random.default_rng(0)
    x = g.standard_normal((40, 16)).astype(np.float32)
    for k in (1, 3, 8):
        for got in (mf.prdc(x, x, k), M.prdc(torch.from_numpy(x), torch.from_numpy(x), k)):
            assert got == {"precision": 1.0, "recall": 1.0, "density": (k + 1) / k, "coverage": 1.0}
    kap = mf.kappa(x, x)
    closed = 2.0 / 40 ** 2 * ((kap.sum() - np.trace(kap)) / 39 - np.trace(kap))
    for got in (mf.kid(x, x), M.kid(torch.from_numpy(x), torch.from_numpy(x))):
        assert abs(got - closed) <= 1e-12 * np.abs(kap).mean()
    same = np.tile(np.arange(-8, 8, dtype=np.int64), (9, 1))  # nine copies of one integer row: every kappa is (344 / 16 + 1)^3, exact
    assert mf.kid(same, same) == 0.0 and M.kid(_t(same), _t(same)) == 0.0
    got = _api_prdc(same, same, 3)  # all radii 0, all distances 0: every point in every ball
    assert got == mf.prdc(same, same, 3) == {"precision": 1.0, "recall": 1.0, "density": 9 / 3, "coverage": 1.0}


# --------------------------------------------------------------------------------------------- the CPU path = the restatement
@pytest.mark.parametrize("name", sorted(mf.NORMAL_CASES))
def test_cpu_path_equals_the_restatement(name):
    nq, nc, d, k, _, _ = mf.NORMAL_CASES[name]
    q, c = mf.normal_case(name)
    tq, tc = torch.from_numpy(q), torch.from_numpy(c)
    rad = M.knn_radii(tc, k)
    want = mf.radii(c, k)
    assert rad.shape == (nc,) and np.abs(rad.numpy() - want).max() <= 1e-12 * want.max()
    cnt, mn = M.ball_counts(tq, tc, torch.from_numpy(want))
    want_c, want_m = mf.ball_counts(q, c, want)
    assert cnt.dtype == torch.int32 and np.array_equal(cnt.numpy().astype(np.int64), want_c)
    assert np.abs(mn.numpy() - want_m).max() <= 1e-12 * want_m.max()
    assert M.prdc(tc, tq, k) == mf.prdc(c, q, k)
    for skip in (False, True):
        a, b = (tq, tc) if not skip else (tc, tc)
        got, ref = float(M.poly_kernel_sum(a, b, skip)), mf.kernel_sum(a.numpy(), b.numpy(), skip)
        assert abs(got - ref) <= mf.kernel_sum_bound(a.numpy(), b.numpy())
    assert abs(M.kid(tc, tq) - mf.kid(c, q)) <= mf.kid_bound(c, q)


def test_cpu_path_is_exact_on_integers_with_ties():
    c, q = mf.integer_set(70, 16, seed=1, lo=-2, hi=2, copies=3), mf.integer_set(33, 16, seed=2, lo=-2, hi=2)
    q[-1] = c[0]
    for k in (1, 3, 5):
        rad = mf.radii(c, k)
        assert np.array_equal(M.knn_radii(_t(c), k).numpy(), rad.astype(np.float64))
        cnt, mn = M.ball_counts(_t(q), _t(c), torch.from_numpy(rad.astype(np.float64)))
        want_c, want_m = mf.ball_counts(q, c, rad)
        assert np.array_equal(cnt.numpy().astype(np.int64), want_c) and np.array_equal(mn.numpy(), want_m.astype(np.float64))
    num, den = mf.kernel_sum_int(q, c)
    assert float(M.poly_kernel_sum(_t(q), _t(c))) == num / den == mf.kernel_sum(q, c)


# ------------------------------------------------------------------------------------------------------------ planted defects
def _tie_case():
    """integers with exact duplicates and a query on a centre: ties everywhere"""
    c, q = mf.integer_set(40, 16, seed=3, lo=-2, hi=2, copies=3), mf.integer_set(20, 16, seed=4, lo=-2, hi=2)
    q[-1] = c[0]
    return q, c


def test_the_criterion_rejects_self_in_the_neighbour_search():
    q, c = _tie_case()
    with_self = np.sort(mf.d2(c, c), axis=1)[:, 3 - 1]  # the row's own 0 takes a place
    assert not np.array_equal(with_self, mf.radii(c, 3))
    x = _line(12)
    assert np.array_equal(np.sort(mf.d2(x, x), axis=1)[:, 0], np.zeros(12)) and (mf.radii(x, 1) == 1).all()


def test_the_criterion_rejects_k_off_by_one():
    q, c = _tie_case()
    x = _line(12)
    for k in (2, 3, 5):
        for wrong in (k - 1, k + 1):
            assert not np.array_equal(mf.radii(c, wrong), mf.radii(c, k))
            assert not np.array_equal(mf.ball_counts(q, c, mf.radii(c, wrong))[0], mf.ball_counts(q, c, mf.radii(c, k))[0])
    assert not np.array_equal(mf.radii(x, 1), mf.radii(x, 2)) and np.array_equal(mf.radii(x, 1)[1:-1], mf.radii(x, 2)[1:-1])  # the ends tell


def test_the_criterion_rejects_a_strict_comparison_on_duplicates():
    q, c = _tie_case()
    rad = mf.radii(c, 3)
    assert rad[0] == 0  # three copies elsewhere
    want, _ = mf.ball_counts(q, c, rad)
    strict = (mf.d2(q, c) < rad[None, :]).sum(1)
    assert strict[-1] < want[-1] and want[-1] >= 4 and not np.array_equal(strict, want)


def _spread_case():
    """tight fakes inside a wide real cloud: the two sets' radii differ by far"""
    g = np.random.default_rng(5)
    return g.standard_normal((60, 16)).astype(np.float32), (0.05 * g.standard_normal((50, 16))).astype(np.float32)


def test_the_criterion_rejects_precision_with_the_queries_radii():
    real, fake = _spread_case()
    k = 3
    want = mf.prdc(real, fake, k)
    wrong = int(((mf.d2(fake, real) <= mf.radii(fake, k)[:, None]).sum(1) > 0).sum()) / len(fake)  # each fake's OWN radius
    assert want["precision"] == 1.0 and wrong == 0.0
    assert _api_prdc(real, fake, k) == want


def test_the_criterion_rejects_coverage_with_any_ball():
    real, fake = _spread_case()
    k = 3
    want = mf.prdc(real, fake, k)
    rad_r = mf.radii(real, k)
    dd = mf.d2(real, fake)
    any_ball = int((dd.min(1) <= rad_r.max()).sum()) / len(real)       # some real's ball, not the point's own
    other_set = int((dd <= mf.radii(fake, k)[None, :]).any(1).sum()) / len(real)  # the fakes' balls: that is recall
    assert any_ball != want["coverage"] and other_set != want["coverage"] and other_set == want["recall"]
    assert 0 < want["coverage"] < 1 and _api_prdc(real, fake, k)["coverage"] == want["coverage"]


def test_the_criterion_rejects_kid_with_the_diagonal():
    q, c = mf.normal_case("unit-48")
    M_, N = len(q), len(c)
    biased = mf.kernel_sum(q, q) / (M_ * (M_ - 1)) + mf.kernel_sum(c, c) / (N * (N - 1)) - 2 * mf.kernel_sum(q, c) / (M_ * N)
    assert abs(biased - mf.kid(c, q)) > 1000 * mf.kid_bound(c, q)
    same = np.tile(np.arange(-8, 8, dtype=np.int64), (9, 1))
    assert mf.kernel_sum(same, same) != mf.kernel_sum(same, same, True) and mf.kernel_sum(same, same) - mf.kernel_sum(same, same, True) == 9 * 22.5 ** 3


def _d2_gram_fp32(a, b):
    """the planted defect: the Gram identity in fp32"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - np.float32(2) * (a @ b.T), np.float32(0)).astype(np.float64)


@pytest.mark.parametrize("name", ["offset100-48", "offset100-384"])
def test_the_criterion_rejects_an_fp32_gram_identity_on_offset_data(name):
    nq, nc, d, k, _, _ = mf.NORMAL_CASES[name]
    q, c = mf.normal_case(name)
    err = np.abs(_d2_gram_fp32(q, c) - mf.d2(q, c))
    assert (err > mf.gram_bound(q, c)).mean() > 0.9 and err.max() > 1e4 * mf.gram_bound(q, c).max()
    rad = mf.radii(c, k)
    assert np.abs(mf.radii(c, k, _d2_gram_fp32) - rad).max() > mf.gram_bound(c, c).max()
    assert not np.array_equal(mf.ball_counts(q, c, rad, _d2_gram_fp32)[0], mf.ball_counts(q, c, rad)[0])


# -------------------------------------------------------------------------------------------------------------------- margins
@pytest.mark.parametrize("name", sorted(mf.NORMAL_CASES))
def test_every_normal_gpu_case_is_far_from_a_flip(name):
    """the smallest relative margin min |d2 - rad2| / (|a|^2 + |b|^2) of every comparison the GPU tests make on this case - queries in
    the centres' balls at the reference's radii, and the whole of prdc with the sets in either role - exceeds 1000 x the kernel's error
    bound 4 (d + 2) 2^-53; the seeds in manifold_ref.NORMAL_CASES were chosen so"""
    nq, nc, d, k, _, _ = mf.NORMAL_CASES[name]
    q, c = mf.normal_case(name)
    got = min(mf.margin(q, c, mf.radii(c, k)), mf.case_margin(c, q, k), mf.case_margin(q, c, k))
    print(f"{name}: margin {got:.3e}, needed {mf.margin_needed(d):.3e}")
    assert got > mf.margin_needed(d)


# ---------------------------------------------------------------------------------------------------------- the caller's errors
def test_argument_errors_of_the_functions():
    x, y = torch.randn(20, 32), torch.randn(10, 32)
    for bad in (lambda: M.knn_radii(x, 0), lambda: M.knn_radii(x, 9), lambda: M.knn_radii(x, True), lambda: M.knn_radii(x, 2.0),
                lambda: M.knn_radii(x[:3], 3), lambda: M.knn_radii(x[:, :24], 1), lambda: M.knn_radii(x[0], 1), lambda: M.knn_radii(x[:0], 1),
                lambda: M.ball_counts(x, y[:, :16], torch.zeros(10, dtype=torch.float64)), lambda: M.ball_counts(x, y, torch.zeros(10)),
                lambda: M.ball_counts(x, y, torch.zeros(9, dtype=torch.float64)), lambda: M.ball_counts(x, y, None),
                lambda: M.poly_kernel_sum(x, y[:, :16]), lambda: M.prdc(x, y, 10), lambda: M.prdc(x, y[:4], 4), lambda: M.prdc(x, y, 0),
                lambda: M.kid(x, y[:1]), lambda: M.kid(x[:1], y), lambda: M.kid(x, torch.randn(10, 40))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: M.knn_radii(x.double(), 1), lambda: M.poly_kernel_sum(x, y.long()), lambda: M.kid(x.double(), y)):
        with pytest.raises(TypeError):
            bad()
    assert torch.equal(M.knn_radii(x.to(torch.bfloat16), 2), M.knn_radii(x.to(torch.bfloat16).float(), 2))  # widened, like the moments


class _Stub(torch.nn.Module):
    def __init__(self, gain=0.4):
        super().__init__()
        self.latent, self.calls = 8, 0
        self.w = torch.nn.Parameter(torch.randn(8, 3 * 8 * 8, generator=torch.Generator().manual_seed(2)) * gain)

    def forward(self, z):
        self.calls += 1
        return torch.tanh(z @ self.w).reshape(-1, 3, 8, 8)


class _Projection:
    def __init__(self):
        self.p = torch.randn(192, 16, generator=torch.Generator().manual_seed(3))
        self.calls = 0

    def __call__(self, x):
        self.calls += 1
        return x.reshape(x.shape[0], -1) @ self.p


def _dataset(N=90):
    from vit_gan_amd.data import DeviceDataset
    images = torch.randint(0, 256, (N, 3, 8, 8), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    return DeviceDataset(images, None, layout="nchw")


def test_evaluator_options_on_the_cpu_path(tmp_path):
    from vit_gan_amd.metrics import FrechetDistance
    ds, f, f0, G = _dataset(), _Projection(), _Projection(), _Stub()
    on = FrechetDistance(f, n_fake=50, batch=32, seed=7, manifold_k=3, kid=True, bank_real=25).fit_real(ds)
    off = FrechetDistance(f0, n_fake=50, batch=32, seed=7).fit_real(ds)
    assert f.calls == f0.calls == 3 and off.bank is None
    picks = torch.tensor([(j * 90) // 25 for j in range(25)])
    assert torch.equal(on.bank["feats"], f(ds.decode(picks))) and on.bank["k"] == 3
    assert np.abs(on.bank["rad2"].numpy() - mf.radii(on.bank["feats"].numpy(), 3)).max() <= 1e-9
    f.calls = f0.calls = 0
    d_on, calls = on(G), G.calls
    d_off = off(G)
    assert d_on == d_off and (f.calls, calls) == (f0.calls, G.calls - calls) == (2, 2)
    assert set(off.last) == {"distance", "mean_term", "trace_term", "n_real", "n_fake"} and all(on.last[k_] == off.last[k_] for k_ in off.last)
    real, fake = on.bank["feats"].numpy(), on.fake_feats.numpy()
    assert fake.shape == (50, 16) and mf.case_margin(real, fake, 3) > mf.margin_needed(16)
    want = mf.prdc(real, fake, 3)
    assert {k_: on.last[k_] for k_ in want} == want and abs(on.last["kid"] - mf.kid(real, fake)) <= mf.kid_bound(real, fake)
    assert (on.last["manifold_k"], on.last["n_real_bank"]) == (3, 25)
    # one option alone: the other half is NaN
    only_kid = FrechetDistance(_Projection(), n_fake=50, batch=32, seed=7, kid=True, bank_real=25).fit_real(ds)
    only_kid(G)
    assert only_kid.bank["rad2"] is None and only_kid.last["kid"] == on.last["kid"] and only_kid.last["precision"] != only_kid.last["precision"]
    # an iterable keeps the first n_keep images it sees
    it = FrechetDistance(_Projection(), n_fake=50, batch=32, manifold_k=2, bank_real=40)
    it.lut = ds.lut.clone()
    it.fit_real([ds.images[:30], (ds.images[30:], None)])
    assert torch.equal(it.bank["feats"], it.features(ds.decode(torch.arange(40)))) and it.real["n"] == 90
    # the file: unchanged keys with the options off, the bank under new ones, and the refusal names the option
    p_on, p_off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    on.save_real(p_on), off.save_real(p_off)
    with np.load(p_on) as a, np.load(p_off) as b:
        assert set(b.files) == {"mean", "cov", "n", "d", "tag", "lut"} and set(a.files) - set(b.files) == {"bank_feats", "bank_k", "bank_rad2", "bank_self_sum"}
        assert all(np.array_equal(a[k_], b[k_]) for k_ in b.files)
    again = FrechetDistance(f, n_fake=50, batch=32, seed=7, manifold_k=3, kid=True).load_real(p_on)
    assert again(G) == d_on and again.last == on.last
    assert FrechetDistance(f, n_fake=50, batch=32, seed=7).load_real(p_on)(G) == d_on
    for kw, name in (({"manifold_k": 3}, "manifold_k"), ({"kid": True}, "kid")):
        with pytest.raises(ValueError, match=name):
            FrechetDistance(f, n_fake=50, **kw).load_real(p_off)
        ev = FrechetDistance(f, n_fake=50, **kw)
        ev.real, ev.lut = off.real, off.lut  # statistics without a bank
        with pytest.raises(RuntimeError, match=name):
            ev(G)


def test_argument_errors_of_the_evaluator_and_the_trainer():
    from vit_gan_amd import training as T
    from vit_gan_amd.metrics import FrechetDistance
    f = _Projection()
    for kw in ({"manifold_k": 9}, {"manifold_k": -1}, {"manifold_k": True}, {"manifold_k": 2.0}, {"kid": 1}, {"kid": "yes"}, {"bank_real": 1},
               {"bank_real": 2.5}, {"manifold_k": 5, "n_fake": 5}):
        with pytest.raises(ValueError):
            FrechetDistance(f, **kw)
    with pytest.raises(ValueError, match="needs more than k"):  # fewer real rows kept than k + 1
        FrechetDistance(f, n_fake=50, manifold_k=5, bank_real=4).fit_real(_dataset(20))
    base = dict(steps_per_epoch=1, save_artifacts=False)
    with pytest.raises(ValueError, match='fid="random-vit"'):
        T.train_model({"epochs": 1}, manifold_k=3, **base)
    with pytest.raises(ValueError, match='fid="random-vit"'):
        T.train_model({"epochs": 1}, kid=True, fid_fn=lambda gan, epoch: 0.0, **base)
    for kw in ({"manifold_k": 9}, {"manifold_k": -1}, {"manifold_k": True}, {"kid": 1}):
        with pytest.raises(ValueError, match="manifold_k|kid"):
            T.train_model({"epochs": 1}, fid="random-vit", **kw, **base)
    with pytest.raises(ValueError, match="needs more than k"):
        T.train_model({"epochs": 1}, fid="random-vit", fid_samples=4, manifold_k=4, **base)
    if not torch.cuda.is_available():  # legal options pass the argument checks: the next stop is the device
        with pytest.raises(RuntimeError, match="MI355X"):
            T.train_model({"epochs": 1}, fid="random-vit", fid_samples=8, manifold_k=3, kid=True, **base)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "vitgan_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"^(int|long long) " + name + r"\(", header, re.M), name
        assert name in _lib._SIGNATURES and hasattr(lib, name), name
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9  # additive
    for name in ("knn_radii", "ball_counts", "poly_kernel_sum", "prdc", "kid"):
        assert name in M.__all__ and callable(getattr(M, name))


def test_host_side_rejections_need_no_device():
    lib = _lib.lib()
    p = C.c_void_p(4096)  # non-null dummy: never dereferenced on a rejected call
    knn = lambda X=p, ld=64, n=8, d=64, k=3, r=p, w=p: lib.vg_knn_radii(X, ld, n, d, k, r, w, None)  # noqa: E731
    ball = lambda Q=p, ldq=64, nq=8, Cn=p, ldc=64, nc=8, d=64, r=p, c=p, m=p, w=p: lib.vg_ball_counts(Q, ldq, nq, Cn, ldc, nc, d, r, c, m, w, None)  # noqa: E731
    ksum = lambda Q=p, ldq=64, nq=8, Cn=p, ldc=64, nc=8, d=64, o=p, w=p: lib.vg_poly_kernel_sum(Q, ldq, nq, Cn, ldc, nc, d, 1, o, w, None)  # noqa: E731
    assert knn(X=None) == knn(r=None) == knn(w=None) == knn(n=0) == -1
    assert ball(Q=None) == ball(Cn=None) == ball(r=None) == ball(c=None) == ball(m=None) == ball(w=None) == ball(nq=0) == ball(nc=0) == -1
    assert ksum(Q=None) == ksum(Cn=None) == ksum(o=None) == ksum(w=None) == ksum(nq=0) == ksum(nc=0) == -1
    for d in (0, 8, 24, 40, 2040, 2064, 4096, -16):
        assert knn(d=d, ld=8192) == ball(d=d, ldq=8192, ldc=8192) == ksum(d=d, ldq=8192, ldc=8192) == -2, d
    assert knn(ld=63) == ball(ldq=63) == ball(ldc=63) == ksum(ldq=63) == ksum(ldc=63) == -2
    assert knn(k=0) == knn(k=9) == knn(k=8) == knn(k=3, n=3) == -3 and knn(n=0, k=0) == -1 and knn(d=8, k=0) == -2  # the order of the checks
    # the workspace: no n x n term - linear in the rows at a fixed width, and bounded by (nq + nc) k splits doubles
    assert lib.vg_pair_ws_bytes(0, 8, 1) == lib.vg_pair_ws_bytes(8, 0, 1) == lib.vg_pair_ws_bytes(8, 8, 9) == -1
    for n in (100, 10000, 50000):
        for k in (0, 5, 8):
            got = lib.vg_pair_ws_bytes(n, n, k)
            assert 0 < got <= 8 * (2 * n) * max(k, 2) * 64 and got < 8 * n * n / 4, (n, k, got)
    assert lib.vg_pair_ws_bytes(10000, 50000, 0) < 64 << 20
