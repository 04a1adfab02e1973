"""The Frechet distance without a GPU: the three new exports and their host-side rejections, ``frechet_distance`` against closed
forms, torchmetrics' own form and scipy's sqrtm, ``FeatureMoments`` on CPU tensors against tests/metrics_ref.py (chunking, merge,
state_dict, a two-rank gloo all-reduce), ``FrechetDistance`` with a CPU feature function and a stub generator, and the trainer's new
arguments.  Every test here fails on the parent commit: no ``metrics`` module, no exports, no ``fid`` keyword.

(``train_model`` itself needs the GPU, so its ``fid=""`` log line, ``FID: nan``, is asserted in tests/test_metrics_gpu.py; here the
order of its argument checks is.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import engine_util as eu
import metrics_ref as mr
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib

SHAPES = [(16, 200), (64, 40), (128, 200), (384, 200), (384, 2000)]  # (d, n); n < d: rank-deficient covariances


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def test_exports_and_abi_version():
    lib = _lib.lib()
    for name in ("vg_vit_features", "vg_moments_update", "vg_moments_finish"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES, name
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9
    assert vit_gan_amd.FeatureMoments is not None and vit_gan_amd.FrechetDistance is not None and callable(vit_gan_amd.frechet_distance)


def test_host_side_rejections():
    lib = _lib.lib()
    p = C.c_void_p(4096)  # non-null dummy: never dereferenced on a rejected call
    upd = lambda f=p, ld=64, n=8, d=64, s=p, g=p: lib.vg_moments_update(f, ld, n, d, s, g, None)  # noqa: E731
    assert upd(f=None) == -1 and upd(s=None) == -1 and upd(g=None) == -1
    assert upd(n=0) == -1 and upd(n=-3) == -1
    for d in (0, 8, 24, 40, 2040, 2064, 4096, -16):
        assert upd(d=d, ld=8192) == -2, d
    assert upd(ld=63) == -2 and upd(d=2048, ld=2047) == -2
    fin = lambda s=p, g=p, n=8, d=64, m=p, c=p: lib.vg_moments_finish(s, g, n, d, m, c, None)  # noqa: E731
    assert fin(s=None) == -1 and fin(g=None) == -1 and fin(m=None) == -1 and fin(c=None) == -1
    assert fin(n=1) == -1 and fin(n=0) == -1
    for d in (0, 8, 24, 2064):
        assert fin(d=d) == -2, d
    dims = _lib.VgVitDims(3, 32, 4, 384, 6, 2, 4, 1)
    net = _lib.VgVitNet(dims, 16, 16, None, 0.0, 0, None, None, 0, 0)
    feat = lambda net_=C.byref(net), B=4, img=p, ws=p, lg=p, ft=p: lib.vg_vit_features(net_, B, img, 0, ws, lg, ft, None)  # noqa: E731
    assert feat(net_=None) == -1 and feat(img=None) == -1 and feat(ws=None) == -1 and feat(lg=None) == -1 and feat(ft=None) == -1
    assert feat(B=0) == -1
    bad = _lib.VgVitNet(_lib.VgVitDims(3, 32, 4, 100, 6, 2, 4, 1), 16, 16, None, 0.0, 0, None, None, 0, 0)
    assert feat(net_=C.byref(bad)) < 0  # dims the layout refuses, as vg_vit_forward
    assert feat(net_=C.byref(bad)) == lib.vg_vit_forward(C.byref(bad), 4, p, 0, p, p, None)


# ------------------------------------------------------------------------------------------------------------- frechet_distance
def _two_sets(d, n, seed):
    g = np.random.default_rng(seed)
    mix = g.standard_normal((d, d)) / np.sqrt(d)
    a = g.standard_normal((n, d)) @ mix + 0.3 * g.standard_normal(d)
    b = 1.3 * g.standard_normal((n, d)) @ mix.T + 0.1
    return a, b


def test_identical_moments_give_zero():
    from vit_gan_amd.metrics import frechet_distance
    for d, n in SHAPES:
        mu, cov = mr.two_pass(_two_sets(d, n, 1)[0])
        got = frechet_distance(mu, cov, mu, cov)
        assert 0.0 <= got <= 1e-6 * 2 * np.trace(cov), (d, n, got)


def test_commuting_covariances_closed_form():
    """diagonal covariances, and the same ones rotated by one orthogonal matrix: sum (sqrt a - sqrt b)^2 + |mu1 - mu2|^2"""
    from vit_gan_amd.metrics import frechet_distance
    for d, _ in SHAPES:
        g = np.random.default_rng(d)
        a, b = g.uniform(0.0, 4.0, d), g.uniform(0.0, 4.0, d)
        a[:3] = 0.0  # rank-deficient too
        mu1, mu2 = g.standard_normal(d), g.standard_normal(d)
        want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((mu1 - mu2) ** 2).sum()
        tol = 1e-6 * (a.sum() + b.sum())
        assert abs(frechet_distance(mu1, np.diag(a), mu2, np.diag(b)) - want) <= tol
        q, _ = np.linalg.qr(g.standard_normal((d, d)))
        got = frechet_distance(torch.from_numpy(mu1), torch.from_numpy(q @ np.diag(a) @ q.T), mu2, q @ np.diag(b) @ q.T)  # tensors too
        assert abs(got - want) <= tol, (d, got, want)


@pytest.mark.parametrize("d,n", SHAPES)
def test_formula_against_torchmetrics_form_and_sqrtm(d, n):
    from vit_gan_amd.metrics import frechet_distance, frechet_terms
    a, b = _two_sets(d, n, 100 + d + n)
    (mu1, c1), (mu2, c2) = mr.two_pass(a), mr.two_pass(b)
    got = frechet_distance(mu1, c1, mu2, c2)
    tol = 1e-6 * (np.trace(c1) + np.trace(c2))
    tm, sq = mr.frechet_torchmetrics(mu1, c1, mu2, c2), mr.frechet_sqrtm(mu1, c1, mu2, c2)
    print(f"d={d} n={n}: symmetric {got!r} torchmetrics {tm!r} sqrtm {sq!r}; |d|/scale {abs(got - tm) / tol * 1e-6:.2e} {abs(got - sq) / tol * 1e-6:.2e}")
    assert got > 100 * tol  # the two sets differ: the check below is not of two zeros
    assert abs(got - tm) <= tol, (got, tm)
    assert abs(got - sq) <= tol, (got, sq)
    mt, tt = frechet_terms(mu1, c1, mu2, c2)
    assert got == max(mt + tt, 0.0) and abs(mt - ((mu1 - mu2) ** 2).sum()) <= 1e-12 * max(mt, 1.0)
    assert abs(frechet_distance(mu2, c2, mu1, c1) - got) <= tol  # symmetric in its arguments
    with pytest.raises(ValueError):
        frechet_distance(mu1, c1, mu2[:-1], c2)


# ---------------------------------------------------------------------------------------------------------------- FeatureMoments
def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300)


def test_feature_moments_cpu_path_against_the_restatement():
    from vit_gan_amd.metrics import FeatureMoments
    d, n = 48, 333
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(5)) * 2 + 1
    one = FeatureMoments(d).update(x)
    s, g = mr.gram_update(np.zeros(d), np.zeros((d, d)), x.numpy())
    assert one.n == n and _close(one.sum, s) and _close(one.gram, g)
    mean, cov = mr.two_pass(x.numpy())
    assert _close(one.mean, mean) and _close(one.cov, cov, 1e-11)
    fm, fc = mr.finish(s, g, n)
    assert _close(one.mean, fm, 1e-15) and _close(one.cov, fc, 1e-13)
    # chunked = one update; bf16 / fp16 are widened first
    parts = FeatureMoments(d)
    for lo, hi in ((0, 1), (1, 100), (100, 101), (101, 333)):
        parts.update(x[lo:hi])
    assert parts.n == n and _close(parts.sum, s) and _close(parts.gram, g)
    for dt in (torch.bfloat16, torch.float16):
        h = FeatureMoments(d).update(x.to(dt))
        sh, gh = mr.gram_update(np.zeros(d), np.zeros((d, d)), x.to(dt).float().numpy())
        assert _close(h.sum, sh) and _close(h.gram, gh)
    # merge
    a, b = FeatureMoments(d).update(x[:120]), FeatureMoments(d).update(x[120:])
    a.merge(b)
    assert a.n == n and _close(a.sum, s) and _close(a.gram, g) and _close(a.cov, cov, 1e-11)
    # state_dict round trip, exact
    c = FeatureMoments(d)
    c.load_state_dict(one.state_dict())
    assert c.n == n and torch.equal(c.sum, one.sum) and torch.equal(c.gram, one.gram) and torch.equal(c.cov, one.cov)
    # the caller's errors
    for bad in (lambda: FeatureMoments(40), lambda: FeatureMoments(8), lambda: FeatureMoments(4096), lambda: one.update(x[:, :32]),
                lambda: one.update(x[0]), lambda: one.merge(FeatureMoments(64)), lambda: FeatureMoments(d).update(x[:1]).cov,
                lambda: FeatureMoments(64).load_state_dict(one.state_dict())):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        one.update(x.double())


def _worker(rank, world):
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.metrics import FeatureMoments

    torch.set_num_threads(2)
    d, n = 32, 101
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(9))
    lo, hi = (0, 37) if rank == 0 else (37, n)  # uneven shards
    m = FeatureMoments(d).update(x[lo:hi]).all_reduce()
    whole = FeatureMoments(d).update(x)
    err = max(float((m.sum - whole.sum).abs().max()), float((m.gram - whole.gram).abs().max()) / float(whole.gram.abs().max()))
    if rank == 0:
        return m.n, err


@pytest.mark.timeout(300)
def test_two_rank_gloo_all_reduce_of_the_moments():
    val = eu.run_ranks(_worker, 2, 240)[0]
    assert val[0] == 101 and val[1] <= 1e-13, val


# --------------------------------------------------------------------------------------------------------------- FrechetDistance
class _StubGenerator(torch.nn.Module):
    """latent -> image by one fixed linear map; records the latents (and labels) it is given"""

    def __init__(self, latent=8, n_classes=0, gain=1.5):
        super().__init__()
        self.latent, self.n_classes = latent, n_classes
        self.w = torch.nn.Parameter(torch.randn(latent, 3 * 8 * 8, generator=torch.Generator().manual_seed(2)) * gain)
        self.seen, self.modes = [], []

    def forward(self, z, labels=None):
        self.seen.append((z.clone(), None if labels is None else labels.clone()))
        self.modes.append((self.training, torch.is_grad_enabled()))
        x = torch.tanh(z @ self.w).reshape(-1, 3, 8, 8) * 1.2  # beyond [-1, 1]: the clamp matters
        return x + (0.0 if labels is None else 0.05 * labels.reshape(-1, 1, 1, 1).float())


class _Counting:
    """images [n, 3, 8, 8] -> [n, 16]: a fixed projection; keeps what it was shown"""

    def __init__(self):
        self.p = torch.randn(192, 16, generator=torch.Generator().manual_seed(3))
        self.batches = []

    def __call__(self, x):
        self.batches.append(x.clone())
        return x.reshape(x.shape[0], -1) @ self.p


def _dataset(N=50, labels=False):
    from vit_gan_amd.data import DeviceDataset
    g = torch.Generator().manual_seed(11)
    images = torch.randint(0, 256, (N, 3, 8, 8), generator=g, dtype=torch.uint8)
    return DeviceDataset(images, torch.arange(N) % 3 if labels else None, layout="nchw", mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.3))


def test_fit_real_visits_every_image_in_storage_order():
    from vit_gan_amd.metrics import FrechetDistance
    ds, f = _dataset(50), _Counting()
    ev = FrechetDistance(f, n_fake=40, batch=16).fit_real(ds)
    assert [b.shape[0] for b in f.batches] == [16, 16, 16, 2]  # the tail of 2 that steps_per_epoch(16) drops is there
    seen = torch.cat(f.batches)
    assert torch.equal(seen, ds.decode(torch.arange(50)))  # storage order, unflipped, through the table
    assert np.array_equal(seen.numpy(), mr.table((0.4, 0.5, 0.6), (0.2, 0.25, 0.3))[np.arange(3).reshape(1, 3, 1, 1), ds.images.numpy()])
    mean, cov = mr.two_pass((seen.reshape(50, -1) @ f.p).numpy())
    assert ev.real["n"] == 50 and ev.real["d"] == 16 and _close(ev.real["mean"], mean) and _close(ev.real["cov"], cov, 1e-10)
    # an iterable of batches: uint8 through the table, pairs accepted
    f2 = _Counting()
    ev2 = FrechetDistance(f2, n_fake=40, batch=16)
    ev2.lut = ds.lut.clone()
    ev2.fit_real([(ds.images[:30], None), (ds.images[30:], None)])
    assert torch.equal(torch.cat(f2.batches), seen) and _close(ev2.real["cov"], cov, 1e-10)
    with pytest.raises(ValueError):
        FrechetDistance(_Counting()).fit_real([ds.images[:1]])


@pytest.mark.parametrize("K", [0, 3])
def test_same_latents_every_call_eval_mode_and_the_quantisation_path(K):
    from vit_gan_amd.metrics import FrechetDistance, frechet_distance
    ds, f, G = _dataset(50), _Counting(), _StubGenerator(n_classes=K)
    ev = FrechetDistance(f, n_fake=40, batch=16, seed=7).fit_real(ds)
    with pytest.raises(RuntimeError):
        FrechetDistance(_Counting())(G)  # no real statistics
    f.batches.clear()
    gan = torch.nn.Module()
    gan.generator = G.train()
    state = torch.get_rng_state()
    first = ev(gan, 0)
    shown = torch.cat(f.batches)
    again = ev(gan, 1)
    assert torch.equal(torch.get_rng_state(), state), "the evaluation drew from the global generator"
    assert first == again and np.isfinite(first) and first > 0
    assert G.training and all(m == (False, False) for m in G.modes)  # eval mode under no_grad, and the mode restored
    assert [z.shape[0] for z, _ in G.seen] == [16, 16, 8] * 2  # a smaller last batch
    z1, z2 = torch.cat([z for z, _ in G.seen[:3]]), torch.cat([z for z, _ in G.seen[3:]])
    assert torch.equal(z1, z2) and float(z1.std()) > 0.5
    if K:
        assert torch.equal(torch.cat([l for _, l in G.seen[:3]]), (torch.arange(40) % K).to(torch.int32))
    else:
        assert all(l is None for _, l in G.seen)
    assert not torch.equal(torch.cat([z for z, _ in G.seen[:3]]), next(FrechetDistance(f, n_fake=40, batch=40, seed=8).latents(G, "cpu"))[0])
    # the quantisation path, bit for bit: clamp, the reference's truncation, the dataset's own table
    with torch.no_grad():
        raw = torch.cat([G.eval()(z, l) for z, l in G.seen[:3]]).numpy()
    want = mr.quantize(raw, mr.table((0.4, 0.5, 0.6), (0.2, 0.25, 0.3)))
    assert float(np.abs(raw).max()) > 1.0 and np.array_equal(shown.numpy(), want)
    # .last, and the distance of its own moments
    mean, cov = mr.two_pass((torch.from_numpy(want).reshape(40, -1) @ f.p).numpy())
    fm, fc = ev.fake.moments()
    assert _close(fm, mean) and _close(fc, cov, 1e-10)
    assert ev.last["distance"] == first == frechet_distance(ev.real["mean"], ev.real["cov"], fm, fc)
    assert (ev.last["n_real"], ev.last["n_fake"]) == (50, 40) and ev.last["distance"] == max(ev.last["mean_term"] + ev.last["trace_term"], 0.0)
    # quantize=False hands the generator's own values on
    f3 = _Counting()
    ev3 = FrechetDistance(f3, n_fake=40, batch=16, seed=7, quantize=False).fit_real(ds)
    f3.batches.clear()
    ev3(G)
    assert np.array_equal(torch.cat(f3.batches).numpy(), raw)


def test_real_statistics_round_trip_and_the_tag(tmp_path):
    from vit_gan_amd.metrics import FrechetDistance
    ds, f = _dataset(50), _Counting()
    ev = FrechetDistance(f, n_fake=40, batch=16, tag="projection-a").fit_real(ds)
    path = str(tmp_path / "real_stats.npz")
    ev.save_real(path)
    with np.load(path) as z:
        assert set(z.files) >= {"mean", "cov", "n", "d", "tag"} and int(z["n"]) == 50 and int(z["d"]) == 16 and str(z["tag"]) == "projection-a"
    other = FrechetDistance(f, n_fake=40, batch=16, tag="projection-a").load_real(path)
    assert np.array_equal(other.real["mean"], ev.real["mean"]) and np.array_equal(other.real["cov"], ev.real["cov"]) and other.real["n"] == 50
    assert torch.equal(other.lut, ev.lut)
    G = _StubGenerator()
    assert other(G) == ev(G)
    with pytest.raises(ValueError, match="projection-b"):
        FrechetDistance(f, tag="projection-b").load_real(path)
    with pytest.raises(RuntimeError):
        FrechetDistance(f).save_real(path)


def test_random_vit_is_fixed_by_its_seed_and_leaves_the_global_rng_alone():
    from vit_gan_amd.config import Config
    from vit_gan_amd.metrics import FrechetDistance
    dims = dict(n_channels=3, embed_dim=128, n_layers=1, n_attention_heads=4, forward_mul=2, image_size=32, patch_size=4)
    state = torch.get_rng_state()
    a, b, c = FrechetDistance.random_vit(dims, seed=0), FrechetDistance.random_vit(dims, seed=0), FrechetDistance.random_vit(dims, seed=1)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(a.features.flat, b.features.flat) and a.tag == b.tag and not torch.equal(a.features.flat, c.features.flat)
    assert a.tag != c.tag and "seed=0" in a.tag and "embed_dim=128" in a.tag and a.features.d == 128
    assert not a.features.flat.requires_grad
    cfg = FrechetDistance.random_vit(Config(embeddings_dimension=384, transformer_blocks_count=1), seed=0, n_fake=64)
    assert cfg.features.d == 384 and cfg.n_fake == 64
    with pytest.raises(RuntimeError):
        a.features(torch.zeros(2, 3, 32, 32))  # no CPU fallback for the ViT
    for bad in (lambda: FrechetDistance(3), lambda: FrechetDistance.random_vit({"embed_dim": 128})):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: FrechetDistance(_Counting(), n_fake=1), lambda: FrechetDistance(_Counting(), batch=0)):
        with pytest.raises(ValueError):
            bad()


def test_a_frozen_copy_does_not_follow_its_source():
    from vit_gan_amd.config import Config
    from vit_gan_amd.metrics import FrechetDistance
    from vit_gan_amd.modules import ViTDiscriminator
    D = ViTDiscriminator(Config(embeddings_dimension=128, attention_heads_count=4, transformer_blocks_count=1, classes_count=1))
    ev = FrechetDistance(D, n_fake=8)
    before = ev.features.flat.clone()
    with torch.no_grad():
        for p in D.parameters():
            p.add_(1.0)
    assert torch.equal(ev.features.flat, before) and not torch.equal(D.vit._flat.flat, before)
    assert ev.tag.startswith("vit:") and ev.tag != FrechetDistance(D, n_fake=8).tag  # the tag follows the parameters


# ---------------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_argument_checks_come_before_the_device_check():
    from vit_gan_amd import training as T
    with pytest.raises(ValueError, match="fid must be"):
        T.train_model({"epochs": 1}, steps_per_epoch=1, save_artifacts=False, fid="inception")
    with pytest.raises(ValueError, match="either fid or fid_fn"):
        T.train_model({"epochs": 1}, steps_per_epoch=1, save_artifacts=False, fid="random-vit", fid_fn=lambda gan, epoch: 0.0)
    with pytest.raises(ValueError, match="fid_samples"):
        T.train_model({"epochs": 1}, steps_per_epoch=1, save_artifacts=False, fid="random-vit", fid_samples=1)
    with pytest.raises(ValueError, match="pass fid_fn"):  # as before: the plateau rule without a score
        T.train_model({"epochs": 1}, steps_per_epoch=1, save_artifacts=False, lr_plateau=(0.5, 1))
    assert T.parse_lr_plateau((0.5, 1), "random-vit") is not None
    if not torch.cuda.is_available():  # lr_plateau with fid alone passes the argument checks: the next stop is the device
        with pytest.raises(RuntimeError, match="MI355X"):
            T.train_model({"epochs": 1}, steps_per_epoch=1, save_artifacts=False, fid="random-vit", fid_samples=8, lr_plateau=(0.5, 1))
