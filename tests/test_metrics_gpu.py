"""The Frechet distance on the GPU: vg_moments_update held to int64 arithmetic on integer features at every (d, n, ld) - every value
exactly representable, so a mis-indexed lane, a dropped k-group or a tail row shows as a wrong integer - and to the fp64 dot-product
bound on normal ones; vg_moments_finish against two-pass fp64 within the one-pass formula's cancellation bound; vg_vit_features
against vg_vit_forward (logits bit-equal, the workspace good for the backward) and the fp64 LayerNorm of the workspace's xtop; the
evaluator end to end against features recomputed through ``VisionTransformer.features`` and tests/metrics_ref.py; the trainer.
Every test here fails on the parent commit: no exports, no ``metrics`` module, no ``features`` method, no ``fid`` keyword."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import gpu_util as u
import metrics_ref as mr

pytestmark = pytest.mark.gpu

GUARD = -7.25
PAD = 64  # guard words in front of, between and behind the two outputs


def _outputs(d, sum0=None, gram0=None):
    """guard | sum [d] | guard | gram [d, d] | guard in one fp64 buffer -> (buf, sum view, gram view)"""
    buf = torch.full((3 * PAD + d + d * d,), GUARD, dtype=torch.float64, device="cuda")
    s, g = buf[PAD:PAD + d], buf[2 * PAD + d:2 * PAD + d + d * d].view(d, d)
    s.copy_(torch.zeros(d, dtype=torch.float64) if sum0 is None else sum0)
    g.copy_(torch.zeros(d, d, dtype=torch.float64) if gram0 is None else gram0)
    return buf, s, g


def _guards_intact(buf, d):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[PAD:PAD + d] = False
    keep[2 * PAD + d:2 * PAD + d + d * d] = False
    return bool((buf[keep] == GUARD).all())


def _update(x, d, buf_s_g, n=None, ld=None):
    buf, s, g = buf_s_g
    u.call("vg_moments_update", u.ptr(x), x.stride(0) if ld is None else ld, x.shape[0] if n is None else n, d, u.ptr(s), u.ptr(g), u.stream())
    u.sync()
    assert _guards_intact(buf, d), "a guard word around sum / gram was written"
    return s.cpu().numpy().copy(), g.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------- vg_moments_update: exactness
NS = (1, 3, 4, 5, 63, 64, 65, 256, 1000)


@pytest.mark.parametrize("d", [16, 48, 384, 2048])
def test_moments_update_is_exact_on_integers(d):
    g = torch.Generator().manual_seed(d)
    whole = torch.randint(-8, 9, (max(NS), d), generator=g).float()
    seen = 0
    for n in NS:
        xi = whole[:n].numpy().astype(np.int64)
        # |sum| <= 8 n and |gram| <= 64 n, far inside 2^53: the fp64 BLAS product of these integers is the int64 one
        want_s, want_g = xi.sum(0), (xi.astype(np.float64).T @ xi.astype(np.float64)).astype(np.int64)
        if d <= 48:
            assert np.array_equal(want_g, xi.T @ xi)
        for ld in (d, d + 16):
            x = torch.full((n, ld), 1e30, dtype=torch.float32)  # the padding columns would wreck any sum they entered
            x[:, :d] = whole[:n]
            xd = x.cuda()[:, :d]
            assert xd.stride(0) == ld
            s, gm = _update(xd, d, _outputs(d))
            assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(s, want_s.astype(np.float64)), (d, n, ld, "sum")
            bad = np.argwhere(gm != want_g.astype(np.float64))
            assert bad.size == 0, (d, n, ld, "gram", bad[:4].tolist(), len(bad))
            assert np.array_equal(gm, gm.T), (d, n, ld, "gram is not symmetric bit for bit")
            seen += 1
            if ld == d and n in (5, 65, 1000):
                # two runs are bit-equal, and two updates (split off the k-group grid) equal one update of the concatenation
                s2, g2 = _update(xd, d, _outputs(d))
                assert np.array_equal(s2.view(np.int64), s.view(np.int64)) and np.array_equal(g2.view(np.int64), gm.view(np.int64))
                cut = n // 2 + 1
                out = _outputs(d)
                _update(xd[:cut], d, out)
                s3, g3 = _update(xd[cut:], d, out)
                assert np.array_equal(s3, s) and np.array_equal(g3, gm), (d, n, "two updates")
    assert seen == 2 * len(NS)


def test_moments_update_accumulates_onto_what_it_is_given():
    d, n = 48, 37
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-8, 9, (n, d), generator=g).float()
    a = torch.randint(-100, 100, (d, d), generator=g).double()
    s0, g0 = torch.randint(-100, 100, (d,), generator=g).double(), a + a.t()
    s, gm = _update(x.cuda(), d, _outputs(d, s0, g0))
    xi = x.numpy().astype(np.int64)
    assert np.array_equal(s, (s0.numpy() + xi.sum(0))) and np.array_equal(gm, g0.numpy() + xi.T @ xi)


# --------------------------------------------------------------------------------------------------- vg_moments_update: rounding
def test_moments_update_rounding_is_an_fp64_dot_product():
    """standard-normal fp32 features, n = 1000, d = 384, against numpy fp64 of the same fp32 values: elementwise
    |d gram_ij| <= n 2^-53 sum_k |x_ki x_kj| (gamma_n of an fp64 dot product of n terms, any order), and the same with |x| for sum"""
    n, d = 1000, 384
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(2))
    s, gm = _update(x.cuda(), d, _outputs(d))
    x64 = x.numpy().astype(np.float64)
    want_s, want_g = mr.gram_update(np.zeros(d), np.zeros((d, d)), x64)
    ax = np.abs(x64)
    lim_s, lim_g = n * 2.0 ** -53 * ax.sum(0), n * 2.0 ** -53 * (ax.T @ ax)
    es, eg = np.abs(s - want_s), np.abs(gm - want_g)
    print(f"sum: worst err/limit {float((es / lim_s).max()):.3e}; gram: worst err/limit {float((eg / lim_g).max()):.3e}")
    assert (es <= lim_s).all() and (eg <= lim_g).all()
    assert np.array_equal(gm, gm.T)
    assert float(eg.max()) < 1e-9 and float(np.abs(want_g).max()) > 500  # not fp32 products: those would be off by 1e-4 here


# ------------------------------------------------------------------------------------------------------------ vg_moments_finish
def _finish(s, gm, n, d):
    buf = torch.full((3 * PAD + d + d * d,), GUARD, dtype=torch.float64, device="cuda")
    mean, cov = buf[PAD:PAD + d], buf[2 * PAD + d:2 * PAD + d + d * d].view(d, d)
    sd, gd = torch.from_numpy(s).cuda(), torch.from_numpy(gm).cuda()
    u.call("vg_moments_finish", u.ptr(sd), u.ptr(gd), n, d, u.ptr(mean), u.ptr(cov), u.stream())
    u.sync()
    assert _guards_intact(buf, d), "a guard word around mean / cov was written"
    return mean.cpu().numpy().copy(), cov.cpu().numpy().copy()


@pytest.mark.parametrize("n,d", [(1000, 384), (77, 48), (2, 16)])
def test_moments_finish_against_two_pass(n, d):
    """features with a large mean (100 +- 0.01): the one-pass formula cancels n mean^2 against the Gram matrix, so
    |d cov_ij| <= 8 n 2^-53 max_k sum_i x_ik^2 / (n - 1) against two-pass fp64"""
    x = (100.0 + 0.01 * torch.randn(n, d, generator=torch.Generator().manual_seed(n + d))).float()
    s, gm = _update(x.cuda(), d, _outputs(d))
    mean, cov = _finish(s, gm, n, d)
    x64 = x.numpy().astype(np.float64)
    want_mean, want_cov = mr.two_pass(x64)
    lim = 8 * n * 2.0 ** -53 * float((x64 ** 2).sum(0).max()) / (n - 1)
    err = float(np.abs(cov - want_cov).max())
    print(f"n={n} d={d}: cov err {err:.3e}, limit {lim:.3e}, |cov| {float(np.abs(want_cov).max()):.3e}")
    assert err <= lim
    assert float(np.abs(mean - want_mean).max()) <= 4 * 2.0 ** -53 * 100.01 * 2
    assert np.array_equal(cov, cov.T)
    fm, fc = mr.finish(s, gm, n)  # the same formula in numpy, from the same sums: a rounding or two apart
    assert float(np.abs(cov - fc).max()) <= lim and np.array_equal(mean, fm)


def test_moments_finish_against_numpy_cov_on_benign_data():
    n, d = 500, 64
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(3)) * torch.linspace(0.5, 2.0, d)
    s, gm = _update(x.cuda(), d, _outputs(d))
    mean, cov = _finish(s, gm, n, d)
    want = np.cov(x.numpy().astype(np.float64), rowvar=False)
    assert float(np.abs(cov - want).max()) <= 1e-12 * float(np.abs(want).max())
    assert float(np.abs(mean - x.numpy().astype(np.float64).mean(0)).max()) <= 1e-14


def test_feature_moments_on_the_device():
    """the Python accumulator on cuda tensors: chunked = one update for integers, strided rows, bf16 widened, merge, mean / cov"""
    from vit_gan_amd.metrics import FeatureMoments
    n, d = 301, 48
    x = torch.randint(-8, 9, (n, d), generator=torch.Generator().manual_seed(4)).float()
    xi = x.numpy().astype(np.int64)
    one = FeatureMoments(d, "cuda").update(x.cuda())
    parts = FeatureMoments(d, "cuda")
    wide = torch.zeros(n, 2 * d).cuda()
    wide[:, :d] = x.cuda()
    for lo, hi in ((0, 1), (1, 130), (130, 301)):
        parts.update(wide[lo:hi, :d])  # a strided view: no copy
    for m in (one, parts):
        assert m.n == n and np.array_equal(m.sum.cpu().numpy(), xi.sum(0)) and np.array_equal(m.gram.cpu().numpy(), xi.T @ xi)
    assert np.array_equal(FeatureMoments(d, "cuda").update(x.cuda().to(torch.bfloat16)).gram.cpu().numpy(), xi.T @ xi)
    a, b = FeatureMoments(d, "cuda").update(x[:100].cuda()), FeatureMoments(d, "cpu").update(x[100:])
    assert torch.equal(a.merge(b).gram, one.gram) and a.n == n
    mean, cov = mr.two_pass(x.numpy())
    gm, gc = one.moments()
    assert np.abs(gm - mean).max() <= 1e-14 and np.abs(gc - cov).max() <= 1e-12 * np.abs(cov).max()
    with pytest.raises(ValueError):
        one.update(x)  # a CPU tensor into a device accumulator


# -------------------------------------------------------------------------------------------------------------- vg_vit_features
def _vit(B, seed=7):
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat
    d = vo.VitDims(layers=2, classes=1)  # the suite's small geometry: 65 tokens, E = 384, two blocks
    st = {k: (v * 2.5 if v.dim() > 1 else v) for k, v in vo.init_vit_state(d, seed=seed).items()}
    g = torch.Generator().manual_seed(seed)
    st["vit.norm.weight"] = 1.0 + 0.3 * torch.randn(d.embed, generator=g)  # a final LayerNorm that is not the identity's
    st["vit.norm.bias"] = 0.3 * torch.randn(d.embed, generator=g)
    gd = _lib.VgVitDims(d.channels, d.image, d.patch, d.embed, d.heads, d.layers, d.mlp_ratio, d.classes)
    lay, slots = flat.vit_layout(gd), flat.vit_slots(gd)
    P = flat.pack(slots, lay.total, {k: v.numpy() for k, v in st.items()}, device="cuda")
    x = torch.rand(B, 3, d.image, d.image, generator=torch.Generator().manual_seed(3)) * 2 - 1
    return _lib, d, st, gd, P, P.to(torch.bfloat16), x


def _forward(_lib, gd, P, Pb, x, dense, features):
    B = x.shape[0]
    G = torch.zeros_like(P)
    net = _lib.VgVitNet(gd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), 0.0, 0, None, None, 0, dense)
    ws = torch.zeros(_lib.lib().vg_vit_ws_bytes(C.byref(gd), B), dtype=torch.uint8, device="cuda")
    logits = torch.full((B + 2, 1), GUARD, device="cuda")
    feats = torch.full((B + 2, gd.E), GUARD, device="cuda") if features else None
    xd = x.cuda()
    if features:
        u.call("vg_vit_features", C.byref(net), B, u.ptr(xd), int(x.dtype == torch.bfloat16), u.ptr(ws), u.ptr(logits[1:]), u.ptr(feats[1:]), u.stream())
    else:
        u.call("vg_vit_forward", C.byref(net), B, u.ptr(xd), int(x.dtype == torch.bfloat16), u.ptr(ws), u.ptr(logits[1:]), u.stream())
    dl = (torch.randn(B, 1, generator=torch.Generator().manual_seed(4)) / B).cuda()
    dimg = torch.empty(B, 3, gd.IH, gd.IH, dtype=torch.bfloat16, device="cuda")
    u.sync()
    kept = ws.clone()
    u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(dl), u.ptr(dimg), 1, u.stream())
    u.sync()
    for t in (logits, feats):
        assert t is None or (bool((t[0] == GUARD).all()) and bool((t[B + 1] == GUARD).all())), "a guard row was written"
    return logits[1:B + 1].cpu(), None if feats is None else feats[1:B + 1].cpu(), G.cpu(), dimg.float().cpu(), kept, net


@pytest.mark.parametrize("bf16_in", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_vit_features(B, bf16_in):
    import norm_ref as nr
    from second_order_ref import assert_elementwise
    _lib, d, st, gd, P, Pb, x = _vit(B)
    if bf16_in:
        x = x.to(torch.bfloat16)
    feats = {}
    for dense in (0, 1):
        lf, _, Gf, df, _, _ = _forward(_lib, gd, P, Pb, x, dense, False)
        lg, ft, Gg, dg, ws, _ = _forward(_lib, gd, P, Pb, x, dense, True)
        assert torch.equal(lg.view(torch.int32), lf.view(torch.int32)), f"dense_top {dense}: the logits differ from vg_vit_forward's"
        assert torch.equal(Gg, Gf) and torch.equal(dg, df), f"dense_top {dense}: the backward after vg_vit_features differs"
        assert torch.isfinite(ft).all() and torch.equal(ft.to(torch.bfloat16).float(), ft), "features are widened bf16 values"
        assert float(ft.std()) > 0.3
        feats[dense] = ft
        if dense == 0:  # the pruned tail keeps X[L] on the CLS rows: the features are the final LayerNorm of exactly those rows
            wm = _lib.VgVitWsMap()
            u.call("vg_vit_ws_map", C.byref(gd), B, C.byref(wm))
            xtop = ws[wm.xtop:wm.xtop + B * gd.E * 2].view(torch.bfloat16).view(B, gd.E).float().cpu()
            ref = nr.ln_fwd(xtop.double(), st["vit.norm.weight"].double(), st["vit.norm.bias"].double())
            assert_elementwise(ft, ref["y"], ref["mag_y"], nr.kappa_fwd(gd.E), f"B={B} features vs LayerNorm(xtop)")
    # the tolerance of test_fullsize_gpu.test_pruned_top_block_equals_the_dense_one on the logits, here on the features
    assert float((feats[0] - feats[1]).abs().max()) <= 2.0 ** -6 * float(feats[1].abs().max()) + 1e-4


def test_module_features_match_the_frozen_copy():
    from vit_gan_amd.config import Config
    from vit_gan_amd.metrics import FrozenViTFeatures
    from vit_gan_amd.modules import ViTDiscriminator
    D = ViTDiscriminator(Config(embeddings_dimension=128, attention_heads_count=4, transformer_blocks_count=2, classes_count=1)).cuda().eval()
    x = torch.rand(5, 3, 32, 32, device="cuda") * 2 - 1
    frozen = FrozenViTFeatures(D)
    logits, feats = D.vit.features(x)
    with torch.no_grad():
        assert torch.equal(logits, D(x))
    assert torch.equal(frozen(x), feats) and feats.shape == (5, 128)
    with torch.no_grad():
        for p in D.parameters():
            p.mul_(1.5)
    assert torch.equal(frozen(x), feats) and not torch.equal(D.vit.features(x)[1], feats)  # frozen at construction


# ------------------------------------------------------------------------------------------------------------------- end to end
DIMS = dict(n_channels=3, embed_dim=128, n_layers=2, n_attention_heads=4, forward_mul=2, image_size=32, patch_size=4)


def _dataset(N=200, K=0, seed=9):
    from vit_gan_amd.data import DeviceDataset
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N, 3, 32, 32), generator=g, dtype=torch.uint8)
    return DeviceDataset(images, torch.arange(N) % K if K else None, device="cuda")


def _random_vit(seed):
    """FrechetDistance.random_vit's network, rebuilt here as a live module"""
    from vit_gan_amd.modules import VisionTransformer
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return VisionTransformer(n_classes=1, dropout=0.0, **DIMS).cuda().eval()


@pytest.fixture(scope="module")
def fitted():
    """one evaluator with the real statistics of the 200-image set, and those statistics recomputed (shared, never modified)"""
    from vit_gan_amd.metrics import FrechetDistance
    ds = _dataset()
    ev = FrechetDistance.random_vit(DIMS, seed=5, latent_seed=3, n_fake=96, batch=32).fit_real(ds)
    vit = _random_vit(5)
    feats = torch.cat([vit.features(ds.decode(torch.arange(lo, min(lo + 64, 200))))[1] for lo in range(0, 200, 64)])
    return ds, ev, vit, mr.two_pass(feats.double().cpu().numpy())


def _fro_close(got, want, rel=1e-11):
    err, scale = float(np.linalg.norm(got - want)), float(np.linalg.norm(want))
    print(f"|d| {err:.3e} of |.| {scale:.3e}: {err / scale:.2e}")
    return err <= rel * scale


@pytest.mark.parametrize("K", [0, 3])
def test_evaluator_against_recomputed_features(fitted, K):
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.metrics import frechet_distance
    ds, ev, vit, (rmean, rcov) = fitted
    assert ev.real["n"] == 200 and _fro_close(ev.real["mean"], rmean) and _fro_close(ev.real["cov"], rcov)
    torch.manual_seed(K)
    G = SirenGenerator(embed=128, layers=1, siren_hidden=256, dropout=0.0, n_classes=K).cuda().train()
    first = ev(G)
    last = dict(ev.last)
    fmean, fcov = ev.fake.moments()
    # the same pass restated: latents of the seed batch by batch, labels i % K, eval mode, the reference's quantisation, the features
    gen = torch.Generator(device="cuda").manual_seed(3)
    tab = mr.table([0.5], [0.5])
    assert np.array_equal(tab, ds.lut[:1].cpu().numpy())
    feats = []
    G.eval()
    with torch.no_grad():
        for lo in (0, 32, 64):
            z = torch.randn(32, G.latent, device="cuda", generator=gen)
            x = G(z, (torch.arange(lo, lo + 32, device="cuda") % K).to(torch.int32)) if K else G(z)
            feats.append(vit.features(torch.from_numpy(mr.quantize(x.float().cpu().numpy(), tab)).cuda())[1])
    G.train()
    wmean, wcov = mr.two_pass(torch.cat(feats).double().cpu().numpy())
    assert _fro_close(fmean, wmean) and _fro_close(fcov, wcov)
    assert first == last["distance"] == frechet_distance(ev.real["mean"], ev.real["cov"], fmean, fcov)
    assert (last["n_real"], last["n_fake"]) == (200, 96)
    scale = 1e-6 * (np.trace(ev.real["cov"]) + np.trace(fcov))
    print(f"K={K}: distance {first!r} (mean term {last['mean_term']!r}, trace term {last['trace_term']!r}); 1e-6 scale {scale:.3e}")
    assert np.isfinite(first) and first >= 100 * scale
    assert ev(G) == first and G.training  # an unchanged generator scores the same, bit for bit


class _Replay(torch.nn.Module):
    """a "generator" that hands back the dataset's own images in storage order, as the centres of their uint8 bins"""

    def __init__(self, ds):
        super().__init__()
        self.latent, self.ds, self.at = 4, ds, 0
        self.anchor = torch.nn.Parameter(torch.zeros(1, device="cuda"))

    def forward(self, z):
        idx = torch.arange(self.at, self.at + z.shape[0]) % self.ds.N
        self.at += z.shape[0]
        x = self.ds.images[idx.cuda()]
        return (x.float() + 0.5) / 255 * 2 - 1


def test_replaying_the_real_set_scores_zero(fitted):
    from vit_gan_amd.metrics import FrechetDistance
    ds, ev, _, _ = fitted
    same = FrechetDistance(ev.features, n_fake=200, batch=32)
    same.real, same.lut = ev.real, ev.lut
    got = same(_Replay(ds))
    scale = 1e-6 * (np.trace(ev.real["cov"]) + np.trace(same.fake.moments()[1]))
    print(f"replay: distance {got!r}, bound {scale:.3e}")
    assert 0.0 <= got <= scale


# ----------------------------------------------------------------------------------------------------------------------- trainer
CFG = {"epochs": 2, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}


def test_trainer_scores_its_epochs(tmp_path):
    from vit_gan_amd.metrics import FrechetDistance
    from vit_gan_amd.training import train_model
    ds = _dataset(N=20, seed=10)
    out = train_model(CFG, dataset=ds, output_base=str(tmp_path), fid="random-vit", fid_samples=64, ema_decay=0.999, lr_plateau=(0.5, 1))
    d, ev = out["dirs"], out["fid"]
    log = open(os.path.join(d.save, "training.log")).read()
    assert "Exception" not in log
    fids = [float(v) for v in re.findall(r"Epoch \[[01]/2\] \| Disc Loss: \S+, Gen Loss: \S+ \| FID: (\S+)", log)]
    assert len(fids) == 2 and all(np.isfinite(fids)) and all(f > 0 for f in fids), log
    head = re.search(r"Frechet distance: feature net (random-vit:seed=0:\S+), latent seed 0, n_real 20, n_fake 64", log)
    assert head and "embed_dim=128" in head.group(1) and head.group(1) == ev.tag
    assert "Learning-rate schedule: constant" in log and "on a plateau of the FID" in log  # lr_plateau took the built hook
    # the last epoch's score is the evaluator's on the averaged generator it returns
    assert isinstance(ev, FrechetDistance) and ev.last["n_real"] == 20 and ev.last["n_fake"] == 64
    last = ev.last["distance"]
    assert abs(last - fids[1]) <= 5.1e-5
    holder = torch.nn.Module()
    holder.generator = out["generator_ema"]
    assert ev(holder, 2) == last
    best = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d.checkpoints, "best_model_epoch_*_fid_*.pth")))
    assert best and f"best_model_epoch_0_fid_{int(fids[0])}.pth" in best, best
    stats = os.path.join(d.save, "real_stats.npz")
    with np.load(stats) as z:
        assert int(z["n"]) == 20 and int(z["d"]) == 128 and str(z["tag"]) == ev.tag
        assert np.array_equal(z["mean"], ev.real["mean"]) and np.array_equal(z["cov"], ev.real["cov"])
    again = FrechetDistance.random_vit(dict(n_channels=3, embed_dim=128, n_layers=1, n_attention_heads=4, forward_mul=2, image_size=32,
                                            patch_size=4), seed=0, n_fake=64).load_real(stats)
    assert again(holder) == last


def test_trainer_without_fid_is_as_before(tmp_path):
    from vit_gan_amd.training import train_model
    out = train_model(CFG, dataset=_dataset(N=20, seed=10), max_epochs=1, output_base=str(tmp_path), fid="")
    log = open(os.path.join(out["dirs"].save, "training.log")).read()
    assert len(re.findall(r"Epoch \[0/1\] \| Disc Loss: \S+, Gen Loss: \S+ \| FID: nan\n", log)) == 1, log
    assert "Frechet" not in log and "fid" not in out and not os.path.exists(os.path.join(out["dirs"].save, "real_stats.npz"))
    assert glob.glob(os.path.join(out["dirs"].checkpoints, "best_model_*")) == []
