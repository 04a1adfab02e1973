"""Class conditioning without a GPU: the off-device restatement (tests/cond_ref.py) against torch autograd, ``index_add_`` and the
one-hot-concat form of the oracle generator; the statistics of the label hash; the C ABI of the new exports and their host-side
return codes; the module's state_dict; every argument error of the engine and the trainer.  Every test here fails on the parent
commit's library and package: the exports and the keyword arguments are this feature's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cond_ref as cr
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib
from vit_gan_amd.config import Config

SEED = 0x1234ABCD5678EF01


def _logits(n, Kc, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, Kc, generator=g, dtype=torch.float64) * scale, torch.randint(0, Kc, (n,), generator=g)


# --------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("role", [0, 1, 2])
def test_restated_loss_is_autograd_on_the_gathered_logits(kind, role):
    for n, Kc in ((1, 1), (7, 3), (300, 10)):
        lg, y = _logits(n, Kc, 10 * n + Kc)
        x = lg.clone().requires_grad_(True)
        want = cr.torch_cond_loss(x, y, cr.KINDS[kind], role)
        (gx,) = torch.autograd.grad(want, x)
        want = want.detach()
        loss, dl, sel = cr.cond_loss64(lg.numpy(), y.numpy(), kind, role)
        assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
        np.testing.assert_allclose(dl, gx.numpy(), rtol=1e-12, atol=1e-15)
        assert np.array_equal(sel, lg.gather(1, y.reshape(-1, 1)).reshape(-1).numpy())
        assert int((dl != 0).sum()) <= n, "at most one non-zero gradient per row"
        # the kernel's fp32 order lies within fp32 round-off of it: n terms of magnitude <= max|l|, and a grad_scale
        l32, d32, s32 = cr.cond_loss32(lg.numpy(), y.numpy(), kind, role, 0.5)
        assert abs(float(l32) - loss) <= 2.0 ** -22 * (8 + np.log2(max(n, 2))) * max(1.0, float(np.abs(lg.numpy()).max()) + 1.0)
        # d = sigmoid(x) - t cancels: a few roundings of values <= 1 (2^-24 each), then the scaling by inv and grad_scale
        np.testing.assert_allclose(d32, 0.5 * dl, rtol=2.0 ** -21, atol=2.0 ** -21 * 0.5 / n)


def test_restated_table_gradient_is_index_add():
    g = torch.Generator().manual_seed(5)
    for B, N, K in ((1, 8, 1), (6, 16, 3), (67, 40, 10)):
        dw = torch.randn(B, N, generator=g)
        y = torch.randint(0, K, (B,), generator=g)
        want = torch.zeros(K, N, dtype=torch.float64).index_add_(0, y, dw.double())
        got = cr.class_grad(dw.numpy(), y.numpy(), K)
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=2.0 ** -23 * B * float(dw.abs().max()))
        old = torch.randn(K, N, generator=g).numpy()
        acc = cr.class_grad(dw.numpy(), y.numpy(), K, into=old)
        np.testing.assert_allclose(acc, old + want.numpy(), rtol=0, atol=2.0 ** -22 * (B + 1) * (float(dw.abs().max()) + float(np.abs(old).max())))
        for k in set(range(K)) - set(y.tolist()):  # absent: +0 when overwriting, untouched when accumulating
            assert np.array_equal(got[k].view(np.uint32), np.zeros(N, dtype=np.uint32)) and np.array_equal(acc[k], old[k])
    # labels out of range are clamped, not dropped
    assert np.array_equal(cr.class_grad(np.ones((2, 4), np.float32), [-5, 99], 3), np.array([[1] * 4, [0] * 4, [1] * 4], np.float32))


def test_class_add_rounds_to_nearest_even():
    x = torch.tensor([1.0, 1.0, 1.0, -2.5, 3.0e38, 1.0, 0.0, 5.0]).to(torch.bfloat16).reshape(1, 8)
    t = torch.tensor([[2.0 ** -8, 3 * 2.0 ** -9, 2.0 ** -9, 2.5, 0.0, 2.0 ** -7, -0.0, 0.25]]).to(torch.bfloat16)
    got = cr.bf16_bits_to_f32(cr.class_add(cr.bits_of(x), cr.bits_of(t), [0]))
    want = (x.float() + t.float()).to(torch.bfloat16).float().numpy()  # torch's cast is round-to-nearest-even
    assert np.array_equal(got, want)
    assert got[0, 0] == 1.0 and got[0, 1] == 1.0 + 2.0 ** -7 and got[0, 2] == 1.0, "a tie goes to the even mantissa"


def test_gather_form_equals_the_onehot_concat_oracle():
    from oracle import gen_oracle as go
    d = go.GenDims(latent=16, tokens=8, embed=64, heads=2, layers=1, siren_hidden=32, channels=3, image=8)
    K, B = 3, 5
    st = {k: v.double() for k, v in go.init_gen_state(d, seed=2).items()}
    g = torch.Generator().manual_seed(1)
    table = (torch.rand(K, d.tokens * d.embed, generator=g, dtype=torch.float64) * 2 - 1) / 4
    z = torch.randn(B, d.latent, generator=g, dtype=torch.float64)
    y = torch.tensor([0, 2, 2, 0, 1])
    ext = go.gen_forward(cr.extended_state(st, table), cr.extended_latent(z, y, K), d)
    gat = cr.gen_forward_gather(st, table, z, y, d)
    assert ext.shape == gat.shape == (B, 3, 8, 8)
    assert float((ext - gat).abs().max()) < 1e-9, "sin(30 x) amplifies the 1e-16 reassociation of the K extra products"
    assert float((ext - go.gen_forward(st, z, d)).abs().max()) > 1e-3, "the table moves the image"


# ----------------------------------------------------------------------------------------------------------------- the label hash
def test_label_draws_are_in_range_uniform_and_move():
    for K, q999 in ((10, 27.877), (3, 13.816)):  # the 99.9 % quantiles of chi-square with K - 1 degrees of freedom
        n = 4096 * K
        y = cr.draw_labels(n, K, SEED, cr.LABEL_SITE, 1)
        assert y.dtype == np.int32 and int(y.min()) >= 0 and int(y.max()) < K
        counts = np.bincount(y, minlength=K).astype(np.float64)
        chi2 = float(((counts - n / K) ** 2 / (n / K)).sum())
        print(f"K {K}: chi-square {chi2:.3f} over {n} draws (99.9 % quantile {q999})")
        assert chi2 < q999
    for K in (1, 16):
        y = cr.draw_labels(1000, K, SEED, cr.LABEL_SITE, 7)
        assert int(y.min()) >= 0 and int(y.max()) < K
    a = cr.draw_labels(256, 10, SEED, cr.LABEL_SITE, 1)
    assert not np.array_equal(a, cr.draw_labels(256, 10, SEED, cr.LABEL_SITE, 2)), "consecutive steps"
    assert not np.array_equal(a, cr.draw_labels(256, 10, SEED, 2, 1)) and not np.array_equal(a, cr.draw_labels(256, 10, SEED, 0, 1)), "sites"
    assert not np.array_equal(a, cr.draw_labels(256, 10, SEED + 1, cr.LABEL_SITE, 1)), "seeds"
    assert np.array_equal(a, cr.draw_labels(256, 10, SEED, cr.LABEL_SITE, 1)) and np.array_equal(a[:67], cr.draw_labels(67, 10, SEED, cr.LABEL_SITE, 1))


# ------------------------------------------------------------------------------------------------------------------------ C ABI
NEW = ("vg_draw_labels", "vg_class_add", "vg_class_grad", "vg_gan_loss_cond", "vg_gan_loss_cond_pair")
GEN = ("vg_gen_forward_cond", "vg_gen_backward_cond", "vg_gen_backward_stages_cond")


def test_exports_exist_with_abi_9():
    lib = _lib.lib()
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitgan_hip.h")).read()
    for name in NEW + GEN:
        assert hasattr(lib, name) and name in _lib._SIGNATURES and f"int {name}(" in header, name
    assert "typedef struct VgGenCond" in header and [f[0] for f in _lib.VgGenCond._fields_] == ["labels", "table_bf16", "table_grad", "K"]


def test_return_codes_come_back_before_any_launch():
    lib, p = _lib.lib(), C.c_void_p(64)  # (a non-null, 16-byte aligned dummy: never dereferenced on these paths; no device here)
    odd = C.c_void_p(72)
    assert lib.vg_draw_labels(None, 4, 3, 1, 3, None, None) == -1 and lib.vg_draw_labels(p, 0, 3, 1, 3, None, None) == -1
    assert lib.vg_draw_labels(p, 4, 0, 1, 3, None, None) == -2 and lib.vg_draw_labels(p, 4, 17, 1, 3, None, None) == -2
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.vg_class_add(*a, 2, 8, 3, None) == -1 and lib.vg_class_grad(*a, 2, 8, 3, 0, None) == -1
    assert lib.vg_class_add(p, p, p, 0, 8, 3, None) == -1 and lib.vg_class_add(p, p, p, 2, 0, 3, None) == -1
    assert lib.vg_class_add(p, p, p, 2, 8, 0, None) == -2 and lib.vg_class_add(p, p, p, 2, 8, 17, None) == -2
    assert lib.vg_class_add(p, p, p, 2, 12, 3, None) == -3 and lib.vg_class_add(odd, p, p, 2, 8, 3, None) == -3
    assert lib.vg_class_grad(p, p, p, 0, 8, 3, 0, None) == -1
    assert lib.vg_class_grad(p, p, p, 2, 8, 0, 0, None) == -2 and lib.vg_class_grad(p, p, p, 2, 8, 17, 1, None) == -2
    assert lib.vg_class_grad(p, p, p, 2, 8, 3, 2, None) == -2
    assert lib.vg_class_grad(p, p, p, 2, 6, 3, 0, None) == -3 and lib.vg_class_grad(p, p, odd, 2, 8, 3, 0, None) == -3
    for a in ((None, p, p, None, p), (p, None, p, None, p), (p, p, None, None, p), (p, p, p, None, None)):
        assert lib.vg_gan_loss_cond(*a, 4, 3, 0, 0, 1.0, None) == -1 and lib.vg_gan_loss_cond_pair(*a, 4, 0, 4, 1, 3, 0, 1.0, None) == -1
    assert lib.vg_gan_loss_cond(p, p, p, None, p, 0, 3, 0, 0, 1.0, None) == -1
    assert lib.vg_gan_loss_cond_pair(p, p, p, p, p, 4, 0, 0, 1, 3, 0, 1.0, None) == -1
    for Kc in (0, 17):
        assert lib.vg_gan_loss_cond(p, p, p, None, p, 4, Kc, 0, 0, 1.0, None) == -2
        assert lib.vg_gan_loss_cond_pair(p, p, p, p, p, 4, 0, 4, 1, Kc, 0, 1.0, None) == -2
    assert lib.vg_gan_loss_cond(p, p, p, None, p, 4, 3, 3, 0, 1.0, None) == -2 and lib.vg_gan_loss_cond(p, p, p, None, p, 4, 3, 0, 3, 1.0, None) == -2
    assert lib.vg_gan_loss_cond(p, p, p, None, p, 2 ** 30, 16, 0, 0, 1.0, None) == -2, "(n0 + n1) Kc >= 2^31"
    # the generator passes: the conditioning argument is checked before anything is enqueued
    d = _lib.VgGenDims(1024, 32, 384, 4, 2, 768, 96, 30.0, 0, 3, 32)
    net = _lib.VgGenNet(d, 64, 64, 64, 0.0, 0, None, None)
    cond = lambda *f: C.byref(_lib.VgGenCond(*f))  # noqa: E731
    assert lib.vg_gen_forward_cond(C.byref(net), 2, p, p, p, cond(None, 64, None, 3), None) == -1
    assert lib.vg_gen_forward_cond(C.byref(net), 2, p, p, p, cond(64, None, None, 3), None) == -1
    assert lib.vg_gen_forward_cond(C.byref(net), 2, p, p, p, cond(64, 64, None, 0), None) == -2
    assert lib.vg_gen_forward_cond(C.byref(net), 2, p, p, p, cond(64, 64, None, 17), None) == -2
    assert lib.vg_gen_backward_cond(C.byref(net), 2, p, p, cond(64, 64, None, 3), None) == -1, "a backward needs table_grad"
    assert lib.vg_gen_backward_stages_cond(C.byref(net), 2, p, p, 0, 1, cond(64, 64, 64, 17), None) == -2
    assert lib.vg_gen_backward_stages_cond(C.byref(net), 2, p, p, 3, 2, cond(64, 64, 64, 3), None) == -2


# ----------------------------------------------------------------------------------------------------------------------- modules
def _small_gen(**kw):
    from vit_gan_amd.generator import SirenGenerator
    return SirenGenerator(latent=64, embed=128, heads=4, layers=1, siren_hidden=128, dropout=0.0, **kw)


def test_state_dict_keys_of_the_generator():
    from oracle import gen_oracle as go
    from vit_gan_amd import flat
    torch.manual_seed(0)
    G0 = _small_gen()
    torch.manual_seed(0)
    G3 = _small_gen(n_classes=3)
    d = go.GenDims(latent=64, embed=128, heads=4, layers=1, siren_hidden=128)
    assert list(G0.state_dict()) == list(go.gen_param_shapes(d)), "n_classes=0: today's keys, in order"
    assert list(G3.state_dict()) == list(G0.state_dict()) + ["class_embedding.weight"]
    T_E = G3._dims.T * G3._dims.E
    w = G3.class_embedding.weight
    assert w.shape == (3, T_E) and float(w.detach().abs().max()) <= 1 / 8 and float(w.detach().abs().max()) > 0.9 / 8, "U(+-1/sqrt(latent)), latent = 64"
    for k, v in G0.state_dict().items():
        assert torch.equal(v, G3.state_dict()[k]), f"{k}: the table is drawn last, the other parameters keep their draws"
    lay = flat.gen_layout(G3._dims)
    off, total = flat.gen_class_table(G3._dims, 3)
    assert off >= lay.total and off % 64 == 0 and total == off + 3 * T_E == G3._flat.total and G0._flat.total == lay.total
    assert G3._flat.slots["class_embedding.weight"] == (off, (3, T_E)) and G3._flat.aliased()
    assert w.data_ptr() == G3._flat.flat.data_ptr() + 4 * off
    for bad in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="n_classes"):
            _small_gen(n_classes=bad)
    with pytest.raises(ValueError, match="labels"):
        G3._labels(None, 2, torch.device("cpu"))
    with pytest.raises(ValueError, match="labels"):
        G0._labels(torch.zeros(2, dtype=torch.int64), 2, torch.device("cpu"))
    for bad, match in ((torch.zeros(2), "integer"), (torch.zeros(3, dtype=torch.int64), "shape"), (torch.tensor([0, 3]), r"\[0, 3\)"),
                       (torch.tensor([-1, 0]), r"\[0, 3\)")):
        with pytest.raises(ValueError, match=match):
            G3._labels(bad, 2, torch.device("cpu"))
    assert G3._labels(torch.tensor([2, 0]), 2, torch.device("cpu")).dtype == torch.int32


def _nets(Kc=3, n_classes=3):
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=Kc, dropout_rate=0.0, batch_size=4, transformer_blocks_count=1))
    return D, _small_gen(n_classes=n_classes)


def test_engine_refuses_bad_combinations_without_a_device(monkeypatch):
    from vit_gan_amd import engine
    D, G = _nets()
    for kw, match in ((dict(gp_weight=10.0, loss="wasserstein"), "gradient penalties"), (dict(r1_gamma=10.0), "gradient penalties"),
                      (dict(two_stream=True), "two_stream"), (dict(n_classes=2), "classes_count=3, generator.n_classes=3, n_classes=2"),
                      (dict(n_classes=0), "classes_count=3, generator.n_classes=3, n_classes=0"), (dict(n_classes=17), "n_classes"),
                      (dict(n_classes=True), "n_classes"), (dict(n_classes=3.0), "n_classes")):
        with pytest.raises(ValueError, match=match):
            engine.GanEngine(D, G, batch=4, **{"n_classes": 3, **kw})
    D1, G0 = _nets(Kc=1, n_classes=0)
    with pytest.raises(ValueError, match="classes_count=1, generator.n_classes=0, n_classes=3"):
        engine.GanEngine(D1, G0, batch=4, n_classes=3)
    D3, G0 = _nets(Kc=3, n_classes=0)
    with pytest.raises(ValueError, match="classes_count=3, generator.n_classes=0, n_classes=3"):
        engine.GanEngine(D3, G0, batch=4, n_classes=3)
    monkeypatch.setattr(engine, "world_size", lambda pg: 2)
    with pytest.raises(ValueError, match="more than one rank"):
        engine.GanEngine(D, G, batch=4, n_classes=3)
    monkeypatch.undo()
    # what is allowed gets as far as the device check: no argument error
    for kw in (dict(), dict(exchange_single_rank=True), dict(diffaug="color", ada_target=0.6), dict(bcr=(1, 1), bcr_aug="translation"),
               dict(ema_decay=0.99), dict(spectral_norm="qkv"), dict(fuse_real_fake=False)):
        with pytest.raises(RuntimeError, match="cuda"):
            engine.GanEngine(D, G, batch=4, n_classes=3, **kw)
    with pytest.raises(RuntimeError, match="cuda"):  # off is off: a Kc = 3 head without labels stays what it was
        engine.GanEngine(D3, G0, batch=4)


def test_trainer_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.training import SyntheticLoader, train_model, trainable_config
    for kw, match in ((dict(gp_weight=10.0, loss="wasserstein"), "conditional"), (dict(r1_gamma=1.0), "conditional"),
                      (dict(config=dict(classes_count=17)), "classes_count")):
        with pytest.raises(ValueError, match=match):
            train_model(conditional=True, save_artifacts=False, **kw)
    c = Config(classes_count=7)
    assert trainable_config(c).classes_count == 1 and trainable_config(c, conditional=True).classes_count == 7
    assert trainable_config(c, True).generator_kind == trainable_config(c).generator_kind == "sln_siren"
    c = Config(batch_size=4, image_size=8)
    (x, y), = list(SyntheticLoader(c, 1, torch.device("cpu"), labels=3))
    assert y.shape == (4,) and y.dtype == torch.int64 and 0 <= int(y.min()) and int(y.max()) < 3
    (x0, none), = list(SyntheticLoader(c, 1, torch.device("cpu")))
    assert none is None and torch.equal(x0, x), "labels are drawn behind the images: the images of a seed stay"
