"""Differentiable augmentation without a GPU: the restatement checks itself (tests/diffaug_ref.py), the parameter function is held to
the uniform distributions it claims, the two C entry points validate their arguments before any launch, and the Python surface refuses
what it does not take."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import diffaug_ref as dr
import vit_gan_amd  # noqa: F401
from second_order_ref import assert_elementwise
from vit_gan_amd import _lib

F64 = torch.float64


def _images(B, Cc, IH, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, Cc, IH, IH, generator=g) * 2 - 1 + offset).to(torch.bfloat16)).double()


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("policy", range(8))
@pytest.mark.parametrize("Cc,IH", [(3, 32), (3, 36), (1, 32), (8, 9)])
def test_adjoint_is_the_transpose(policy, Cc, IH):
    """hand-written adjoint == autograd's gradient of <T x, w>, and <T x, w> = <x, T^T w> + <T 0, w>, both to 1e-12"""
    B = 6
    params = dr.draw(11, 0, 5, B, IH, policy)
    x = _images(B, Cc, IH, 1).requires_grad_(True)
    w = torch.randn(B, Cc, IH, IH, dtype=F64, generator=torch.Generator().manual_seed(2))
    y, _ = dr.augment(x, params)
    (gx,) = torch.autograd.grad((y * w).sum(), x)
    y = y.detach()
    adj, _ = dr.adjoint(w, params)
    scale = float(w.abs().max())
    assert float((gx - adj).abs().max()) <= 1e-12 * scale
    y0, _ = dr.augment(torch.zeros_like(x), params)
    lhs, rhs = float((y * w).sum()), float((x.detach() * adj).sum() + (y0 * w).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((y * w).abs().sum() + 1)
    if policy == 0:
        assert float((y - x.detach()).abs().max()) <= 1e-12 and float((adj - w).abs().max()) <= 1e-12 * scale
    # off the live pixels the output is exactly zero, and the cutout / the frame really remove something when they are on
    live = dr.live_mask(params, IH).expand_as(y)
    assert float(y[~live].abs().sum()) == 0.0
    if policy & 6:
        assert int((~live).sum()) > 0


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("Cc,IH", [(3, 32), (3, 36), (3, 64), (3, 224), (1, 32)])
def test_float32_evaluation_stays_inside_the_bound(Cc, IH, offset):
    """the bound the GPU tests hold the kernels to (rel = 0: no bf16 rounding here) admits a float32 evaluation of the restatement,
    at image scale and on a large DC offset where the means cancel"""
    B = 3
    params = dr.draw(7, 1, 3, B, IH, 7)
    x = _images(B, Cc, IH, 3, offset)
    w = _images(B, Cc, IH, 4, offset)
    y64, mag = dr.augment(x, params)
    y32, _ = dr.augment(x, params, dtype=torch.float32)
    assert_elementwise(y32, y64, mag, dr.kappa(Cc, IH), "float32 forward", rel=0.0)
    a64, amag = dr.adjoint(w, params)
    a32, _ = dr.adjoint(w, params, dtype=torch.float32)
    assert_elementwise(a32, a64, amag, dr.kappa(Cc, IH), "float32 adjoint", rel=0.0)


def test_kappa_follows_the_reduction_tree():
    assert dr.threads(32) == 128 and dr.threads(36) == 192 and dr.threads(8) == 64 and dr.threads(224) == 1024
    assert dr.kappa(3, 32) == (3 + 3 + 6 + 2 + 2) + 5 + 9
    assert dr.kappa(3, 224) == (3 + 3 * 7 + 6 + 16 + 2) + 5 + 9


# ------------------------------------------------------------------------------------------------ the parameter function
SEED, SITE, STEPS, IMAGES, IH_STAT = 20240607, 0, 256, 256, 32  # 65 536 (step, image) pairs


def _stream(p, seed=SEED, site=SITE):
    return dr.k24(seed, site, np.arange(1, STEPS + 1)[:, None], np.arange(IMAGES)[None, :], p)  # [step, image]


def _lag1(a, axis):
    a = a.astype(np.float64) - a.mean()
    x, y = (a[:-1], a[1:]) if axis == 0 else (a[:, :-1], a[:, 1:])
    return float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum())), x.size


@pytest.mark.parametrize("p", range(7))
def test_parameters_are_uniform_and_uncorrelated(p):
    k = _stream(p)
    n = k.size
    assert n == 65536 and int(k.max()) < 1 << 24
    r = IH_STAT // 8
    if p < 3:
        v = k.astype(np.float64) * 2.0 ** -24
        v, lo, hi = ((v - 0.5, -0.5, 0.5), (2 * v, 0.0, 2.0), (v + 0.5, 0.5, 1.5))[p]
        assert v.min() >= lo and v.max() < hi
        mean, sd = (lo + hi) / 2, (hi - lo) / math.sqrt(12)
    else:
        m, base = (2 * r + 1, -r) if p < 5 else (IH_STAT + 1, 0)
        v = ((k * np.uint64(m)) >> np.uint64(24)).astype(np.int64) + base
        assert v.min() >= base and v.max() <= base + m - 1
        assert set(np.unique(v).tolist()) == set(range(base, base + m))  # every value of tx, ty, cx, cy occurs
        mean, sd = base + (m - 1) / 2, math.sqrt((m * m - 1) / 12)
        v = v.astype(np.float64)
    assert abs(v.mean() - mean) <= 5 * sd / math.sqrt(n), (p, v.mean(), mean)
    for axis in (0, 1):  # across steps, across images
        c, cnt = _lag1(v, axis)
        assert abs(c) <= 5 / math.sqrt(cnt), (p, axis, c)


def test_sites_and_seeds_give_different_streams():
    for p in range(7):
        a = _stream(p)
        for other in (_stream(p, site=1), _stream(p, seed=SEED + 1)):
            assert float((a == other).mean()) < 1e-3
            c = np.corrcoef(a.ravel().astype(np.float64), other.ravel().astype(np.float64))[0, 1]
            assert abs(c) <= 5 / math.sqrt(a.size)
    # parameters of one image are different streams too
    assert abs(np.corrcoef(_stream(3).ravel().astype(np.float64), _stream(4).ravel().astype(np.float64))[0, 1]) <= 5 / 256
    # and draw() is what the streams say: identities for members that are off
    d0 = dr.draw(SEED, 0, 1, 4, 32, 0)
    assert (d0 == np.array([0, 1, 1, 0, 0, -32, -32, 0], dtype=np.float32)).all()
    d7 = dr.draw(SEED, 0, 1, 4, 32, 7)
    assert (d7[:, 0] == (_stream(0)[0, :4].astype(np.float64) * 2.0 ** -24 - 0.5).astype(np.float32)).all()
    assert (dr.draw(SEED, 0, 1, 4, 32, 2)[:, 3:5] == d7[:, 3:5]).all() and (dr.draw(SEED, 0, 2, 4, 32, 7) != d7).any()


# -------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_and_validate_before_any_launch():
    lib = _lib.lib()
    for n in ("vg_diffaug_fwd", "vg_diffaug_bwd"):
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert lib.vg_abi_version() == 9
    p = C.c_void_p(4096)  # never dereferenced: validation fails first
    fwd = lambda x=p, y=p, B=4, Cc=3, IH=32, pol=7: lib.vg_diffaug_fwd(x, y, None, B, Cc, IH, pol, 1, 0, None, None)  # noqa: E731
    bwd = lambda x=p, y=p, B=4, Cc=3, IH=32, pol=7: lib.vg_diffaug_bwd(x, y, 0, B, Cc, IH, pol, 1, 0, None, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(x=None) == -1 and f(y=None) == -1 and f(B=0) == -1
        assert f(pol=-1) == -2 and f(pol=8) == -2 and f(Cc=0) == -2 and f(IH=7) == -2 and f(IH=256) == -2
        assert f(Cc=3, IH=9) == -3 and f(Cc=1, IH=10) == -3  # 243 and 100 elements per image


# --------------------------------------------------------------------------------------------------- the Python surface
def test_policy_strings():
    from vit_gan_amd.ops import parse_aug_policy
    assert parse_aug_policy("") == 0 and parse_aug_policy("color") == 1 and parse_aug_policy("translation, cutout") == 6
    assert parse_aug_policy("color,translation,cutout") == 7 and parse_aug_policy(5) == 5
    for bad in ("colour", "color,", "color;cutout", "flip", 8, -1, None):
        with pytest.raises(ValueError, match="color.*translation.*cutout|\\[0, 7\\]"):
            parse_aug_policy(bad)


def test_engine_and_trainer_refuse_bad_policies_without_a_device():
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.training import train_model
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1))
    G = SirenGenerator(layers=1)
    with pytest.raises(ValueError, match="color, translation, cutout"):
        GanEngine(D, G, batch=4, diffaug="color,flip")
    with pytest.raises(ValueError, match="two_stream"):
        GanEngine(D, G, batch=4, diffaug="color", two_stream=True)
    with pytest.raises(ValueError, match="color, translation, cutout"):
        train_model(diffaug="mixup", save_artifacts=False)


def test_diff_augment_has_no_cpu_fallback():
    from vit_gan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.diff_augment(torch.zeros(2, 3, 32, 32), "color", 0, 0)
