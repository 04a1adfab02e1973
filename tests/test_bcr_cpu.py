"""Balanced consistency regularisation without a GPU: the float64 restatement (tests/bcr_ref.py) against torch autograd on the formula,
a float32 emulation of the kernel's operation order against the bound the GPU tests hold the kernel to, four planted mistakes that
must leave that bound, the argument errors of the Python surface, and the export of the C entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

import bcr_ref as br
import vit_gan_amd  # noqa: F401
from second_order_ref import assert_elementwise
from vit_gan_amd import _lib

F64 = torch.float64
SIZES = [(B, Kc) for B in (1, 7, 256, 1000) for Kc in (1, 10)]
SCALES = ["unit", "dc_offset"]
W_REAL, W_FAKE = 10.0, 2.5  # exact in fp32, and different: a swap is visible


def logits(B, Kc, scale, seed=0):
    """fp32 logits [2B, Kc] on x and on T(x): of order 1, or on a DC offset of 100 with differences of order 1e-2"""
    g = torch.Generator().manual_seed(seed * 1000 + B * 10 + Kc)
    lx = torch.randn(2 * B, Kc, generator=g)
    if scale == "unit":
        return lx, torch.randn(2 * B, Kc, generator=g)
    lx = 100.0 + lx
    return lx, lx + 1e-2 * torch.randn(2 * B, Kc, generator=g)


def check(got, ref, Kc, what):
    """(loss, gx, ga) against the restatement inside the derived bound; returns the worst fraction of it"""
    n, n_real = ref["gx"].shape[0], ref["gx"].shape[0] // 2
    loss, gx, ga = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t) for t in got)
    worst = assert_elementwise(loss, ref["loss"], ref["loss_mag"], br.kappa_losses(n, n_real, Kc), what + " loss", rel=0.0)
    worst = max(worst, assert_elementwise(gx, ref["gx"], ref["gx_mag"], br.kappa_grad(), what + " d/dD(x)", rel=0.0))
    return max(worst, assert_elementwise(ga, ref["ga"], ref["ga_mag"], br.kappa_grad(), what + " d/dD(T x)", rel=0.0))


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,Kc", [(1, 1), (7, 10), (256, 1)])
def test_restatement_equals_autograd_on_the_formula(B, Kc, scale):
    lx, la = (t.double().requires_grad_(True) for t in logits(B, Kc, scale))
    total, parts = br.autograd_consistency(lx, la, B, W_REAL, W_FAKE)
    gx, ga = torch.autograd.grad(total, (lx, la))
    ref = br.consistency(lx, la, B, W_REAL, W_FAKE)
    tol = 1e-12
    for s in range(2):
        assert abs(float(parts[s].detach()) - float(ref["loss"][s])) <= tol * (1 + float(parts[s].detach()))
    assert float((gx - ref["gx"]).abs().max()) <= tol * (1 + float(gx.abs().max()))
    assert float((ga - ref["ga"]).abs().max()) <= tol * (1 + float(ga.abs().max()))
    assert torch.equal(ref["ga"], -ref["gx"]) and float(ref["gx"].abs().max()) > 0  # both branches carry gradient, opposite signs
    # accumulate adds to what is there, grad_scale scales the gradients and leaves the losses, a zero weight changes nothing
    old_x, old_a = torch.randn(2 * B, Kc, dtype=F64), torch.randn(2 * B, Kc, dtype=F64)
    acc = br.consistency(lx, la, B, W_REAL, W_FAKE, grad_scale=0.5, into_x=old_x, into_a=old_a)
    assert torch.allclose(acc["gx"], old_x + 0.5 * ref["gx"], rtol=0, atol=1e-12) and torch.allclose(acc["ga"], old_a + 0.5 * ref["ga"], rtol=0, atol=1e-12)
    assert torch.equal(acc["loss"], ref["loss"])
    zero = br.consistency(lx, la, B, 0.0, W_FAKE, into_a=old_a)
    assert torch.equal(zero["gx"][:B], torch.zeros(B, Kc, dtype=F64)) and torch.equal(zero["ga"][:B], old_a[:B])
    assert torch.equal(zero["loss"], ref["loss"]) and torch.equal(zero["gx"][B:], ref["gx"][B:])


def test_the_mean_is_over_images():
    """two logits per image that each differ by 1: |D(x) - D(T x)|^2 = 2 per image, whatever the batch"""
    lx = torch.zeros(6, 2)
    ref = br.consistency(lx, lx + 1.0, 2, 1.0, 1.0)
    assert ref["loss"].tolist() == [2.0, 2.0]
    assert torch.equal(ref["gx"][:2], torch.full((2, 2), -1.0, dtype=F64)) and torch.equal(ref["gx"][2:], torch.full((4, 2), -0.5, dtype=F64))


# ------------------------------------------------------------------------------------------------------------- the bound
def test_kappa_follows_the_kernel():
    assert br.kappa_grad() == 6
    assert br.kappa_loss(1, 1) == 3 + 1 + 6 + 3 + 2 + 1 and br.kappa_loss(256, 1) == 16 and br.kappa_loss(1000, 10) == 15 + 40
    assert br.kappa_losses(2000, 1000, 10) == 55


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,Kc", SIZES)
def test_float32_emulation_stays_inside_the_bound(B, Kc, scale):
    lx, la = logits(B, Kc, scale)
    ref = br.consistency(lx, la, B, W_REAL, W_FAKE)
    worst = check(br.emulate32(lx.numpy(), la.numpy(), B, W_REAL, W_FAKE), ref, Kc, f"B {B} Kc {Kc} {scale}")
    old_x, old_a = torch.randn(2 * B, Kc), torch.randn(2 * B, Kc)
    acc = br.consistency(lx, la, B, W_REAL, W_FAKE, grad_scale=0.5, into_x=old_x, into_a=old_a)
    worst = max(worst, check(br.emulate32(lx.numpy(), la.numpy(), B, W_REAL, W_FAKE, 0.5, old_x.numpy(), old_a.numpy()), acc, Kc, "accumulating"))
    assert worst <= 1.0
    if scale == "dc_offset":  # the expanded square a^2 - 2ab + b^2 would lose everything here: the bound does not admit it
        a, b = lx.numpy(), la.numpy()
        expanded = (a * a - np.float32(2) * a * b + b * b).reshape(2, -1).sum(1) / np.float32(B)
        lim = br.kappa_losses(2 * B, B, Kc) * 2.0 ** -24 * ref["loss_mag"].numpy()
        assert (np.abs(expanded.astype(np.float64) - ref["loss"].numpy()) > lim).any()


@pytest.mark.parametrize("mistake", ["same_sign", "mean_over_elements", "no_factor_2", "swapped_weights"])
@pytest.mark.parametrize("scale", SCALES)
def test_planted_mistakes_leave_the_bound(mistake, scale):
    B, Kc = 7, 10
    lx, la = logits(B, Kc, scale)
    ref = br.consistency(lx, la, B, W_REAL, W_FAKE)
    check(br.emulate32(lx.numpy(), la.numpy(), B, W_REAL, W_FAKE), ref, Kc, "the kernel's order")
    with pytest.raises(AssertionError, match="outside"):
        check(br.emulate32(lx.numpy(), la.numpy(), B, W_REAL, W_FAKE, mistake=mistake), ref, Kc, mistake)


# --------------------------------------------------------------------------------------------------- the Python surface
def test_engine_and_trainer_refuse_bad_arguments_without_a_device():
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.training import train_model
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1))
    G = SirenGenerator(layers=1)
    for bad in ((-1.0, 1.0), (1.0, float("nan")), (float("inf"), 0.0), (1.0,), 3.0, None):
        with pytest.raises(ValueError, match="bcr"):
            GanEngine(D, G, batch=4, bcr=bad, diffaug="color")
    with pytest.raises(ValueError, match="needs a transform"):
        GanEngine(D, G, batch=4, bcr=(10.0, 10.0))
    with pytest.raises(ValueError, match="diffaug's own transform"):
        GanEngine(D, G, batch=4, bcr=(10.0, 10.0), diffaug="color", bcr_aug="translation")
    with pytest.raises(ValueError, match="bcr_aug.*weights"):
        GanEngine(D, G, batch=4, bcr_aug="translation")
    with pytest.raises(ValueError, match="color, translation, cutout"):
        GanEngine(D, G, batch=4, bcr=(10.0, 10.0), bcr_aug="flip")
    with pytest.raises(ValueError, match="two_stream"):
        GanEngine(D, G, batch=4, bcr=(10.0, 10.0), bcr_aug="translation", two_stream=True)
    with pytest.raises(ValueError, match="fuse_real_fake"):
        GanEngine(D, G, batch=4, bcr=(10.0, 0.0), bcr_aug="translation", fuse_real_fake=False)
    with pytest.raises(ValueError, match="bcr"):
        train_model(bcr=(-1.0, 0.0), diffaug="color", save_artifacts=False)
    with pytest.raises(ValueError, match="bcr"):
        train_model(bcr=(10.0, 10.0), save_artifacts=False)
    with pytest.raises(ValueError, match="diffaug's own transform"):
        train_model(bcr=(10.0, 10.0), diffaug="color", bcr_aug="cutout", save_artifacts=False)
    # a good set of arguments gets as far as the device check
    with pytest.raises(RuntimeError, match="cuda|MI355X"):
        GanEngine(D, G, batch=4, bcr=(10.0, 10.0), bcr_aug="translation,cutout")


def test_consistency_loss_has_no_cpu_fallback():
    from vit_gan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consistency_loss(torch.zeros(4, 1), torch.zeros(4, 1), 2, 1.0, 1.0)
    with pytest.raises(ValueError, match="bcr"):
        ops.consistency_loss(torch.zeros(4, 1), torch.zeros(4, 1), 2, -1.0, 1.0)


# -------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_point_is_exported_and_validates_before_any_launch():
    lib = _lib.lib()
    assert hasattr(lib, "vg_bcr_loss") and "vg_bcr_loss" in _lib._SIGNATURES
    assert lib.vg_abi_version() == 9
    p = C.c_void_p(4096)  # never dereferenced: validation fails first
    f = lambda lx=p, la=p, dx=p, da=p, out=p, Br=4, Bf=4, Kc=1, wr=1.0, wf=1.0, ax=0, aa=0: lib.vg_bcr_loss(  # noqa: E731
        lx, la, dx, da, out, Br, Bf, Kc, wr, wf, ax, aa, 1.0, None)
    for name in ("lx", "la", "dx", "da", "out"):
        assert f(**{name: None}) == -1, name
    assert f(Br=0) == -1 and f(Bf=0) == -1 and f(Kc=0) == -1 and f(Br=-3) == -1
    assert f(wr=-1.0) == -2 and f(wf=float("nan")) == -2 and f(ax=2) == -2 and f(aa=-1) == -2
    assert f(Br=1 << 30, Bf=1 << 30, Kc=2) == -2
