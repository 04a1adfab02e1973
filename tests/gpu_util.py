"""Helpers for the -m gpu parity tests: raw C-ABI calls on torch device tensors."""
import torch

import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib

BF = torch.bfloat16
ptr, stream, call = _lib.ptr, _lib.stream, _lib.call


def dev(t, dtype=None):
    t = torch.as_tensor(t)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def rbf(t):
    """round to bf16 and back: the fp32 value the kernel actually sees"""
    return t.to(BF).float()


def sync():
    torch.cuda.synchronize()


def dropout_mask(shape, p, seed, site, step=None):
    """vg_dropout_apply on bf16 ones of ``shape``, as fp32 on the host: 0 where dropped, bf16(256 / (256 - thr)) where kept.
    step: None (no device counter) or a one-element 32-bit integer device tensor"""
    ones = torch.ones(shape, dtype=BF, device="cuda")
    out = torch.empty_like(ones)
    call("vg_dropout_apply", ptr(ones), ptr(out), ones.numel(), p, seed, site, ptr(step), stream())
    sync()
    return out.float().cpu()


def assert_close(got, ref, rel, what="", floor=1e-6):
    """max|got-ref| <= rel * max|ref|  (per-tensor tolerance)"""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= rel * scale + floor, f"{what}: max err {err:.3e} > {rel:g} * max|ref| {scale:.3e}"
    return err / max(scale, floor)
