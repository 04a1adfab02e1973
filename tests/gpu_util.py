"""Helpers for the -m gpu parity tests: raw C-ABI calls on torch device tensors."""
import ctypes

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


def off(t, elems):
    """the address of element ``elems`` of ``t``"""
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


GUARD, MARK = 64, -777.25  # elements in front of and behind a guarded buffer's body, and what they hold


def guard_mark(dtype):
    """the guard pattern as ``dtype`` holds it (bf16 rounds it, int32 truncates it)"""
    return torch.tensor(MARK).to(dtype).item()


def guarded(n, fill, dtype=torch.float32):
    """a [GUARD | n | GUARD] device buffer: the guards hold a recognisable pattern, the body ``fill`` (a value or a tensor); a kernel is
    handed ``off(buf, GUARD)``"""
    buf = torch.full((n + 2 * GUARD,), guard_mark(dtype), dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = fill if not torch.is_tensor(fill) else fill.reshape(-1).to(dtype).cuda()
    return buf


def assert_intact(buf, what):
    m = guard_mark(buf.dtype)
    assert bool((buf[:GUARD] == m).all()) and bool((buf[-GUARD:] == m).all()), f"{what}: a guard element was written"


def adamw_state(n, seed):
    """(p, m, v, g, generator) with per-element edges: gradients of exactly 0 (eps dominates), ~1e-6, ~1 and ~1e3; moments carried over
    from earlier steps (some zero); |p| from 1e-4 to 10.  The generator is handed back for what a caller draws on top (an average)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.sign(torch.randn(n, generator=gen)) * 10.0 ** (torch.rand(n, generator=gen) * 5 - 4)
    g = torch.randn(n, generator=gen) * torch.tensor([0.0, 1e-6, 1.0, 1e3])[torch.arange(n) % 4]
    h = torch.tensor([1.0, 1e-6, 1e3, 0.0])[torch.randperm(n, generator=gen) % 4]
    m = torch.randn(n, generator=gen) * h * 0.3
    v = (torch.randn(n, generator=gen) * h) ** 2
    return p, m, v, g, gen


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
