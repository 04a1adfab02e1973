"""The optimizer kernels on the engine's path: vg_adamw_step with the device step counter (what GanEngine passes) and without it,
against the float64 AdamW of tests/adamw_ref.py, and vg_cast_f32_bf16 (the only writer of the bf16 shadow every GEMM reads)
against torch's round-to-nearest-even."""

import numpy as np
import pytest
import torch

from adamw_ref import check_adamw_step
import gpu_util as u

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LR, EPS = 5e-4, 1e-8


def _run(t, betas, device_counter, n=8196, lo=0, total=None, seed=None, lr=LR, wds=(0.0, 1e-3)):
    """All (gscale, wd) combinations at step t on n elements starting at element lo of buffers of `total` elements."""
    total = n if total is None else total
    p0, m0, v0, g, _ = u.adamw_state(total, seed if seed is not None else 7 * t + int(100 * betas[0]))
    worst = (0.0, 0.0)
    for gscale in (1.0, 0.5, 0.125):
        for wd in wds:
            P, M, V, G_ = (u.dev(x.clone()) for x in (p0, m0, v0, g))
            SH = torch.full((total,), -7.0, dtype=BF, device="cuda")
            step_dev = torch.tensor([t], dtype=torch.int32, device="cuda") if device_counter else None
            u.call("vg_adamw_step", u.off(P, lo), u.off(G_, lo), u.off(M, lo), u.off(V, lo), u.off(SH, lo), n, lr, betas[0], betas[1], EPS, wd,
                   0 if device_counter else t, u.ptr(step_dev), gscale, u.stream())
            u.sync()
            if device_counter:
                assert int(step_dev[0]) == t  # the kernel reads the counter, never writes it
            s = slice(lo, lo + n)
            what = f"t={t} betas={betas} gscale={gscale} wd={wd} {'device' if device_counter else 'host'} counter [{lo}, {lo + n})"
            r = check_adamw_step(p0[s], m0[s], v0[s], g[s], t, (lr, betas[0], betas[1], EPS, wd), gscale, P.cpu()[s], M.cpu()[s], V.cpu()[s],
                                 SH.cpu()[s], what)
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
            # nothing outside the range is touched
            out = torch.ones(total, dtype=torch.bool)
            out[s] = False
            for buf, ref in ((P, p0), (M, m0), (V, v0), (G_, g)):
                assert torch.equal(buf.cpu()[out], ref[out]), f"{what}: wrote outside its range"
            assert bool((SH.cpu()[out] == -7.0).all()), f"{what}: shadow written outside its range"
    return worst


STEPS = [1, 2, 3, 10, 100, 10 ** 4, 10 ** 6]


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("t", STEPS)
def test_adamw_device_counter_matches_fp64(t, betas):
    """The engine's path: the bias corrections computed on the device from the int32 step counter."""
    worst = _run(t, betas, device_counter=True)
    print(f"\nadamw device counter t={t} betas={betas}: worst {worst[0]:.4f} of the bound, update error {worst[1]:.4f} x 2^-12")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("t", STEPS)
def test_adamw_host_counter_matches_fp64(t, betas):
    """step_dev = nullptr: the bias corrections from the host's powf, same bounds."""
    worst = _run(t, betas, device_counter=False)
    print(f"\nadamw host counter t={t} betas={betas}: worst {worst[0]:.4f} of the bound, update error {worst[1]:.4f} x 2^-12")


@pytest.mark.parametrize("t", [1, 10 ** 4])
def test_adamw_on_a_subrange_at_an_element_offset(t):
    """What _adamw_g_sharded issues: the kernel on [lo, lo + n) of larger buffers, lo a multiple of 4 but not of 1024, n not a multiple
    of 1024; nothing outside the range changes."""
    _run(t, (0.9, 0.999), device_counter=True, n=3 * 1024 + 12, lo=1028, total=1028 + 3 * 1024 + 12 + 2052)


@pytest.mark.parametrize("t", [1, 3, 100])
def test_adamw_decays_before_the_moment_step(t):
    """At the engine's lr * wd = 5e-7 the order of decay and step moves a weight by 5e-7 of its update, below any bound above; at
    lr * wd = 0.05 decaying after the step would be 5 % of every update off."""
    _run(t, (0.9, 0.999), device_counter=True, lr=1e-2, wds=(5.0,))


def test_adamw_rejects_a_length_not_divisible_by_4():
    from vit_gan_amd import _lib
    n = 4098
    P, G_, M, V = (torch.full((n,), 0.25, device="cuda") for _ in range(4))
    SH = torch.zeros(n, dtype=BF, device="cuda")
    step_dev = torch.ones(1, dtype=torch.int32, device="cuda")
    for sd in (step_dev, None):
        rc = _lib.lib().vg_adamw_step(u.ptr(P), u.ptr(G_), u.ptr(M), u.ptr(V), u.ptr(SH), n, LR, 0.9, 0.999, EPS, 1e-3, 1, u.ptr(sd), 1.0,
                                      u.stream())
        assert rc != 0
    u.sync()
    assert all(bool((x == 0.25).all()) for x in (P, G_, M, V)) and bool((SH == 0).all()), "a rejected call launched a kernel"


# ---- vg_cast_f32_bf16 ---------------------------------------------------------------------------------------------------------------
def _bits(words):
    return torch.tensor(np.array(words, dtype=np.uint32).view(np.int32)).view(torch.float32)


def _special_words():
    w = [0x00000000, 0x80000000,                                   # +-0
         0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00017FFF, 0x00008001, 0x007FFFFF, 0x807FFFFF, 0x00400000,  # subnormals
         0x7F7F0000, 0x7F7F7FFF, 0x7F7E8000, 0x7F7F8000, 0x7F7FFFFF,    # largest finite: stays, ties down (even), ties up to inf, rounds to inf
         0xFF7F0000, 0xFF7F7FFF, 0xFF7E8000, 0xFF7F8000, 0xFF7FFFFF,
         0x7F800000, 0xFF800000,                                   # +-inf
         0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,  # ties with even / odd mantissa
         0x00800000, 0x00808000, 0x00818000, 0x007F8000, 0x807F8000]  # around the smallest normal (a tie that carries into it)
    rng = np.random.default_rng(11)
    hi = rng.integers(0, 0x7F7F, 256, dtype=np.uint32) | (rng.integers(0, 2, 256, dtype=np.uint32) << 15)
    w += [int(x) for x in (hi << 16) | 0x8000]   # exact ties over the whole exponent range, both signs and mantissa parities
    w += [int(x) for x in (hi << 16) | 0x7FFF] + [int(x) for x in (hi << 16) | 0x8001]
    return w


NAN_WORDS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FBF8000]


def _cast(x, lo=0, total=None):
    n = x.numel()
    total = n if total is None else total
    src = torch.zeros(total, dtype=torch.float32, device="cuda")
    src[lo:lo + n] = x.cuda()
    dst = torch.full((total,), 3.0, dtype=BF, device="cuda")
    u.call("vg_cast_f32_bf16", u.off(src, lo), u.off(dst, lo), n, u.stream())
    u.sync()
    d = dst.cpu()
    out = torch.ones(total, dtype=torch.bool)
    out[lo:lo + n] = False
    assert bool((d[out] == 3.0).all()), "cast wrote outside its range"
    return d[lo:lo + n]


def _assert_rne(x, y):
    want = x.to(BF)  # torch on the host: round to nearest, ties to even; overflow to inf
    nan = torch.isnan(x)
    assert bool(torch.isnan(y[nan]).all()), "NaN input did not stay NaN"
    yb, wb = y[~nan].view(torch.int16), want[~nan].view(torch.int16)
    bad = yb != wb
    assert not bool(bad.any()), [(hex(int(a.view(torch.int32)) & 0xFFFFFFFF), hex(int(b) & 0xFFFF), hex(int(c) & 0xFFFF))
                                 for a, b, c in zip(x[~nan][bad][:6], yb[bad][:6], wb[bad][:6])]


def test_cast_special_values_are_rne():
    words = _special_words() + NAN_WORDS
    words += [0] * (-len(words) % 4)
    x = _bits(words)
    _assert_rne(x, _cast(x))
    # and at an element offset inside a larger buffer, as a ranged refresh issues it
    _assert_rne(x, _cast(x, lo=1028, total=1028 + x.numel() + 1024))


@pytest.mark.parametrize("n", [4, 1020, 1028, (1 << 20) + 4])
def test_cast_random_data_is_rne(n):
    rng = np.random.default_rng(n)
    words = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)  # every exponent, NaNs and infs included
    x = _bits(words)
    x[: n // 2] = torch.randn(n // 2, generator=torch.Generator().manual_seed(n)) * 10.0 ** rng.integers(-8, 8)
    _assert_rne(x, _cast(x))


def test_cast_rejects_a_length_not_divisible_by_4():
    from vit_gan_amd import _lib
    src = torch.ones(6, device="cuda")
    dst = torch.zeros(6, dtype=BF, device="cuda")
    assert _lib.lib().vg_cast_f32_bf16(u.ptr(src), u.ptr(dst), 6, u.stream()) != 0
    u.sync()
    assert bool((dst == 0).all()), "a rejected cast launched a kernel"
