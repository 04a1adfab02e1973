"""The generator's weight EMA without a GPU: the float64 reference of tests/ema_ref.py against its closed form, the bound of
check_ema_step against a float32 emulation of the specified expression (and against three planted mistakes), the new entry points'
argument codes, and the Python surface's argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_gan_amd  # noqa: F401
from adamw_ref import f32
from ema_ref import check_ema_step, check_ema_trajectory, copies, ema_f32_emulation, ema_step, ema_trajectory

DECAYS = (0.0, 0.5, 0.999, 0.9999)


@pytest.mark.parametrize("start", [0, 1, 2, 5, 12, 20])
@pytest.mark.parametrize("decay", DECAYS)
def test_recursion_equals_its_closed_form(decay, start):
    """e_N = d^(N-k) p_k + (1 - d) sum_{j > k} d^(N-j) p_j with k = max(1, start); e_N = p_N while N <= k."""
    gen = torch.Generator().manual_seed(17 + start)
    N, n = 12, 64
    ps = [torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(N)]
    e = torch.full((n,), float("nan"), dtype=torch.float64)  # the first step must not read it
    for t in range(1, N + 1):
        e = ema_step(e, ps[t - 1], t, decay, start)
    k = max(1, start)
    if N <= k:
        want = ps[N - 1]
    else:
        want = decay ** (N - k) * ps[k - 1] + (1 - decay) * sum(decay ** (N - j) * ps[j - 1] for j in range(k + 1, N + 1))
    assert torch.allclose(e, want, rtol=1e-13, atol=1e-13), float((e - want).abs().max())
    # the trajectory helper walks the same recursion (on fp32 masters, with the decay as the kernel receives it)
    ps32 = [p.float() for p in ps]
    e32, allowed = ema_trajectory(ps32, decay, start)
    d = f32(decay)
    want32 = ps32[N - 1].double() if N <= k else d ** (N - k) * ps32[k - 1].double() + (1 - d) * sum(d ** (N - j) * ps32[j - 1].double()
                                                                                                  for j in range(k + 1, N + 1))
    assert torch.allclose(e32, want32, rtol=1e-13, atol=1e-13)
    assert bool((allowed >= 0).all()) and (N <= k) == bool((allowed == 0).all())


def _edges(n=4096, seed=3):
    """|p| and |e0| from 1e-4 to 10; differences from exactly 0 over 1e-6 |p| and 1e-3 |p| to the order of p (either sign)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.sign(torch.randn(n, generator=gen)) * 10.0 ** (torch.rand(n, generator=gen) * 5 - 4)
    rel = torch.tensor([0.0, 1e-6, 1e-3, 1.0])[torch.arange(n) % 4]
    e0 = p - p * rel * torch.randn(n, generator=gen)
    e0[n // 2::8] = 10.0 ** (torch.rand(len(e0[n // 2::8]), generator=gen) * 5 - 4)  # unrelated to p, sign included
    return e0.float(), p.float()


CASES = [(t, s) for t in (1, 2, 3, 10, 100, 10 ** 4, 10 ** 6) for s in sorted({0, max(t - 1, 0), t, t + 1})]


@pytest.mark.parametrize("decay", DECAYS)
def test_float32_form_passes_the_check_on_edge_inputs(decay):
    e0, p = _edges()
    worst = 0.0
    for t, start in CASES:
        E = torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), t, decay, start))
        worst = max(worst, check_ema_step(e0, p, t, decay, start, E, f"t={t} start={start} d={decay}"))
    print(f"\nfloat32 form, d={decay}: worst {worst:.4f} of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("decay", [0.999, 0.9999])
def test_swapped_weights_fail_the_check(decay):
    """e = e0 + d (p - e0): d and 1 - d exchanged."""
    e0, p = _edges()
    E = torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), 10, decay, 0, swap=True))
    with pytest.raises(AssertionError, match="average off"):
        check_ema_step(e0, p, 10, decay, 0, E)


@pytest.mark.parametrize("start", [3, 10])
def test_warm_up_boundary_off_by_one_fails_the_check(start):
    e0, p = _edges()
    early = lambda t, s: t <= max(1, s) - 1  # noqa: E731  (stops copying one step early: blends at t = start)
    late = lambda t, s: t <= max(1, s) + 1   # noqa: E731  (copies one step too long: copies at t = start + 1)
    E = torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), start, 0.999, start, copy_rule=early))
    with pytest.raises(AssertionError, match="must copy"):
        check_ema_step(e0, p, start, 0.999, start, E)
    E = torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), start + 1, 0.999, start, copy_rule=late))
    with pytest.raises(AssertionError, match="average off"):
        check_ema_step(e0, p, start + 1, 0.999, start, E)
    # and the right rule passes on both sides of the boundary
    for t in (start, start + 1):
        check_ema_step(e0, p, t, 0.999, start, torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), t, 0.999, start)))


@pytest.mark.parametrize("start", [0, 1])
def test_blending_on_the_first_step_fails_the_check(start):
    """Step 1 copies whatever ema_start says: a kernel that blends there depends on how the buffer was initialised."""
    e0, p = _edges()
    E = torch.from_numpy(ema_f32_emulation(e0.numpy(), p.numpy(), 1, 0.999, start, copy_rule=lambda t, s: False))
    with pytest.raises(AssertionError, match="must copy"):
        check_ema_step(e0, p, 1, 0.999, start, E)
    assert copies(1, 0) and copies(1, 1) and not copies(2, 0) and not copies(2, 1) and copies(2, 2)


def test_trajectory_check_accepts_the_float32_form_and_rejects_a_swap():
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(2048, generator=gen)
    masters = []
    for _ in range(12):
        p = (p + 5e-4 * torch.randn(2048, generator=gen)).float()
        masters.append(p)
    for start in (0, 5, 12, 30):
        for swap in (False, True):
            e = np.full(2048, np.nan, dtype=np.float32)
            for t, m in enumerate(masters, start=1):
                e = ema_f32_emulation(e, m.numpy(), t, 0.999, start, swap=swap)
            if swap and start < 12:
                with pytest.raises(AssertionError, match="average off"):
                    check_ema_trajectory(masters, 0.999, start, torch.from_numpy(e))
            else:
                assert check_ema_trajectory(masters, 0.999, start, torch.from_numpy(e)) <= 1.0


def test_entry_points_validate_their_arguments_without_a_device():
    from vit_gan_amd import _lib
    lib = _lib.lib()
    p16 = C.c_void_p(4096)  # never dereferenced: validation fails first
    hyp = (5e-4, 0.9, 0.999, 1e-8, 1e-3)

    def fused(p=p16, g=p16, m=p16, v=p16, sh=p16, ema=p16, n=1024, decay=0.999, start=0):
        return lib.vg_adamw_ema_step(p, g, m, v, sh, ema, n, *hyp, 1, None, 1.0, decay, start, None)

    for name in ("p", "g", "m", "v", "sh", "ema"):
        assert fused(**{name: None}) == -1, name
    assert fused(n=1022) == -3 and fused(n=6) == -3
    for decay in (1.0, 1.5, -0.001, float("nan")):
        assert fused(decay=decay) == -2, decay
    assert fused(start=-1) == -2
    assert lib.vg_ema_update(None, p16, 1024, 0.999, 0, 1, None, None) == -1
    assert lib.vg_ema_update(p16, None, 1024, 0.999, 0, 1, None, None) == -1
    assert lib.vg_ema_update(p16, p16, 1022, 0.999, 0, 1, None, None) == -3
    assert lib.vg_ema_update(p16, p16, 1024, 1.0, 0, 1, None, None) == -2
    assert lib.vg_ema_update(p16, p16, 1024, -0.5, 0, 1, None, None) == -2
    assert lib.vg_ema_update(p16, p16, 1024, 0.999, -1, 1, None, None) == -2
    assert lib.vg_abi_version() == _lib.ABI_VERSION  # additive exports: the ABI number stays


def test_engine_and_trainer_refuse_bad_ema_arguments_without_a_device():
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.training import train_model
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1))
    G = SirenGenerator(layers=1)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            GanEngine(D, G, batch=4, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            train_model(ema_decay=bad, save_artifacts=False)
    with pytest.raises(ValueError, match="ema_start"):
        GanEngine(D, G, batch=4, ema_decay=0.999, ema_start=-1)
    with pytest.raises(ValueError, match="ema_start"):
        train_model(ema_decay=0.999, ema_start=-1, save_artifacts=False)
    # good arguments get as far as the device check (CPU modules: no CPU fallback)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GanEngine(D, G, batch=4, ema_decay=0.999, ema_start=5)
