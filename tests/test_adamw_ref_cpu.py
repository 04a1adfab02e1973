"""The fp64 AdamW reference (tests/adamw_ref.py) against torch.optim.AdamW(foreach=False) in float64, on injected states."""
import pytest
import torch

from adamw_ref import adamw_step, bias_correction, f32


def _state(n, seed):
    """Per-element edges: zero gradients, |g| ~ 1e-6, ~1, ~1e3; moments carried over from earlier steps; |p| from 1e-4 to 10."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.float64
    p = torch.sign(torch.randn(n, generator=gen, dtype=d)) * 10.0 ** (torch.rand(n, generator=gen, dtype=d) * 5 - 4)
    scale = torch.tensor([0.0, 1e-6, 1.0, 1e3], dtype=d)[torch.arange(n) % 4]
    g = torch.randn(n, generator=gen, dtype=d) * scale
    h = torch.tensor([1.0, 1e-6, 1e3, 0.0], dtype=d)[torch.randperm(n, generator=gen) % 4]  # history scale, not tied to g's
    m = torch.randn(n, generator=gen, dtype=d) * h
    v = (torch.randn(n, generator=gen, dtype=d) * h) ** 2
    return p, m, v, g


@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 10 ** 6])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("fp32_hyper", [False, True])
def test_reference_matches_torch_adamw_in_float64(t, betas, wd, fp32_hyper):
    cvt = f32 if fp32_hyper else float
    lr, b1, b2, eps, wd = cvt(5e-4), cvt(betas[0]), cvt(betas[1]), cvt(1e-8), cvt(wd)
    p0, m0, v0, g = _state(4 * 257, seed=t)
    for gscale in (1.0, 0.5, 0.125):
        param = torch.nn.Parameter(p0.clone())
        param.grad = g * gscale
        opt = torch.optim.AdamW([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        opt.state[param] = {"step": torch.tensor(float(t - 1), dtype=torch.float64), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        opt.step()
        st = opt.state[param]
        assert float(st["step"]) == t
        p1, m1, v1 = adamw_step(p0, m0, v0, g, t, lr, b1, b2, eps, wd, gscale)
        gg = g * gscale
        # per element, relative to the magnitude of the terms that form each value (m's two terms may cancel)
        for what, got, ref, scale in (("p", p1, param.detach(), p0.abs()),
                                      ("m", m1, st["exp_avg"], b1 * m0.abs() + (1 - b1) * gg.abs()),
                                      ("v", v1, st["exp_avg_sq"], v1.abs())):
            err = (got - ref).abs()
            bad = err > 1e-12 * scale
            assert not bool(bad.any()), (what, t, gscale, float(err.max()), int(bad.sum()))
        # the update itself (what moves the weight), well above the 1e-12 * |p| rounding of p
        upd, upd_ref = p1 - p0 * (1 - lr * wd), param.detach() - p0 * (1 - lr * wd)
        assert float((upd - upd_ref).abs().max()) <= 1e-12 * float(upd_ref.abs().max()) + 1e-15 * float(p0.abs().max())


def test_bias_correction_does_not_cancel():
    b2 = f32(0.999)
    assert bias_correction(b2, 1) == 1.0 - b2  # exact: 1 - b is exact in float64 for b in [0.5, 1]
    for t in (2, 3, 10, 1000):
        want = 1.0 - b2 ** t
        assert abs(bias_correction(b2, t) - want) <= 1e-13 * want
    assert bias_correction(b2, 10 ** 6) == 1.0
    assert bias_correction(f32(0.9), 1) == 1.0 - f32(0.9)
