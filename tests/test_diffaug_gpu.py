"""Differentiable augmentation on the GPU: the kernels (csrc/augment.hip) against the off-device restatement (tests/diffaug_ref.py),
the autograd operator, and the augmented GanEngine step against a reference step composed from the step oracle's pieces.

Error bound of the operator tests: ``assert_elementwise`` as it stands - rel |ref| + kappa 2^-24 mag with rel = 2^-8 (one bf16
rounding of the output) - with kappa = diffaug_ref.kappa(C, IH), the depth of the fp32 evaluation derived there from the reduction tree
and the operation count of the kernels as written, and mag the magnitude sum of the member-by-member composition.
tests/test_diffaug_cpu.py shows that a float32 evaluation of the restatement lies inside the same bound."""
import numpy as np
import pytest
import torch

import diffaug_ref as dr
import engine_util as eu
import gpu_util as u
from second_order_ref import assert_elementwise

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMETRIES = [(3, 32), (3, 36), (3, 64), (3, 128), (3, 224), (1, 32)]


def _fwd(x, policy, seed, site, step=None, want_params=True):
    B, Cc, IH, _ = x.shape
    y = torch.full_like(x, float("nan"))
    params = torch.full((B, 8), float("nan"), dtype=torch.float32, device=x.device) if want_params else None
    u.call("vg_diffaug_fwd", u.ptr(x), u.ptr(y), u.ptr(params), B, Cc, IH, policy, seed, site, u.ptr(step), None)
    torch.cuda.synchronize()
    return y, (None if params is None else params.cpu())


def _bwd(dy, policy, seed, site, step=None, into=None):
    B, Cc, IH, _ = dy.shape
    dx = torch.full_like(dy, float("nan")) if into is None else into.clone()
    u.call("vg_diffaug_bwd", u.ptr(dy), u.ptr(dx), int(into is not None), B, Cc, IH, policy, seed, site, u.ptr(step), None)
    torch.cuda.synchronize()
    return dx


def _images(B, Cc, IH, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, Cc, IH, IH, generator=g) * 2 - 1 + offset).to(BF)


def _step(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------- parameters
def test_parameters_are_bit_exact():
    x = _images(7, 3, 32, 0).cuda()
    for seed in (1, 0xDEADBEEFCAFEF00D):
        for site in (0, 1):
            for step in (1, 2, 70000):
                _, got = _fwd(x, 7, seed, site, _step(step))
                assert np.array_equal(got.numpy(), dr.draw(seed, site, step, 7, 32, 7)), (seed, site, step)
    _, got = _fwd(x, 7, 5, 0, None)  # no device counter: the host key alone
    assert np.array_equal(got.numpy(), dr.draw(5, 0, None, 7, 32, 7))
    for B in (1, 7, 256):
        for policy, IH in ((7, 32), (5, 36), (2, 64)):
            _, got = _fwd(_images(B, 3, IH, 1).cuda(), policy, 9, 1, _step(3))
            assert np.array_equal(got.numpy(), dr.draw(9, 1, 3, B, IH, policy)), (B, policy, IH)


# --------------------------------------------------------------------------------------------------- operator and adjoint
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("Cc,IH", GEOMETRIES + [(8, 9)])  # 8 x 9 x 9: planes of 81 elements, the 2-byte access path
def test_operator_and_adjoint_match_the_float64_restatement(Cc, IH, offset):
    B = 5 if IH <= 64 else 3
    x, w = _images(B, Cc, IH, 2, offset), _images(B, Cc, IH, 3, offset)
    old = _images(B, Cc, IH, 4)
    kap = dr.kappa(Cc, IH)
    worst = {}
    for policy in range(8):
        step = _step(10 + policy)
        y, params = _fwd(x.cuda(), policy, 31, 0, step)
        assert np.array_equal(params.numpy(), dr.draw(31, 0, 10 + policy, B, IH, policy))
        ref, mag = dr.augment(x, params)
        worst["fwd"] = max(worst.get("fwd", 0.0), assert_elementwise(y, ref, mag, kap, f"forward policy {policy} {Cc}x{IH}"))
        dead = ~dr.live_mask(params, IH).expand_as(ref)
        assert int((y.cpu().view(torch.int16)[dead] != 0).sum()) == 0, "outside the frame / inside the cutout must be +0 exactly"
        if policy & 6:
            assert int(dead.sum()) > 0
        if policy == 0:
            assert torch.equal(y.cpu().view(torch.int16), x.view(torch.int16)), "policy 0 is a bitwise copy"
        dx = _bwd(w.cuda(), policy, 31, 0, step)
        aref, amag = dr.adjoint(w, params)
        worst["bwd"] = max(worst.get("bwd", 0.0), assert_elementwise(dx, aref, amag, kap, f"adjoint policy {policy} {Cc}x{IH}"))
        if policy == 0:
            assert torch.equal(dx.cpu().view(torch.int16), w.view(torch.int16))
        acc = _bwd(w.cuda(), policy, 31, 0, step, into=old.cuda())
        worst["acc"] = max(worst.get("acc", 0.0), assert_elementwise(acc, aref + old.double(), amag + old.double().abs(), kap,
                                                                     f"accumulating adjoint policy {policy} {Cc}x{IH}"))
    print(f"diffaug {Cc}x{IH}x{IH} offset {offset}: kappa {kap}, worst fraction of the bound {worst}")


@pytest.mark.parametrize("Cc,IH", [(3, 32), (3, 36), (3, 224)])
def test_same_key_gives_the_same_transform(Cc, IH):
    """<T x, w> = <x, T^T w> + <T 0, w> on the kernels' own outputs, forward and adjoint launched with equal (seed, site, step)"""
    B = 4
    x, w = _images(B, Cc, IH, 5), _images(B, Cc, IH, 6)
    zero = torch.zeros_like(x)
    step = _step(17)
    y, params = _fwd(x.cuda(), 7, 3, 1, step)
    y0, _ = _fwd(zero.cuda(), 7, 3, 1, step)
    dx = _bwd(w.cuda(), 7, 3, 1, step)
    y, y0, dx, x64, w64 = y.double().cpu(), y0.double().cpu(), dx.double().cpu(), x.double(), w.double()
    lhs = (y * w64).sum()
    rhs = (x64 * dx).sum() + (y0 * w64).sum()
    # each stored element is within rel |ref| + kappa 2^-24 mag of its exact value; the inner products inherit the sum of those
    _, mag = dr.augment(x, params)
    _, amag = dr.adjoint(w, params)
    _, mag0 = dr.augment(zero, params)
    tol = lambda v, m, o: ((2.0 ** -8 * v.abs() + dr.kappa(Cc, IH) * 2.0 ** -24 * m) * o.abs()).sum()  # noqa: E731
    bound = float(tol(y, mag, w64) + tol(dx, amag, x64) + tol(y0, mag0, w64))
    assert abs(float(lhs - rhs)) <= bound, (float(lhs), float(rhs), bound)
    print(f"adjoint identity {Cc}x{IH}: |lhs - rhs| = {abs(float(lhs - rhs)):.3e}, bound {bound:.3e}")
    _, other = _fwd(x.cuda(), 7, 3, 1, _step(18))
    assert not np.array_equal(other.numpy(), params.numpy()), "another step counter must give other parameters"


def test_launches_are_reproducible():
    for Cc, IH, B in ((3, 32, 64), (3, 224, 3)):
        x, w = _images(B, Cc, IH, 7, 3.0).cuda(), _images(B, Cc, IH, 8, 3.0).cuda()
        step = _step(4)
        a, b = _fwd(x, 7, 2, 0, step)[0], _fwd(x, 7, 2, 0, step)[0]
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        a, b = _bwd(w, 7, 2, 0, step), _bwd(w, 7, 2, 0, step)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_autograd_operator_is_the_adjoint_kernel():
    from vit_gan_amd import ops
    B, Cc, IH = 6, 3, 32
    x, w = _images(B, Cc, IH, 9).cuda().requires_grad_(True), _images(B, Cc, IH, 10).cuda()
    step = _step(5)
    y = ops.diff_augment(x, "color,translation,cutout", 12, 1, step)
    want_y, _ = _fwd(x.detach(), 7, 12, 1, step)
    assert torch.equal(y.detach().view(torch.int16), want_y.view(torch.int16))
    step_at_forward = step.clone()
    step += 1  # the backward must use the counter value of its forward
    (gx,) = torch.autograd.grad(y, x, w)
    assert torch.equal(gx.view(torch.int16), _bwd(w, 7, 12, 1, step_at_forward).view(torch.int16))
    # fp32 images go through the same kernels (cast to bf16 in, back out)
    xf = x.detach().float().requires_grad_(True)
    yf = ops.diff_augment(xf, 7, 12, 1, step_at_forward)
    assert yf.dtype == torch.float32 and torch.equal(yf.detach().to(BF).view(torch.int16), want_y.view(torch.int16))
    (gf,) = torch.autograd.grad(yf, xf, w.float())
    assert gf.dtype == torch.float32 and torch.equal(gf.to(BF).view(torch.int16), gx.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------- the engine
POLICY = "color,translation,cutout"


def _augmented(params_d, params_g):
    """StepHooks of the augmented step: the float64 operator fed the engine's own parameters - D sees T_1([real ; fake]), the penalty
    too, the generator's pass T_2(fake), with autograd carrying the gradient back through T_2"""
    from oracle.step_oracle import StepHooks
    return StepHooks(d_inputs=lambda real, fake: dr.augment(torch.cat([real, fake]), params_d)[0].float().split(real.shape[0]),
                     g_input=lambda fake: dr.augment(fake, params_g)[0].float())


@pytest.mark.parametrize("gp", [False, True])
def test_augmented_engine_step_matches_the_reference_step(gp):
    """losses and the first AdamW update at the tolerances of test_wasserstein_losses_and_gradient_clipping (its configuration plus the
    augmentation); with gp_weight = 10 and a fixed epsilon at those of test_engine_step_with_gradient_penalty (its configuration)"""
    from vit_gan_amd.engine import GanEngine
    B = 8
    D, G, oracle = eu.build(B, "wasserstein")
    if gp:
        oracle.gp_weight, oracle.clip_d = 10.0, 5.0
        eng = GanEngine(D, G, batch=B, loss="wasserstein", gp_weight=10.0, clip_d=5.0, external_noise=True, d_dropout=0.0, g_dropout=0.0,
                        diffaug=POLICY)
    else:
        oracle.clip_d, oracle.clip_g, oracle.diversity_weight = 0.05, 0.02, 0.1
        eng = GanEngine(D, G, batch=B, loss="wasserstein", clip_d=0.05, clip_g=0.02, diversity_weight=0.1, external_noise=True,
                        d_dropout=0.0, g_dropout=0.0, diffaug=POLICY)
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    z = torch.randn(B, 1024, generator=g)
    eps = torch.rand(B, 1, 1, 1, generator=g)
    if gp:
        eng.gp_epsilon = eps.cuda()
    w0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    losses = eng.step(real.cuda(), z.cuda())
    torch.cuda.synchronize()
    pd, pg = eng.aug_params["d"].cpu(), eng.aug_params["g"].cpu()
    assert np.array_equal(pd.numpy(), dr.draw(eng._aug_seed, 0, 1, 2 * B, 32, 7)) and np.array_equal(pg.numpy(), dr.draw(eng._aug_seed, 1, 1, B, 32, 7))
    assert not np.array_equal(pd[:B].numpy(), pd[B:].numpy()) and not np.array_equal(pd[B:].numpy(), pg.numpy())  # real, fake, T_2: own draws
    # what D was fed in the generator's pass is T_2 of the engine's own fake
    assert_elementwise(eng.imgs_aug[:B], *dr.augment(eng.imgs[B:].cpu(), pg), dr.kappa(3, 32), "T_2(fake) inside the step")
    ref = oracle.step(real.to(BF).float(), z, gp_epsilon=eps if gp else None, hooks=_augmented(pd, pg))
    got = losses.cpu().tolist()
    print(f"augmented step (gp {gp}): engine {got} gp {float(eng.gp_loss):.5f}; reference {ref} gp {oracle.last_gp}")
    eu.assert_losses_match(got, ref, 2e-2)
    if gp:
        eu.assert_penalty_matches(float(eng.gp_loss), oracle.last_gp, 0.03, 1e-3)
    eu.assert_first_update_matches(D, w0, oracle, "vit.encoder.1.fc2.weight", 1.1e-3, 1e-4, 0.9)


def test_augmented_graph_replay_equals_eager_and_draws_fresh_transforms():
    B, n = 4, 3
    runs, made = eu.graph_against_eager(lambda use_graph: eu.bench_like(B, use_graph=use_graph, diffaug=POLICY), eu.batches(B, n),
                                        extras=[("params", lambda e: torch.cat([e.aug_params["d"], e.aug_params["g"]]))])
    for name, run in runs.items():
        eng, seen = made[name][0], run.extras["params"]
        for i in range(n):  # every step - every replay - has the parameters of ITS counter value, and they move
            want = np.concatenate([dr.draw(eng._aug_seed, 0, i + 1, 2 * B, 32, 7), dr.draw(eng._aug_seed, 1, i + 1, B, 32, 7)])
            assert np.array_equal(seen[i].numpy(), want), (name, i)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert torch.isfinite(runs["eager"].losses).all()
    # and the augmentation is really in the step: the plain engine takes another trajectory
    plain, _, _, _ = eu.bench_like(B, use_graph=False)
    assert not torch.equal(eu.run_steps(plain, eu.batches(B, n)).losses, runs["eager"].losses)


def test_empty_policy_is_the_plain_step():
    B, n = 4, 2
    a, _, _, _ = eu.bench_like(B)
    b, _, _, _ = eu.bench_like(B, diffaug="")
    assert b.aug == 0 and not hasattr(b, "imgs_aug")
    eu.assert_same_run(eu.run_steps(a, eu.batches(B, n)), eu.run_steps(b, eu.batches(B, n)), "diffaug=''")
