"""Differentiable augmentation on the GPU: the kernels (csrc/augment.hip) against the off-device restatement (tests/diffaug_ref.py),
the autograd operator, and the augmented GanEngine step against a reference step composed from the step oracle's pieces.

Error bound of the operator tests: ``assert_elementwise`` as it stands - rel |ref| + kappa 2^-24 mag with rel = 2^-8 (one bf16
rounding of the output) - with kappa = diffaug_ref.kappa(C, IH), the depth of the fp32 evaluation derived there from the reduction tree
and the operation count of the kernels as written, and mag the magnitude sum of the member-by-member composition.
tests/test_diffaug_cpu.py shows that a float32 evaluation of the restatement lies inside the same bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffaug_ref as dr
from second_order_ref import assert_elementwise

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMETRIES = [(3, 32), (3, 36), (3, 64), (3, 128), (3, 224), (1, 32)]


def _lib():
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib as L
    return L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fwd(x, policy, seed, site, step=None, want_params=True):
    L = _lib()
    B, Cc, IH, _ = x.shape
    y = torch.full_like(x, float("nan"))
    params = torch.full((B, 8), float("nan"), dtype=torch.float32, device=x.device) if want_params else None
    L.check(L.lib().vg_diffaug_fwd(_p(x), _p(y), _p(params), B, Cc, IH, policy, seed, site, _p(step), None), "vg_diffaug_fwd")
    torch.cuda.synchronize()
    return y, (None if params is None else params.cpu())


def _bwd(dy, policy, seed, site, step=None, into=None):
    L = _lib()
    B, Cc, IH, _ = dy.shape
    dx = torch.full_like(dy, float("nan")) if into is None else into.clone()
    L.check(L.lib().vg_diffaug_bwd(_p(dy), _p(dx), int(into is not None), B, Cc, IH, policy, seed, site, _p(step), None), "vg_diffaug_bwd")
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


def _reference_step(oracle, real, z, params_d, params_g, gp_epsilon=None):
    """The augmented step from the step oracle's public pieces (GanStepOracle.D / .G, the loss functions, gradient_penalty) and the
    float64 operator fed the engine's own parameters: D sees T_1([real ; fake]) - the penalty too - the generator's pass T_2(fake),
    with autograd carrying the gradient back through T_2."""
    from oracle import step_oracle as so
    from oracle.vit_oracle import vit_forward
    B = real.shape[0]
    for p in oracle.d.values():
        p.grad = None
    fake = oracle.G(z)
    pair = dr.augment(torch.cat([real, fake.detach()]), params_d)[0].float()
    loss_real = so.d_loss_real(oracle.D(pair[:B]), oracle.loss)
    loss_real.backward()
    loss_fake = so.d_loss_fake(oracle.D(pair[B:]), oracle.loss)
    loss_fake.backward()
    gp = None
    if oracle.gp_weight:
        gp = so.gradient_penalty(lambda t: vit_forward(oracle.d, t, oracle.ddims), pair[:B], pair[B:], gp_epsilon)
        (oracle.gp_weight * gp).backward()
    if oracle.clip_d is not None:
        torch.nn.utils.clip_grad_norm_(list(oracle.d.values()), max_norm=oracle.clip_d)
    oracle.opt_d.step()
    for p in oracle.g.values():
        p.grad = None
    loss_g = so.g_loss(oracle.D(dr.augment(fake, params_g)[0].float()), oracle.loss)
    total = loss_g + oracle.diversity_weight * so.diversity_loss(fake) if oracle.diversity_weight else loss_g
    total.backward()
    if oracle.clip_g is not None:
        torch.nn.utils.clip_grad_norm_(list(oracle.g.values()), max_norm=oracle.clip_g)
    oracle.opt_g.step()
    return {"d_real": float(loss_real.detach()), "d_fake": float(loss_fake.detach()), "g": float(loss_g.detach()),
            "gp": None if gp is None else float(gp.detach())}


@pytest.mark.parametrize("gp", [False, True])
def test_augmented_engine_step_matches_the_reference_step(gp):
    """losses and the first AdamW update at the tolerances of test_wasserstein_losses_and_gradient_clipping (its configuration plus the
    augmentation); with gp_weight = 10 and a fixed epsilon at those of test_engine_step_with_gradient_penalty (its configuration)"""
    from test_engine_gpu import _build
    from vit_gan_amd.engine import GanEngine
    B = 8
    D, G, oracle = _build(B, "wasserstein")
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
    ref = _reference_step(oracle, real.to(BF).float(), z, pd, pg, eps if gp else None)
    got = losses.cpu().tolist()
    print(f"augmented step (gp {gp}): engine {got} gp {float(eng.gp_loss):.5f}; reference {ref}")
    for v, k in zip(got, ("d_real", "d_fake", "g")):
        assert abs(v - ref[k]) < 2e-2, (k, got, ref)
    if gp:
        assert abs(float(eng.gp_loss) - ref["gp"]) < 0.03 * abs(ref["gp"]) + 1e-3
    k = "vit.encoder.1.fc2.weight"
    upd, ref_upd = D.state_dict()[k].detach().cpu() - w0[k], oracle.d[k].detach() - w0[k]
    assert float((upd - ref_upd).abs().max()) < 1.1e-3 and float(((upd - ref_upd).abs() < 1e-4).float().mean()) > 0.9


def test_augmented_graph_replay_equals_eager_and_draws_fresh_transforms():
    from test_engine_gpu import _bench_like, _run_steps
    B, n = 4, 3
    runs, params = {}, {}
    for name, use_graph in (("eager", False), ("graph", True)):
        eng, D, G, _ = _bench_like(B, use_graph=use_graph, diffaug=POLICY)
        g = torch.Generator().manual_seed(4)
        losses, seen = [], []
        for _ in range(n):
            real = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda()
            z = torch.randn(B, 1024, generator=g).cuda()
            losses.append(eng.step(real, z).clone())
            seen.append(torch.cat([eng.aug_params["d"], eng.aug_params["g"]]).cpu().clone())
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None and int(eng.step_t) == n
        runs[name] = (torch.stack(losses).cpu(), [t.detach().clone().cpu() for t in eng._state_tensors()])
        params[name] = seen
        for i in range(n):  # every step - every replay - has the parameters of ITS counter value, and they move
            want = np.concatenate([dr.draw(eng._aug_seed, 0, i + 1, 2 * B, 32, 7), dr.draw(eng._aug_seed, 1, i + 1, B, 32, 7)])
            assert np.array_equal(seen[i].numpy(), want), (name, i)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert torch.isfinite(runs["eager"][0]).all()
    assert torch.equal(runs["graph"][0], runs["eager"][0]), (runs["graph"][0], runs["eager"][0])
    for i, (a, b) in enumerate(zip(runs["graph"][1], runs["eager"][1])):
        assert torch.equal(a, b), f"state tensor {i} of the replayed steps differs from the eager run"
    # and the augmentation is really in the step: the plain engine takes another trajectory
    plain, _, _, _ = _bench_like(B, use_graph=False)
    assert not torch.equal(_run_steps(plain, n, B)[0], runs["eager"][0])


def test_empty_policy_is_the_plain_step():
    from test_engine_gpu import _bench_like, _run_steps
    B, n = 4, 2
    a, _, _, _ = _bench_like(B)
    b, _, _, _ = _bench_like(B, diffaug="")
    assert b.aug == 0 and not hasattr(b, "imgs_aug")
    la, sa = _run_steps(a, n, B)
    lb, sb = _run_steps(b, n, B)
    assert torch.equal(la, lb)
    for i, (u, v) in enumerate(zip(sa, sb)):
        assert torch.equal(u, v), f"state tensor {i}"
