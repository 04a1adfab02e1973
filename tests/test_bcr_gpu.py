"""Balanced consistency regularisation on the GPU: the kernel (csrc/elementwise.hip, vg_bcr_loss) against the float64 restatement
(tests/bcr_ref.py), the autograd operator, the 4B discriminator pass, and the GanEngine step with bCR against a reference step composed
from the step oracle's pieces.

Error bound of the operator tests: ``assert_elementwise`` as it stands with rel = 0 (fp32 outputs) and kappa = bcr_ref.kappa_grad() /
kappa_losses(), the depth of the fp32 evaluation counted there from the kernel as written; tests/test_bcr_cpu.py shows that a float32
emulation of the kernel's order lies inside it and that four planted mistakes do not."""
import ctypes as C

import numpy as np
import pytest
import torch

import bcr_ref as br
import diffaug_ref as dr
import engine_util as eu
import gpu_util as u
from gpu_util import GUARD
from second_order_ref import assert_elementwise
from test_bcr_cpu import SCALES, SIZES, W_FAKE, W_REAL, check, logits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PARTNER = "translation,cutout"
POLICY = "color,translation,cutout"


def _launch(lx, la, n_real, w_real, w_fake, grad_scale=1.0, into_x=None, into_a=None):
    """one vg_bcr_loss launch on guarded buffers; overwrite targets start as NaN.  Returns cpu (loss [2], gx, ga)."""
    n, Kc = lx.shape
    lxd, lad = lx.contiguous().cuda(), la.contiguous().cuda()
    nan = float("nan")
    dx = u.guarded(n * Kc, nan if into_x is None else into_x)
    da = u.guarded(n * Kc, nan if into_a is None else into_a)
    out = u.guarded(2, nan)
    u.call("vg_bcr_loss", u.ptr(lxd), u.ptr(lad), u.off(dx, GUARD), u.off(da, GUARD), u.off(out, GUARD), n_real, n - n_real, Kc, w_real, w_fake,
           int(into_x is not None), int(into_a is not None), grad_scale, None)
    torch.cuda.synchronize()
    for name, t in (("dlog_x", dx), ("dlog_a", da), ("loss_out", out)):
        u.assert_intact(t, name)
    body = lambda t, m: t[GUARD:GUARD + m].cpu()  # noqa: E731
    return body(out, 2), body(dx, n * Kc).view(n, Kc), body(da, n * Kc).view(n, Kc)


# ----------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,Kc", SIZES)
def test_kernel_matches_the_float64_restatement(B, Kc, scale):
    lx, la = logits(B, Kc, scale)
    got = _launch(lx, la, B, W_REAL, W_FAKE)
    for t in got:
        assert bool(torch.isfinite(t).all()), "an overwrite target poisoned with NaN must come back finite: every element is written"
    worst = check(got, br.consistency(lx, la, B, W_REAL, W_FAKE), Kc, f"B {B} Kc {Kc} {scale}")
    # accumulate against overwrite, with a grad_scale: the same gradient on top of what was there
    g = torch.Generator().manual_seed(B + Kc)
    old_x, old_a = torch.randn(2 * B, Kc, generator=g), torch.randn(2 * B, Kc, generator=g)
    acc = _launch(lx, la, B, W_REAL, W_FAKE, 0.5, old_x, old_a)
    worst = max(worst, check(acc, br.consistency(lx, la, B, W_REAL, W_FAKE, 0.5, old_x, old_a), Kc, "accumulating"))
    mixed = _launch(lx, la, B, W_REAL, W_FAKE, 1.0, None, old_a)  # the engine's form without diffaug: x overwritten, a accumulated
    worst = max(worst, check(mixed, br.consistency(lx, la, B, W_REAL, W_FAKE, 1.0, None, old_a), Kc, "overwrite x, accumulate a"))
    assert torch.equal(mixed[1], got[1]) and torch.equal(mixed[0], got[0])
    # a second launch gives the same bits
    again = _launch(lx, la, B, W_REAL, W_FAKE)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    print(f"vg_bcr_loss B {B} Kc {Kc} {scale}: worst fraction of the bound {worst:.3f}")


def test_unequal_segments_and_zero_weights():
    Kc = 10
    g = torch.Generator().manual_seed(3)
    lx, la = torch.randn(7 + 300, Kc, generator=g), torch.randn(7 + 300, Kc, generator=g)
    ref = br.consistency(lx, la, 7, W_REAL, W_FAKE)
    loss, gx, ga = _launch(lx, la, 7, W_REAL, W_FAKE)
    assert_elementwise(loss, ref["loss"], ref["loss_mag"], br.kappa_losses(307, 7, Kc), "loss", rel=0.0)
    assert_elementwise(gx, ref["gx"], ref["gx_mag"], br.kappa_grad(), "gx", rel=0.0)
    assert_elementwise(ga, ref["ga"], ref["ga_mag"], br.kappa_grad(), "ga", rel=0.0)
    # zero weights: exact +0 where the kernel overwrites, an untouched target where it accumulates; the losses are still reported
    old = torch.randn(307, Kc, generator=g)
    old[0, 0] = -0.0
    z_loss, z_gx, z_ga = _launch(lx, la, 7, 0.0, 0.0, 1.0, None, old)
    assert torch.equal(z_loss.view(torch.int32), loss.view(torch.int32))
    assert int((z_gx.view(torch.int32) != 0).sum()) == 0 and torch.equal(z_ga.view(torch.int32), old.view(torch.int32))
    h_loss, h_gx, h_ga = _launch(lx, la, 7, 0.0, W_FAKE)  # one segment off
    assert int((h_gx[:7].view(torch.int32) != 0).sum()) == 0 and int((h_ga[:7].view(torch.int32) != 0).sum()) == 0
    assert torch.equal(h_gx[7:], gx[7:]) and torch.equal(h_ga[7:], ga[7:]) and torch.equal(h_loss, loss)
    # non-finite logits under a zero weight still give exact zeros
    bad = lx.clone()
    bad[2, 3] = float("inf")
    _, b_gx, b_ga = _launch(bad, la, 7, 0.0, 0.0)
    assert int((b_gx.view(torch.int32) != 0).sum()) == 0 and int((b_ga.view(torch.int32) != 0).sum()) == 0


def test_autograd_operator_gives_the_kernels_gradients():
    from vit_gan_amd import ops
    B, Kc = 7, 10
    lx, la = logits(B, Kc, "unit")
    want_loss, want_gx, want_ga = _launch(lx, la, B, W_REAL, W_FAKE)
    x, a = lx.cuda().requires_grad_(True), la.cuda().requires_grad_(True)
    total, parts = ops.consistency_loss(x, a, B, W_REAL, W_FAKE)
    assert torch.equal(parts.cpu(), want_loss) and not parts.requires_grad
    assert float(total) == pytest.approx(W_REAL * float(want_loss[0]) + W_FAKE * float(want_loss[1]), rel=1e-6)
    gx, ga = torch.autograd.grad(total, (x, a))
    assert torch.equal(gx.cpu().view(torch.int32), want_gx.view(torch.int32)) and torch.equal(ga.cpu().view(torch.int32), want_ga.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ the 4B pass
def test_4b_forward_at_c2_equals_two_2b_forwards():
    """M = 4 * 256 * 65 = 66 560 token rows through vg_vit_forward: the ViT has no cross-sample operator, so without dropout the logits
    of the 4B pass are those of two 2B passes on its halves, bit for bit (grid sizes, element offsets and the CLS-row top block at
    that row count)."""
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd import _lib as L
    B = 256
    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, dropout_rate=0.0, batch_size=B)).cuda()
    vit = D.vit
    fd = vit._flat
    fd.refresh_shadow()
    d = vit._dims
    imgs = (torch.rand(4 * B, d.C, d.IH, d.IH, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(BF).cuda()
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().vg_vit_ws_bytes(C.byref(d), 4 * B), dtype=torch.uint8, device="cuda")
    assert ws.numel() > L.lib().vg_vit_ws_bytes(C.byref(d), 2 * B) > 0
    outs = {}
    for dense in (0, 1):
        net = L.VgVitNet(d, fd.flat.data_ptr(), fd.shadow.data_ptr(), fd.grad.data_ptr(), 0.0, 5, step.data_ptr(), None, 0, dense)
        whole = torch.full((4 * B, d.Kc), float("nan"), dtype=torch.float32, device="cuda")
        u.call("vg_vit_forward", C.byref(net), 4 * B, u.ptr(imgs), 1, u.ptr(ws), u.ptr(whole), None)
        halves = torch.full((4 * B, d.Kc), float("nan"), dtype=torch.float32, device="cuda")
        for h in range(2):
            u.call("vg_vit_forward", C.byref(net), 2 * B, u.ptr(imgs[2 * B * h:]), 1, u.ptr(ws), u.off(halves, 2 * B * d.Kc * h), None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(whole).all()) and float(whole.std()) > 0
        assert torch.equal(whole.view(torch.int32), halves.view(torch.int32)), f"dense_top {dense}"
        outs[dense] = whole


# ------------------------------------------------------------------------------------------------------------- the engine
def _bcr_hooks(bcr_w, params_d, params_g, params_c):
    """StepHooks of the bCR step: the float64 augmentation fed the engine's own parameters and bcr_ref's formula - the adversarial losses
    and the penalty on T_1(x) (diffaug) or x, the consistency loss between D(x) and D(T x) with gradient through both"""
    from oracle.step_oracle import StepHooks

    def consistency(oracle, real, fake, real_in, fake_in):
        n = real.shape[0]
        t_real, t_fake = (real_in, fake_in) if params_d is not None else dr.augment(torch.cat([real, fake]), params_c)[0].float().split(n)
        lx = torch.cat([oracle.D(real).reshape(n, -1), oracle.D(fake).reshape(n, -1)])
        la = torch.cat([oracle.D(t_real).reshape(n, -1), oracle.D(t_fake).reshape(n, -1)])
        return br.autograd_consistency(lx, la, n, *bcr_w)
    return StepHooks(d_inputs=None if params_d is None else (lambda real, fake: dr.augment(torch.cat([real, fake]), params_d)[0].float().split(real.shape[0])),
                     g_input=None if params_g is None else (lambda fake: dr.augment(fake, params_g)[0].float()), d_extra=consistency)


@pytest.mark.parametrize("gp", [False, True], ids=["ns", "wasserstein_gp"])
@pytest.mark.parametrize("diffaug", [True, False], ids=["diffaug", "bcr_aug"])
def test_bcr_engine_step_matches_the_reference_step(diffaug, gp):
    """adversarial losses, the penalty and the first AdamW update at the tolerances of
    test_diffaug_gpu.test_augmented_engine_step_matches_the_reference_step; the consistency losses against bcr_ref on the engine's own
    logits inside the operator bound"""
    from vit_gan_amd.engine import GanEngine
    B = 8
    bcr_w = (W_REAL, W_FAKE)
    loss = "wasserstein" if gp else "ns"
    D, G, oracle = eu.build(B, loss)
    kw = dict(diffaug=POLICY) if diffaug else dict(bcr_aug=PARTNER)
    if gp:
        oracle.gp_weight, oracle.clip_d = 10.0, 5.0
        kw.update(gp_weight=10.0, clip_d=5.0)
    eng = GanEngine(D, G, batch=B, loss=loss, external_noise=True, d_dropout=0.0, g_dropout=0.0, bcr=bcr_w, **kw)
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    z = torch.randn(B, 1024, generator=g)
    eps = torch.rand(B, 1, 1, 1, generator=g)
    if gp:
        eng.gp_epsilon = eps.cuda()
    w0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    losses = eng.step(real.cuda(), z.cuda())
    torch.cuda.synchronize()
    pd = pg = pc = None
    if diffaug:
        pd, pg = eng.aug_params["d"].cpu(), eng.aug_params["g"].cpu()
        assert np.array_equal(pd.numpy(), dr.draw(eng._aug_seed, 0, 1, 2 * B, 32, 7)) and "c" not in eng.aug_params
        assert eng.imgs_aug.data_ptr() == eng.imgs4[2 * B:].data_ptr() and eng.imgs.data_ptr() == eng.imgs4.data_ptr()
    else:
        pc = eng.aug_params["c"].cpu()
        assert np.array_equal(pc.numpy(), dr.draw(eng._aug_seed, 2, 1, 2 * B, 32, 6)), "site-2 parameters"
        for site in (0, 1):  # a stream of its own
            assert not np.array_equal(pc.numpy(), dr.draw(eng._aug_seed, site, 1, 2 * B, 32, 6))
        assert_elementwise(eng.imgs4[2 * B:], *dr.augment(eng.imgs4[:2 * B].cpu(), pc), dr.kappa(3, 32), "T_c(x) inside the step")
    assert eng.logits.shape == (4 * B, 1) and eng.imgs4.shape[0] == 4 * B
    # the consistency losses from the engine's own logits, inside the operator bound
    lg = eng.logits.cpu()
    ref_cr = br.consistency(lg[:2 * B], lg[2 * B:], B, *bcr_w)
    assert_elementwise(eng.bcr_losses, ref_cr["loss"], ref_cr["loss_mag"], br.kappa_losses(2 * B, B, 1), "bcr_losses", rel=0.0)
    assert float(eng.bcr_losses.min()) > 0
    ref = oracle.step(real.to(BF).float(), z, gp_epsilon=eps if gp else None, hooks=_bcr_hooks(bcr_w, pd, pg, pc))
    got = losses.cpu().tolist()
    print(f"bCR step (diffaug {diffaug}, gp {gp}): engine {got} cr {eng.bcr_losses.tolist()} gp {float(eng.gp_loss):.5f}; reference {ref} "
          f"cr {[float(p.detach()) for p in oracle.last_extra]} gp {oracle.last_gp}")
    eu.assert_losses_match(got, ref, 2e-2)
    if gp:
        eu.assert_penalty_matches(float(eng.gp_loss), oracle.last_gp, 0.03, 1e-3)
    eu.assert_first_update_matches(D, w0, oracle, "vit.encoder.1.fc2.weight", 1.1e-3, 1e-4, 0.9)


def _extras(eng):
    """what a bCR run records per step: the two consistency losses and the partner's parameters"""
    return ["bcr_losses", ("params", lambda e: e.aug_params["c" if e.bcr_policy else "d"])] if eng is None or eng.bcr else []


def _steps(eng, n, B, first=0):
    return eu.run_steps(eng, eu.batches(B, n, skip=first), extras=_extras(eng))


def _graph_against_eager(**extra):
    """three replays of the captured bCR step against three eager steps"""
    B, n = 4, 3

    def make(use_graph):
        eng, D, G, _ = eu.bench_like(B, use_graph=use_graph, bcr=(W_REAL, W_FAKE), bcr_aug=PARTNER, **extra)
        if eng.gp_w:  # a fixed epsilon: torch.rand's stream differs between a captured and an eager step
            eng.gp_epsilon = torch.rand(B, 1, 1, 1, generator=torch.Generator().manual_seed(2)).cuda()
        return eng
    runs, engines = eu.graph_against_eager(make, eu.batches(B, n), extras=_extras(None))
    for name, run in runs.items():
        seen = run.extras["params"]
        for i in range(n):  # every replay draws the site-2 parameters of its own counter value, and they move
            assert np.array_equal(seen[i].numpy(), dr.draw(engines[name]._aug_seed, 2, i + 1, 2 * B, 32, 6)), f"{name}: site-2 parameters of step {i + 1}"
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]), f"{name}: site-2 parameters do not move"
        engines[name].close()
    e, cr = runs["eager"], torch.stack(runs["eager"].extras["bcr_losses"])
    assert torch.isfinite(e.losses).all() and torch.isfinite(cr).all() and float(cr.min()) > 0, (e.losses, cr)
    return engines["graph"].graph_active, engines["graph"].graph_fallback_reason


def test_bcr_graph_replay_equals_eager():
    active, reason = _graph_against_eager()
    assert active and reason is None, (active, reason)


def _rccl_worker(rank, world):
    import vit_gan_amd  # noqa: F401
    return _graph_against_eager(spectral_norm="all", ema_decay=0.999, gp_weight=10.0, exchange_single_rank=True, loss="wasserstein", clip_d=5.0)


@pytest.mark.timeout(300)
def test_bcr_graph_replay_with_spectral_ema_penalty_and_exchange():
    """the same with spectral_norm="all", ema_decay, gp_weight=10 and the staged backward with its all-reduces on a one-rank RCCL group,
    all together (the group needs a process of its own, as in test_spectral_gpu)"""
    ((active, reason),) = eu.run_ranks(_rccl_worker, 1, 240, backend="nccl", gpu=True)
    assert active and reason is None, (active, reason)


def test_off_is_off_and_on_changes_the_trajectory():
    B, n = 4, 2
    plain, _, _, _ = eu.bench_like(B, diffaug=POLICY)
    off, _, _, _ = eu.bench_like(B, diffaug=POLICY, bcr=(0, 0))
    assert not off.bcr and not hasattr(off, "imgs4") and not hasattr(off, "bcr_losses") and not hasattr(off, "logits_g")
    assert off.logits.shape[0] == 2 * B and off.ws_d.numel() == plain.ws_d.numel() and "bcr" not in off.state_dict()
    a, b = _steps(plain, n, B), _steps(off, n, B)
    eu.assert_same_run(a, b, "bcr=(0, 0)")
    on, _, _, _ = eu.bench_like(B, diffaug=POLICY, bcr=(10, 10))
    assert on.logits.shape[0] == 4 * B and on.ws_d.numel() > plain.ws_d.numel()
    c = _steps(on, n, B)
    assert torch.isfinite(c.losses).all() and not torch.equal(c.state[0], a.state[0])


def test_resume_equals_the_uninterrupted_run():
    B = 4
    kw = dict(diffaug=POLICY, bcr=(W_REAL, W_FAKE), instance_noise=0.0)
    _, _, _, st, made = eu.resume_against_whole(lambda **net: eu.bench_like(B, **net, **kw), eu.batches(B, 4), 2, extras=_extras(None))
    assert tuple(st["bcr"]) == (W_REAL, W_FAKE, 0)
    b = made[2][0]
    # a state saved with other weights (or without bCR) is refused under strict, and loads without it: bCR holds no state
    for other in ((1.0, W_FAKE, 0), None):
        with pytest.raises(ValueError, match="consistency regularisation"):
            b.load_state_dict({**st, "bcr": other})
    b.load_state_dict({**st, "bcr": (1.0, 1.0, 0)}, strict=False)
    off, _, _, _ = eu.bench_like(B, diffaug=POLICY)
    with pytest.raises(ValueError, match="consistency regularisation"):
        off.load_state_dict({**off.state_dict(), "bcr": st["bcr"]})
