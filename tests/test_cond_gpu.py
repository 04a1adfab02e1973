"""Class conditioning on the GPU: the five kernels against the off-device restatement (tests/cond_ref.py) bit for bit, the
conditional generator against the oracle's extended-latent form, the conditional GanEngine step against a CPU reference step built
from the step oracle's pieces, hipGraph replay against eager, every option it combines with, resume, and the trainer."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import cond_ref as cr
import engine_util as eu
import gpu_util as u
from gpu_util import GUARD

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SEED = 0x1234ABCD5678EF01
K3 = 3


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("K", [1, 3, 10, 16])
def test_draw_labels_equals_the_restatement(K):
    from vit_gan_amd import ops
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    for n in (1, 67, 1024):
        buf = u.guarded(n, -1, torch.int32)
        u.call("vg_draw_labels", u.off(buf, GUARD), n, K, SEED, 3, u.ptr(step), None)
        torch.cuda.synchronize()
        u.assert_intact(buf, "labels")
        assert np.array_equal(buf[GUARD:GUARD + n].cpu().numpy(), cr.draw_labels(n, K, SEED, 3, 5)), (n, K)
        assert np.array_equal(ops.draw_labels(n, K, SEED, 3, step).cpu().numpy(), cr.draw_labels(n, K, SEED, 3, 5))
        assert np.array_equal(ops.draw_labels(n, K, SEED, 2, None).cpu().numpy(), cr.draw_labels(n, K, SEED, 2, None)), "no device counter"


def _label_sets(B, g):
    """(name, labels) at K = 3: a class that never occurs (1) and a class that takes every row"""
    return (("class 1 absent", torch.randint(0, 2, (B,), generator=g) * 2), ("class 1 everywhere", torch.ones(B, dtype=torch.int64)))


@pytest.mark.parametrize("N", [8, 520, 12288])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_class_add_equals_the_restatement(B, N):
    from vit_gan_amd import ops
    g = torch.Generator().manual_seed(B * 100003 + N)
    w = (torch.randn(B, N, generator=g) * 2).to(BF)
    table = (torch.rand(K3, N, generator=g) * 2 - 1).to(BF)
    for name, y in _label_sets(B, g):
        buf = u.guarded(B * N, w, BF)
        td, yd = table.cuda(), y.to(torch.int32).cuda()
        u.call("vg_class_add", u.off(buf, GUARD), u.ptr(td), u.ptr(yd), B, N, K3, None)
        torch.cuda.synchronize()
        u.assert_intact(buf, "wmod")
        want = cr.class_add(cr.bits_of(w), cr.bits_of(table), y.numpy())
        assert np.array_equal(cr.bits_of(buf[GUARD:GUARD + B * N]).reshape(B, N), want), (name, B, N)
        assert np.array_equal(cr.bits_of(ops.class_add(w.cuda(), td, y.cuda())), want), "ops.class_add"


@pytest.mark.parametrize("N", [8, 520, 12288])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_class_grad_equals_the_restatement(B, N):
    from vit_gan_amd import ops
    g = torch.Generator().manual_seed(B * 7919 + N)
    dw = torch.randn(B, N, generator=g)
    old = torch.randn(K3, N, generator=g)
    old[1, 0] = -0.0
    dwd = dw.cuda()
    for name, y in _label_sets(B, g):
        yd = y.to(torch.int32).cuda()
        for accumulate in (0, 1):
            buf = u.guarded(K3 * N, float("nan") if not accumulate else old)
            u.call("vg_class_grad", u.ptr(dwd), u.ptr(yd), u.off(buf, GUARD), B, N, K3, accumulate, None)
            torch.cuda.synchronize()
            u.assert_intact(buf, "dtable")
            got = buf[GUARD:GUARD + K3 * N].cpu().view(K3, N)
            want = cr.class_grad(dw.numpy(), y.numpy(), K3, into=old.numpy() if accumulate else None)
            assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (name, B, N, accumulate)
            for k in set(range(K3)) - set(y.tolist()):  # a class with no sample: +0 overwritten, untouched accumulated
                if accumulate:
                    assert torch.equal(_i32(got[k]), _i32(old[k])), (name, k)
                else:
                    assert int((_i32(got[k]) != 0).sum()) == 0, (name, k)
        # the rows summed over k are the column sums of dw (another order: not bitwise)
        tab = ops.class_grad(dwd, y.cuda(), K3)
        col = torch.empty(N, dtype=torch.float32, device="cuda")
        u.call("vg_colsum_f32", u.ptr(dwd), B, N, u.ptr(col), N, None, 0, None, 0, None, 0, 0, None)
        torch.cuda.synchronize()
        err, scale = float((tab.double().sum(0) - col.double()).abs().max()), float(col.abs().max())
        assert err <= 1e-6 * scale, f"{name}: sum over classes {err:.3e} off the column sums, max {scale:.3e}"
        acc = ops.class_grad(dwd, y.cuda(), K3, out=old.clone().cuda())
        assert torch.equal(_i32(acc), torch.from_numpy(cr.class_grad(dw.numpy(), y.numpy(), K3, into=old.numpy())).view(torch.int32))


def _cond_launch(lg, y, kind, role, grad_scale=1.0, selected=True):
    """one vg_gan_loss_cond launch on guarded buffers whose bodies start as NaN: cpu (loss [1], dlogits [n, Kc], selected [n])"""
    n, Kc = lg.shape
    nan = float("nan")
    dl, sel, out = u.guarded(n * Kc, nan), u.guarded(n, nan), u.guarded(1, nan)
    u.call("vg_gan_loss_cond", u.ptr(lg), u.ptr(y), u.off(dl, GUARD), u.off(sel, GUARD) if selected else None, u.off(out, GUARD), n, Kc, kind, role, grad_scale, None)
    torch.cuda.synchronize()
    for name, t in (("dlogits", dl), ("selected", sel), ("loss_out", out)):
        u.assert_intact(t, name)
    return out[GUARD:GUARD + 1].cpu(), dl[GUARD:GUARD + n * Kc].cpu().view(n, Kc), sel[GUARD:GUARD + n].cpu()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n,Kc", [(1, 1), (8, 3), (67, 10), (600, 16)])
def test_cond_loss_equals_the_plain_loss_on_the_gathered_logits(n, Kc, kind):
    g = torch.Generator().manual_seed(n * 31 + Kc)
    lg = (torch.randn(n, Kc, generator=g) * 2).cuda()
    y = torch.randint(0, Kc, (n,), generator=g).to(torch.int32).cuda()
    s = lg.gather(1, y.long().reshape(-1, 1)).reshape(-1).contiguous()  # gathered on the host side of the call
    picked = torch.zeros(n, Kc, dtype=torch.bool).scatter_(1, y.cpu().long().reshape(-1, 1), True)
    singles = {}
    for role in (0, 1, 2):
        for gs in (1.0, 0.5):
            loss, dl, sel = _cond_launch(lg, y, kind, role, gs)
            ref_d, ref_l = torch.full((n,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
            u.call("vg_gan_loss", u.ptr(s), u.ptr(ref_d), u.ptr(ref_l), n, kind, role, gs, None)
            torch.cuda.synchronize()
            assert torch.equal(_i32(loss), _i32(ref_l)), (role, gs, loss, ref_l)
            assert torch.equal(_i32(dl[picked]), _i32(ref_d)), "the selected gradients"
            assert int((_i32(dl[~picked]) != 0).sum()) == 0, "every other gradient is +0 exactly"
            assert torch.equal(_i32(sel), _i32(s)), "selected is the gather"
            if gs == 1.0:
                singles[role] = (loss, dl)
            # against the float64 restatement: fp32 round-off of n terms
            l64, d64, _ = cr.cond_loss64(lg.cpu().numpy(), y.cpu().numpy(), kind, role, gs)
            assert abs(float(loss) - l64) <= 2.0 ** -20 * (1.0 + float(lg.abs().max()))
            np.testing.assert_allclose(dl.numpy(), d64, rtol=2.0 ** -18, atol=2.0 ** -20 * gs / n)
    assert torch.equal(_cond_launch(lg, y, kind, 0, 1.0, selected=False)[1], singles[0][1]), "selected is nullable"
    # the pair form: one launch, two segments, bit-equal to two single calls
    if n >= 2:
        n0 = n // 3 + 1
        nan = float("nan")
        dl, sel, out = u.guarded(n * Kc, nan), u.guarded(n, nan), u.guarded(2, nan)
        u.call("vg_gan_loss_cond_pair", u.ptr(lg), u.ptr(y), u.off(dl, GUARD), u.off(sel, GUARD), u.off(out, GUARD), n0, 0, n - n0, 1, Kc, kind, 1.0, None)
        torch.cuda.synchronize()
        for name, t in (("dlogits", dl), ("selected", sel), ("loss_out", out)):
            u.assert_intact(t, name)
        a = _cond_launch(lg[:n0].contiguous(), y[:n0].contiguous(), kind, 0)
        b = _cond_launch(lg[n0:].contiguous(), y[n0:].contiguous(), kind, 1)
        assert torch.equal(_i32(out[GUARD:GUARD + 2]), _i32(torch.cat([a[0], b[0]])))
        assert torch.equal(_i32(dl[GUARD:GUARD + n * Kc]), _i32(torch.cat([a[1], b[1]]).reshape(-1)))
        assert torch.equal(_i32(sel[GUARD:GUARD + n]), _i32(torch.cat([a[2], b[2]])))


def test_labels_out_of_range_are_clamped_inside_every_kernel():
    """labels written straight into the buffers (ops would refuse them): finite results, the clamped label's, and no guard touched"""
    from vit_gan_amd import ops
    B, N, Kc = 6, 520, 3
    bad = torch.tensor([-1, 3, 2 ** 31 - 1, -2 ** 31, 1, 1000], dtype=torch.int32)
    good = bad.clamp(0, Kc - 1)
    g = torch.Generator().manual_seed(9)
    lg = torch.randn(B, Kc, generator=g).cuda()
    for role in (0, 1, 2):
        got, want = _cond_launch(lg, bad.cuda(), 0, role), _cond_launch(lg, good.cuda(), 0, role)
        for a, b in zip(got, want):
            assert bool(torch.isfinite(a).all()) and torch.equal(_i32(a), _i32(b))
    w, table, dw = (torch.randn(B, N, generator=g)).to(BF), torch.randn(Kc, N, generator=g).to(BF), torch.randn(B, N, generator=g)
    buf = u.guarded(B * N, w, BF)
    td, yd, dwd = table.cuda(), bad.cuda(), dw.cuda()  # (held: a temporary's block could be handed out again before the launch)
    u.call("vg_class_add", u.off(buf, GUARD), u.ptr(td), u.ptr(yd), B, N, Kc, None)
    tab = u.guarded(Kc * N, float("nan"))
    u.call("vg_class_grad", u.ptr(dwd), u.ptr(yd), u.off(tab, GUARD), B, N, Kc, 0, None)
    torch.cuda.synchronize()
    u.assert_intact(buf, "wmod")
    u.assert_intact(tab, "dtable")
    assert np.array_equal(cr.bits_of(buf[GUARD:GUARD + B * N]).reshape(B, N), cr.class_add(cr.bits_of(w), cr.bits_of(table), good.numpy()))
    assert np.array_equal(tab[GUARD:GUARD + Kc * N].cpu().numpy().reshape(Kc, N), cr.class_grad(dw.numpy(), good.numpy(), Kc))
    for fn in (lambda: ops.conditional_gan_loss(lg, bad.cuda()), lambda: ops.class_add(w.cuda(), table.cuda(), bad.cuda()),
               lambda: ops.class_grad(dw.cuda(), bad.cuda(), Kc), lambda: ops.conditional_gan_loss(lg, good.float().cuda())):
        with pytest.raises(ValueError, match="labels"):
            fn()


def test_autograd_operator_gives_the_kernels_gradients():
    from vit_gan_amd import ops
    g = torch.Generator().manual_seed(2)
    lg = torch.randn(8, 3, generator=g).cuda()
    y = torch.randint(0, 3, (8,), generator=g).cuda()  # int64, as a data loader hands them over
    for kind, name in enumerate(cr.KINDS):
        for role, rname in enumerate(("d_real", "d_fake", "g")):
            want = _cond_launch(lg, y.to(torch.int32), kind, role)
            x = lg.clone().requires_grad_(True)
            loss, sel = ops.conditional_gan_loss(x, y, name, rname, return_selected=True)
            (gx,) = torch.autograd.grad(2.0 * loss, x)
            assert torch.equal(_i32(loss.detach().reshape(1)), _i32(want[0])) and torch.equal(_i32(sel), _i32(want[2])) and not sel.requires_grad
            assert torch.equal(gx.cpu(), 2.0 * want[1])


# -------------------------------------------------------------------------------------------------------------------- generator
GEN_KW = dict(latent=256, image_size=32, channels=3, embed=384, heads=4, layers=2, siren_hidden=256, dropout=0.0, patch_size=4)
GEN_LABELS = [0, 0, 2, 2, 2, 0]  # class 1 is absent


@functools.lru_cache(maxsize=None)
def _gen_reference():
    """the oracle generator in its extended-latent form, once: state, table, z, image, cotangent and every gradient (cpu, fp32)"""
    from oracle import gen_oracle as go
    from weights import make_input
    d = go.GenDims(latent=256, tokens=64, embed=384, heads=4, layers=2, siren_hidden=256, channels=3, image=32, patch=4)
    st0 = go.init_gen_state(d, seed=11)
    g = torch.Generator().manual_seed(12)
    table = (torch.rand(K3, d.tokens * d.embed, generator=g) * 2 - 1) / 16  # U(+-1/sqrt(latent))
    B = len(GEN_LABELS)
    z = torch.from_numpy(make_input((B, d.latent), 5))
    st = {k: v.clone().requires_grad_(True) for k, v in cr.extended_state(st0, table).items()}
    out = go.gen_forward(st, cr.extended_latent(z, GEN_LABELS, K3), d)
    R = torch.from_numpy(make_input(tuple(out.shape), 6)).to(BF).float()
    (out * R).sum().backward()
    grads = {k: v.grad.clone() for k, v in st.items()}
    wext = grads.pop("mapping_mlp.model.0.0.weight")
    grads["mapping_mlp.model.0.0.weight"] = wext[:, :d.latent].contiguous()
    grads["class_embedding.weight"] = wext[:, d.latent:].t().contiguous()
    return st0, table, z, out.detach(), R, grads


def test_conditional_generator_vs_the_extended_latent_oracle():
    import gpu_util as u
    from vit_gan_amd.generator import SirenGenerator
    st0, table, z, out, R, grads = _gen_reference()
    G = SirenGenerator(n_classes=K3, **GEN_KW)
    G.load_state_dict({**st0, "class_embedding.weight": table}, strict=True)
    G = G.cuda().eval()
    y = torch.tensor(GEN_LABELS, device="cuda")
    img = G(z.cuda(), y)
    u.assert_close(img, out, 0.08, "generated image")
    G.zero_grad()
    img.backward(R.cuda())
    torch.cuda.synchronize()
    got = {k: p.grad.detach().cpu() for k, p in G.named_parameters()}
    assert set(got) == set(grads)
    for k, ref in grads.items():
        # the tolerances of test_net_gpu.test_gen_forward_backward_vs_oracle; the table takes the mapping bias's
        tol = 0.35 if k.endswith(("gamma", "beta")) else 0.12
        u.assert_close(got[k], ref.reshape(got[k].shape), tol, f"grad {k}", floor=1e-4)
    tg = got["class_embedding.weight"]
    assert int((_i32(tg[1]) != 0).sum()) == 0 and float(grads["class_embedding.weight"][1].abs().max()) == 0.0, "class 1 has no sample"
    assert float(tg[0].abs().max()) > 0 and float(tg[2].abs().max()) > 0
    # labels are required exactly for a conditional generator, and checked
    with pytest.raises(ValueError, match="labels"):
        G(z.cuda())
    with pytest.raises(ValueError, match="labels"):
        G(z.cuda(), torch.full((len(GEN_LABELS),), K3, device="cuda"))


def test_zero_table_is_the_unconditional_generator_bit_for_bit():
    from vit_gan_amd.generator import SirenGenerator
    st0, table, z, _, _, _ = _gen_reference()
    G0 = SirenGenerator(**GEN_KW)
    G0.load_state_dict(st0, strict=True)
    G3 = SirenGenerator(n_classes=K3, **GEN_KW)
    G3.load_state_dict({**st0, "class_embedding.weight": torch.zeros_like(table)}, strict=True)
    G0, G3 = G0.cuda().eval(), G3.cuda().eval()
    y = torch.tensor(GEN_LABELS, device="cuda")
    with torch.no_grad():
        a, b = G0(z.cuda()), G3(z.cuda(), y)
        assert torch.equal(a, b)
        G3.class_embedding.weight.copy_(table.cuda())
        c = G3(z.cuda(), y)
    assert not torch.equal(a, c) and bool(torch.isfinite(c).all())
    with pytest.raises(ValueError, match="labels"):
        G0(z.cuda(), y)


# ----------------------------------------------------------------------------------------------------------------------- engine
B8 = 8
G16 = eu.COND_G


def _nets(n_classes=K3, Kc=K3, d_drop=0.0, g_drop=0.0, seed=3):
    """D: E = 128, H = 4, L = 2, 16 x 16 images, patch 4, Kc logits; G: two SLN blocks on 16 row tokens"""
    assert (d_drop, g_drop) in ((0.0, 0.0), (0.1, 0.2))
    return eu.build_nets(B8, seed, dropout=d_drop > 0, cond=(n_classes, Kc))


def _engine(n_classes=K3, Kc=K3, train=True, seed=3, **kw):
    from vit_gan_amd.engine import GanEngine
    D, G = _nets(n_classes, Kc, 0.1 if train else 0.0, 0.2 if train else 0.0, seed)
    D, G = (D.train(), G.train()) if train else (D.eval(), G.eval())
    opts = dict(batch=B8, seed=77, n_classes=n_classes)
    opts.update(kw)
    return GanEngine(D.cuda(), G.cuda(), **opts), D, G


def _data(n):
    return eu.batches(B8, n, image=16, latent=0, labels=K3)


def _run(eng, data):
    """the steps on ``data``, with the fake labels and the selected logits of every step"""
    if eng.cond:
        return eu.run_steps(eng, data, extras=("fake_labels", "selected"), step=lambda e, b: e.step(b[0], labels=b[1]))
    return eu.run_steps(eng, data, step=lambda e, b: e.step(b[0]))


def _finite(run, what):
    assert bool(torch.isfinite(run.losses).all()), (what, run.losses)
    for i, t in enumerate(run.state):
        assert bool(torch.isfinite(t.float()).all()), f"{what}: state tensor {i}"


def _label_selected(loss, y_real, y_fake):
    """StepHooks of the conditional step: the label-selected losses on D's K-way head"""
    from oracle.step_oracle import StepHooks
    return StepHooks(losses=tuple((lambda t, y=y, role=role: cr.torch_cond_loss(t.reshape(len(y), -1), y, loss, role))
                                  for role, y in enumerate((y_real, y_fake, y_fake))))


@pytest.mark.parametrize("loss,fuse", [("ns", True), ("hinge", False)])
def test_conditional_step_matches_the_reference_step(loss, fuse):
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo
    eng, D, G = _engine(train=False, loss=loss, external_noise=True, fuse_real_fake=fuse)
    d = D.vit._dims
    ddims = vo.VitDims(channels=d.C, image=d.IH, patch=d.P, embed=d.E, heads=d.H, layers=d.L, mlp_ratio=d.R, classes=d.Kc)
    gdims = go.GenDims(latent=256, tokens=16, embed=384, heads=4, layers=2, siren_hidden=256, channels=3, image=16)
    d0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    g0 = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    table0 = g0.pop("class_embedding.weight")
    oracle = so.GanStepOracle(d0, cr.extended_state(g0, table0), ddims, gdims, loss=loss)
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B8, 3, 16, 16, generator=g) * 2 - 1
    z = torch.randn(B8, 256, generator=g)
    y_real, y_fake = torch.randint(0, K3, (B8,), generator=g), torch.tensor([0, 2, 2, 0, 0, 2, 0, 2])  # no fake of class 1
    losses = eng.step(real.cuda(), z.cuda(), y_real.cuda(), y_fake.cuda())
    torch.cuda.synchronize()
    assert torch.equal(eng.real_labels.cpu(), y_real.int()) and torch.equal(eng.fake_labels.cpu(), y_fake.int())
    # the generator in its extended-latent form (its AdamW is elementwise, so the update of [W | table^T] is the update of W and of the table)
    ref = oracle.step(real.to(BF).float(), cr.extended_latent(z, y_fake, K3), hooks=_label_selected(loss, y_real, y_fake))
    got = losses.cpu().tolist()
    print(f"conditional step ({loss}, fused {fuse}): engine {got}; reference {ref}")
    eu.assert_losses_match(got, ref, 2e-2)
    # selected = the gather of D's own logits; the other logits carry +0.  (Rows [0, B) of logits / dlogits were reused by the
    # generator's pass, which reads the fake labels too; rows [B, 2B) still hold the fake half of D's own pass.)
    lg, y2 = eng.logits.cpu(), torch.cat([y_fake, y_fake]).reshape(-1, 1)
    assert torch.equal(eng.selected.cpu()[B8:], lg[B8:].gather(1, y2[B8:]).reshape(-1))
    picked = torch.zeros(2 * B8, K3, dtype=torch.bool).scatter_(1, y2, True)
    assert int((_i32(eng.dlogits.cpu()[~picked]) != 0).sum()) == 0
    # the first AdamW update, at the tolerances of test_bcr_gpu.test_bcr_engine_step_matches_the_reference_step
    eu.assert_first_update_matches(D, d0, oracle, "vit.encoder.1.fc2.weight", 1.1e-3, 1e-4, 0.9)
    # the table: the first AdamW step is lr sign(g), so an element whose gradient lies under the generator's gradient tolerance (0.12 of
    # max|g|, test_net_gpu) may take the other sign - 2 lr = 1e-3 off; every element above it moves as the reference's does
    upd = G.class_embedding.weight.detach().cpu() - table0
    wext = oracle.g["mapping_mlp.model.0.0.weight"]
    ref_upd, ref_g = wext.detach()[:, 256:].t() - table0, wext.grad[:, 256:].t()
    clear = ref_g.abs() > 0.12 * float(ref_g.abs().max())
    assert float((upd - ref_upd).abs().max()) < 1.1e-3 and int(clear.sum()) > 0 and float((upd - ref_upd)[clear].abs().max()) < 1e-4
    assert float(upd[1].abs().max()) < 1e-6, "class 1 had no fake sample: weight decay only"
    assert float(upd[0].abs().max()) > 1e-4 and float(upd[2].abs().max()) > 1e-4
    eng.close()


def _graph_against_eager(n, **kw):
    runs, engines = eu.graph_against_eager(lambda use_graph: _engine(use_graph=use_graph, **kw), _data(n), "graph against eager",
                                           extras=("fake_labels", "selected"), step=lambda e, b: e.step(b[0], labels=b[1]))
    _finite(runs["eager"], "eager")
    return runs, engines


def test_six_steps_of_graph_replay_equal_eager_and_draw_fresh_labels():
    runs, engines = _graph_against_eager(6)
    eng = engines["graph"][0]
    for name in ("eager", "graph"):
        fakes = runs[name].extras["fake_labels"]
        for i, f in enumerate(fakes):  # drawn in front of step i + 1, when the device counter still holds i
            assert np.array_equal(f.numpy(), cr.draw_labels(B8, K3, eng._aug_seed, cr.LABEL_SITE, i)), (name, i)
        assert len({tuple(f.tolist()) for f in fakes}) > 1, "the fake labels move between replays"
    for e, _, _ in engines.values():
        e.close()


@pytest.mark.parametrize("name,kw", [("diffaug_ada", dict(diffaug="color,translation,cutout", ada_target=0.6, ada_interval=1, aug_p=0.3)),
                                      ("bcr", dict(bcr=(10.0, 10.0), bcr_aug="translation,cutout")),
                                      ("ema", dict(ema_decay=0.9)),
                                      ("spectral_qkv", dict(spectral_norm="qkv")),
                                      ("unfused", dict(fuse_real_fake=False)),
                                      ("exchange_off_hinge", dict(loss="hinge", clip_d=5.0, clip_g=0.5))])
def test_conditional_step_with_each_option(name, kw):
    runs, engines = _graph_against_eager(3, **kw)
    eng, D, G = engines["graph"]
    if name == "diffaug_ada":  # the controller fires every step on the B selected real logits of that step
        sel = runs["graph"].extras["selected"][-1][:B8]
        assert eng.ada_rt == pytest.approx(float(torch.sign(sel).mean()), abs=1e-6), (eng.ada_rt, sel)
        assert 0.0 <= eng.ada_p <= 1.0
    if name == "bcr":
        assert bool(torch.isfinite(eng.bcr_losses).all()) and float(eng.bcr_losses.min()) > 0 and eng.logits.shape == (4 * B8, K3)
    if name == "ema":
        from vit_gan_amd.generator import SirenGenerator
        g = torch.Generator().manual_seed(1)
        z, y = torch.randn(5, 256, generator=g).cuda(), torch.tensor([0, 1, 2, 1, 0]).cuda()
        Ge = SirenGenerator(dropout=0.0, n_classes=K3, **G16)
        sd = eng.ema_state_dict()
        assert "class_embedding.weight" in sd
        Ge.load_state_dict(sd, strict=True)
        with torch.no_grad():
            want = Ge.cuda().eval()(z, y)
        assert torch.equal(eng.sample(z, y), want) and not torch.equal(eng.sample(z, y), eng.sample(z, y, ema=False))
        with pytest.raises(ValueError, match="labels"):
            eng.sample(z)
    for e, _, _ in engines.values():
        e.close()


def test_resume_through_state_dict_and_class_count_mismatch():
    _, _, _, sd, made = eu.resume_against_whole(_engine, _data(6), 3, extras=("fake_labels", "selected"), step=lambda e, b: e.step(b[0], labels=b[1]))
    (whole, _, _), (first, _, G1), (second, _, _) = made
    assert sd["n_classes"] == K3 and "class_embedding.weight" in G1.state_dict()
    plain, _, _ = _engine(n_classes=0)
    with pytest.raises(ValueError, match="n_classes=3, this engine has n_classes=0"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="n_classes=0, this engine has n_classes=3"):
        second.load_state_dict(plain.state_dict())
    for e in (whole, first, second, plain):
        e.close()


def test_off_is_off_and_on_is_on():
    """n_classes = 0 on a Kc = 3 head: the B Kc logits are B Kc samples (vg_gan_loss_pair), eager and replayed; with labels the
    trajectory is another one"""
    data = _data(6)
    runs = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        eng, D, G = _engine(n_classes=0, use_graph=use_graph)
        assert eng.real_labels is None and eng.fake_labels is None and not eng.cond and "class_embedding.weight" not in G.state_dict()
        one = _run(eng, data[:1])
        # rows [0, B) of logits / dlogits end the step as the generator's pass (role 2), rows [B, 2B) as the fake half of D's own
        # (role 1): vg_gan_loss_pair on B Kc samples each gives the step's two losses and every gradient
        lg = eng.logits.clone()
        ref_d, ref_l = torch.empty_like(lg), torch.empty(2, device="cuda")
        u.call("vg_gan_loss_pair", u.ptr(lg), u.ptr(ref_d), u.ptr(ref_l), B8 * K3, 2, B8 * K3, 1, 0, 1.0, None)
        torch.cuda.synchronize()
        assert torch.equal(_i32(one.losses[0, [2, 1]]), _i32(ref_l)) and torch.equal(_i32(eng.dlogits), _i32(ref_d))
        assert int((eng.dlogits == 0).sum()) == 0, "every one of the B Kc logits carries gradient"
        rest = _run(eng, data[1:])
        runs[name] = eu.join_runs(one, rest)
        with pytest.raises(ValueError, match="labels"):
            eng.step(data[0][0], labels=data[0][1])
        eng.close()
    _finite(runs["eager"], "unconditional")
    eu.assert_same_run(runs["graph"], runs["eager"], "unconditional: graph against eager")
    cond, _, _ = _engine()
    on = _run(cond, data)
    assert not torch.equal(on.losses, runs["eager"].losses) and not torch.equal(on.losses[:, 0], runs["eager"].losses[:, 0])
    for bad in (dict(), dict(labels=data[0][1].float()), dict(labels=data[0][1][:4]), dict(labels=data[0][1].cpu()),
                dict(labels=data[0][1], fake_labels=data[0][1])):
        with pytest.raises(ValueError, match="labels"):
            cond.step(data[0][0], **bad)
    cond.close()


# ---------------------------------------------------------------------------------------------------------------------- trainer
def test_train_model_conditional(tmp_path):
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTGAN
    from vit_gan_amd.training import SyntheticLoader, train_model, trainable_config
    cfg = {"epochs": 2, "batch_size": 8, "classes_count": 3, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 2}
    loader = SyntheticLoader(Config(**cfg), 2, torch.device("cuda:0"), labels=3)
    out = train_model(cfg, data_loader=loader, output_base=str(tmp_path), conditional=True)
    d, eng = out["dirs"], out["engine"]
    assert len(out["history"]) == 2 and all(bool(torch.isfinite(torch.tensor(h)).all()) for h in out["history"])
    assert eng.n_classes == 3 and eng.steps == 4 and out["discriminator"].vit._dims.Kc == 3 and out["generator"].n_classes == 3
    state = torch.load(os.path.join(d.save, "final_model.ckpt"), map_location="cpu")
    assert state["generator.class_embedding.weight"].shape == (3, 32 * 384)
    assert torch.equal(state["generator.class_embedding.weight"], out["generator"].class_embedding.weight.detach().cpu())
    fresh = ViTGAN(trainable_config(Config(**cfg), conditional=True), conditional=True)
    fresh.load_state_dict(state, strict=True)
    for e in (0, 1):
        assert os.path.getsize(os.path.join(d.images, f"samples_epoch_{e}.png")) > 100
    assert torch.load(os.path.join(d.save, "engine_state.pth"), map_location="cpu")["n_classes"] == 3
    assert "Class-conditional training: 3 classes" in open(os.path.join(d.save, "training.log")).read()
    # a loader without labels is the caller's error, raised out of the trainer; no checkpoint of such a run
    with pytest.raises(ValueError, match="no labels"):
        train_model(cfg, data_loader=SyntheticLoader(Config(**cfg), 1, torch.device("cuda:0")), output_base=str(tmp_path / "none"), conditional=True)
    assert not glob.glob(os.path.join(str(tmp_path / "none"), "output", "*", "final_model.ckpt"))
