"""Teacher-forced trajectory of GanEngine's optimizer.  Before every checked step the D and G training state (master, moments, step
counter) is snapshot; after it, every element of both flat buffers must be one float64 AdamW step (tests/adamw_ref.py) from the
snapshot with the gradient the step consumed (after a step ``fd.grad`` / ``fg.grad`` hold exactly that), at the shared device step
count t.  Eager and hipGraph replay, the three losses, clipping; on ``ns`` the consumed gradients themselves against the fp32 CPU
oracle's networks loaded with the engine's weights.  The oracle runs rounding-faithful (bf16 where the engine stores bf16): by the
last checked step D is confident, the BCE derivative sigmoid(l) - y is small, and the fp32 oracle's logits differ from the engine's
by the bf16 forward's own error - enough to move every D gradient by a common ~6.5 % (measured), which says nothing about the
optimizer's wiring."""
import pytest
import torch

import engine_util as eu
from adamw_ref import check_adamw_step

pytestmark = pytest.mark.gpu

B = 8
STEPS = 12
REPLAYS = 200
CASES = [("ns", {}), ("hinge", {}), ("wasserstein", dict(clip_d=0.05, clip_g=0.02))]


def _slots(module, fp):
    """name -> (offset, numel, shape) of every parameter of ``module`` inside the flat buffer ``fp.flat``."""
    base = fp.flat.data_ptr()
    out = {}
    for k, p in module.named_parameters():
        off = (p.data_ptr() - base) // 4
        assert 0 <= off and off + p.numel() <= fp.total, k
        out[k] = (off, p.numel(), tuple(p.shape))
    return out


def _snapshot(eng):
    fd, fg = eng.vit._flat, eng.gen._flat
    return {"t": int(eng.step_t), "d": (fd.flat.clone(), eng.m_d.clone(), eng.v_d.clone()),
            "g": (fg.flat.clone(), eng.m_g.clone(), eng.v_g.clone())}


def _check_step(eng, snap, t, kw, what):
    """The step just taken, from ``snap``: step counter, both optimizers elementwise, clipping.  Returns the worst update errors."""
    h = eng.hyp
    assert snap["t"] == t - 1 and int(eng.step_t) == t, (what, snap["t"], int(eng.step_t), t)
    gscale = 1.0 / eng.world
    worst = []
    for net, fp, m, v, lr, clip in (("d", eng.vit._flat, eng.m_d, eng.v_d, h["lr_d"], kw.get("clip_d")),
                                    ("g", eng.gen._flat, eng.m_g, eng.v_g, h["lr_g"], kw.get("clip_g"))):
        p0, m0, v0 = snap[net]
        worst.append(check_adamw_step(p0, m0, v0, fp.grad, t, (lr, h["b1"], h["b2"], h["eps"], h["wd"]), gscale, fp.flat, m, v, fp.shadow,
                                      f"{what} step {t} {net.upper()}"))
        if clip is not None:  # the consumed gradient obeys the global norm limit
            norm = float((fp.grad.double() * gscale).norm())
            assert norm <= clip * (1 + 1e-5), f"{what} step {t} {net.upper()}: consumed gradient norm {norm} > {clip}"
    return worst


def _load(params, module, fp, flat):
    """Copy the weights in ``flat`` (a flat master buffer of ``module``) into the oracle's parameter dict."""
    with torch.no_grad():
        for k, (off, n, shape) in _slots(module, fp).items():
            params[k].copy_(flat[off:off + n].view(shape).cpu())


def _check_grads(eng, D, G, oracle, snap, real, what):
    """The gradients the step consumed against the oracle: D's pass with the pre-step D and G weights, G's pass through the
    POST-update D (training.py:197-211)."""
    from oracle import step_oracle as so
    fd, fg = eng.vit._flat, eng.gen._flat
    _load(oracle.d, D, fd, snap["d"][0])
    _load(oracle.g, G, fg, snap["g"][0])
    z = eng.z.detach().cpu().clone()  # the engine's own noise of this step
    real = real.cpu()
    for p in list(oracle.d.values()) + list(oracle.g.values()):
        p.grad = None
    so.d_loss_real(oracle.D(real), "ns").backward()
    fake = oracle.G(z)
    so.d_loss_fake(oracle.D(fake.detach()), "ns").backward()
    _compare(D, fd, oracle.d, 2.0 ** -4, f"{what}: D")
    _load(oracle.d, D, fd, fd.flat)  # the updated discriminator
    for p in oracle.g.values():
        p.grad = None
    so.g_loss(oracle.D(fake), "ns").backward()
    _compare(G, fg, oracle.g, 0.15, f"{what}: G")


def _compare(module, fp, ref_params, rel, what):
    """Every tensor of the consumed gradient whose max|ref| >= 1e-6 (the key biases excepted): max|got - ref| <= rel * max|ref|.  A one-element parameter (the
    generator's self-modulated LayerNorm scalars) has as gradient ONE sum over every batch, token and channel position of its layer,
    which can cancel to far below its terms (seen: 1.1e-5 where its sibling gradients are 8e-5, with the same ~5e-6 absolute bf16
    error as the next layer's uncancelled 2.7e-4): it is held to rel times the largest max|ref| of its module's parameters."""
    slots = _slots(module, fp)
    scales = {k: float(ref_params[k].grad.abs().max()) for k in slots}
    rows, bad = [], []
    for k, (off, n, shape) in slots.items():
        ref = ref_params[k].grad
        scale = scales[k]
        if scale < 1e-6 or k.endswith("attention.keys.bias"):  # (a key bias shifts every score of a query equally: its exact gradient
            continue                                                # is 0, and both sides hold rounding noise there)
        if n == 1:
            parent = k.rsplit(".", 1)[0] + "."
            scale = max(v for j, v in scales.items() if j.startswith(parent))
        err = float((fp.grad[off:off + n].view(shape).cpu() - ref).abs().max()) / scale
        rows.append(f"{k} max|ref| {scale:.3e} rel {err:.4f}")
        if err > rel:
            bad.append(rows[-1])
    print(f"\n{what} gradients:\n  " + "\n  ".join(rows))
    assert len(rows) >= 10 and not bad, f"{what} gradient beyond {rel:g} of max|ref|: {bad}"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("loss,kw", CASES, ids=[c[0] for c in CASES])
def test_optimizer_trajectory_matches_fp64_adamw(loss, kw, use_graph):
    from vit_gan_amd.engine import GanEngine

    D, G, oracle = eu.build(B, loss, faithful=True)
    eng = GanEngine(D, G, batch=B, loss=loss, use_graph=use_graph, **kw)
    gen = torch.Generator().manual_seed(1)
    reals = [(torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(4)]
    what = f"{loss} {'graph' if use_graph else 'eager'}"
    worst = [0.0, 0.0]
    for t in range(1, STEPS + 1):
        snap = _snapshot(eng)
        real = reals[t % 4]
        eng.step(real)
        torch.cuda.synchronize()
        for w in _check_step(eng, snap, t, kw, what):
            worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        if loss == "ns" and t in (1, STEPS):
            _check_grads(eng, D, G, oracle, snap, real, f"{what} step {t}")
    assert eng.graph_active == use_graph, eng.graph_fallback_reason
    t = STEPS
    if use_graph:  # a long replayed run, then one more checked step
        for _ in range(REPLAYS):
            t += 1
            eng.step(reals[t % 4])
        t += 1
        snap = _snapshot(eng)
        eng.step(reals[t % 4])
        torch.cuda.synchronize()
        _check_step(eng, snap, t, kw, what)
    # a fresh optimizer: the next step runs at t = 1 from zero moments
    eng.sync_from_modules(reset_optimizer=True)
    snap = _snapshot(eng)
    assert all(float(x.abs().max()) == 0.0 for x in (snap["d"][1], snap["d"][2], snap["g"][1], snap["g"][2]))
    eng.step(reals[0])
    torch.cuda.synchronize()
    _check_step(eng, snap, 1, kw, f"{what} after reset_optimizer")
    print(f"\ntrajectory {what}: worst {worst[0]:.4f} of the bound, update error {worst[1]:.4f} x 2^-12")
    eng.close()
