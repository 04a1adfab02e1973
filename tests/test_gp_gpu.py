"""Gradient penalty (src/v2/utils.py:124-144, training.py:101-106) on the HIP path.

(1) every twice-differentiable operator of vit_gan_amd.ops2 against torch's own double backward of the same operator:
    first derivative taken with create_graph=True, contracted with a second random tensor, differentiated again;
(2) the product ``gradient_penalty`` on the reference's golden case (tests/golden/gp_v2.npz: produced by the reference's
    gradient_penalty on the reference's ViTDiscriminator) - penalty value and d penalty / d theta;
(3) the engine step with the penalty against the step oracle.
Tolerances: bf16 storage (2^-7 of max|ref| per rounding); second derivatives pass through 2-3 stored bf16 tensors -> 2^-5."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_util as eu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _second_order(fn_hip, fn_ref, inputs, seed):
    """inputs: list of (tensor, differentiate?) - first entry is x.  Returns per-input [first grads (of x), second grads]."""
    import gpu_util as u
    res = []
    for dev, fn in (("cuda", fn_hip), ("cpu", fn_ref)):
        ts = [t.detach().clone().to(dev).requires_grad_(True) for t in inputs]
        y = fn(*ts)
        g = torch.Generator().manual_seed(seed)
        U = u.rbf(torch.randn(y.shape, generator=g)).to(dev)
        V = u.rbf(torch.randn(ts[0].shape, generator=g)).to(dev)
        (gx,) = torch.autograd.grad(y, ts[0], grad_outputs=U, create_graph=True)
        (gx * V).sum().backward()
        res.append((y.detach(), gx.detach(), [t.grad for t in ts]))
    return res


def _compare(res, names, tol1=2.0 ** -6, tol2=2.0 ** -5):
    import gpu_util as u
    (y, gx, gg), (yr, gxr, ggr) = res
    u.assert_close(y, yr, 2.0 ** -7, "forward")
    u.assert_close(gx, gxr, tol1, "first derivative")
    for n, a, b in zip(names, gg, ggr):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, n
            continue
        u.assert_close(a, b, tol2, f"second-order gradient w.r.t. {n}", floor=1e-5)


@pytest.mark.parametrize("kind", ["gelu", "tanh"])
def test_activation_double_backward(kind):
    import gpu_util as u
    from vit_gan_amd import ops2
    h = u.rbf(torch.randn(130, 768, generator=torch.Generator().manual_seed(1)) * 1.5)
    ref = (lambda t: F.gelu(t)) if kind == "gelu" else torch.tanh
    _compare(_second_order(lambda t: ops2.act(t, kind), ref, [h], 2), ["h"])


def test_linear_double_backward():
    import gpu_util as u
    from vit_gan_amd import ops2
    g = torch.Generator().manual_seed(3)
    x = u.rbf(torch.randn(195, 384, generator=g))
    w = u.rbf(torch.randn(1152, 384, generator=g) / math.sqrt(384))
    b = torch.randn(1152, generator=g) * 0.1
    _compare(_second_order(lambda x_, w_, b_: ops2.linear(x_, w_, b_), lambda x_, w_, b_: F.linear(x_, w_, b_), [x, w, b], 4), ["x", "W", "b"])


# every width the first-order LayerNorm takes (E % 128 == 0, E <= 1024): the penalty step must not refuse a network the plain step
# trains - 640 and 896 fell out of the double backward's width switch in round 3, so the two sets are walked together here
@pytest.mark.parametrize("E", [128, 256, 384, 512, 640, 768, 896, 1024])
def test_layernorm_double_backward(E):
    import gpu_util as u
    from vit_gan_amd import ops2
    g = torch.Generator().manual_seed(5 + E)
    x = u.rbf(torch.randn(130 if E == 384 else 20, E, generator=g) * 1.3 + 0.2)
    gam = 1 + 0.2 * torch.randn(E, generator=g)
    bet = 0.1 * torch.randn(E, generator=g)
    _compare(_second_order(lambda x_, g_, b_: ops2.layer_norm(x_, g_, b_), lambda x_, g_, b_: F.layer_norm(x_, (E,), g_, b_, 1e-5),
                           [x, gam, bet], 6), ["x", "gamma", "beta"])


@pytest.mark.parametrize("B,H,S,HE", [(2, 4, 65, 96), (2, 8, 65, 64), (3, 4, 17, 32)])
def test_attention_double_backward(B, H, S, HE):
    import gpu_util as u
    from vit_gan_amd import ops2
    E = H * HE
    qkv = u.rbf(torch.randn(B, S, 3 * E, generator=torch.Generator().manual_seed(7)))

    def ref(t):
        q, k, v = (t[..., i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
        p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(HE), -1)
        return (p @ v).transpose(1, 2).reshape(B, S, E)
    _compare(_second_order(lambda t: ops2.attention(t, H), ref, [qkv], 8), ["qkv"])


def _golden_gp():
    from make_golden import GP_CASE as c
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    d = vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"],
                   layers=c["layers"], mlp_ratio=c["mlp_ratio"], classes=c["classes"])
    st = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    real = torch.from_numpy(make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"], "uniform"))
    fake = torch.from_numpy(make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"] + 1, "uniform"))
    return c, d, st, real, fake, np.load(os.path.join(GOLD, "gp_v2.npz"))


def test_gradient_penalty_matches_the_reference_fixture():
    import gpu_util as u
    from oracle import step_oracle as so, vit_oracle as vo
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.penalty import gradient_penalty
    c, d, st_np, real, fake, npz = _golden_gp()
    D = ViTDiscriminator(Config(attention_heads_count=c["heads"], classes_count=1, dropout_rate=0.0, embeddings_dimension=c["embed"],
                                transformer_blocks_count=c["layers"], batch_size=c["batch"]))
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    D = D.cuda().train()
    eps = torch.from_numpy(npz["epsilon"])
    D.zero_grad()
    pen = gradient_penalty(D, real.cuda(), fake.cuda(), epsilon=eps.cuda())
    pen.backward()
    torch.cuda.synchronize()
    # oracle (fp32 CPU, pinned to the same fixture by tests/test_oracle_golden.py) for element-wise gradient comparison
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    ref = so.gradient_penalty(lambda t: vo.vit_forward(st, t, d), real, fake, eps)
    ref.backward()
    print(f"penalty: HIP {float(pen):.6f}  reference {float(npz['penalty']):.6f}  oracle {float(ref):.6f}")
    assert abs(float(pen) - float(npz["penalty"])) < 2.0 ** -6 * float(npz["penalty"]) + 1e-4
    got = {"vit." + k if not k.startswith("vit.") else k: p.grad for k, p in D.named_parameters()}
    worst = []
    for k, p in st.items():
        if p.grad is None:
            continue
        scale = float(p.grad.abs().max())
        if scale < 1e-7:
            continue
        worst.append((u.assert_close(got[k], p.grad, 2.0 ** -4, f"d penalty / d {k}", floor=1e-5), k))
    print("largest gradient deviations:", [(k, f"{v:.2e}") for v, k in sorted(worst, reverse=True)[:5]])
    for k in ("vit.norm.weight", "vit.classifier.fc2.weight"):   # and directly against the reference's own numbers
        u.assert_close(got[k], torch.from_numpy(npz[f"full/{k}"]), 2.0 ** -4, f"{k} vs the reference fixture", floor=1e-5)


@pytest.mark.parametrize("B,autograd", [(8, False), (16, False), (8, True)])
def test_engine_step_with_gradient_penalty(B, autograd):
    """The reference's Wasserstein discriminator step with the penalty (training.py:83-106: critic loss + lambda_gp * gp,
    clipping) through GanEngine vs the step oracle, same noise and the same epsilon.  The penalty as one C call
    (vg_vit_penalty) - B = 16: 16 x 65 rows are whole units of 16, the fused full-row forms; B = 8: the GEMM + LayerNorm pairs -
    and, gp_autograd=True, as the operator set through autograd."""
    from vit_gan_amd.engine import GanEngine
    D, G, oracle = eu.build(B, "wasserstein")
    oracle.gp_weight = 10.0
    oracle.clip_d = 5.0
    eng = GanEngine(D, G, batch=B, loss="wasserstein", gp_weight=10.0, clip_d=5.0, external_noise=True, gp_autograd=autograd)
    assert eng.gp_c_call == (not autograd)
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    z = torch.randn(B, 1024, generator=g)
    eps = torch.rand(B, 1, 1, 1, generator=g)
    eng.gp_epsilon = eps.cuda()
    w0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    losses = eng.step(real.cuda(), z.cuda())
    torch.cuda.synchronize()
    # the oracle must see the engine's bf16 images (the penalty is evaluated on what D is fed)
    ref = oracle.step(real.to(torch.bfloat16).float(), z, gp_epsilon=eps)
    got = losses.cpu().tolist()
    print(f"gp: engine {float(eng.gp_loss):.5f} oracle {oracle.last_gp:.5f}; losses {got} vs {ref}")
    assert abs(float(eng.gp_loss) - oracle.last_gp) < 0.03 * abs(oracle.last_gp) + 1e-3
    for x, k in zip(got, ("d_real", "d_fake", "g")):
        assert abs(x - ref[k]) < 2e-2, (k, got, ref)
    k = "vit.encoder.1.fc2.weight"
    upd, ref_upd = D.state_dict()[k].detach().cpu() - w0[k], oracle.d[k].detach() - w0[k]
    assert float((upd - ref_upd).abs().max()) < 1.1e-3 and float(((upd - ref_upd).abs() < 1e-4).float().mean()) > 0.9
    with pytest.raises(ValueError):
        GanEngine(D, G, batch=B, gp_weight=1.0, two_stream=True)


@pytest.mark.parametrize("B,p_drop,autograd", [(8, 0.0, True), (8, 0.1, False), (16, 0.0, False), (16, 0.1, False)])
def test_engine_step_with_gradient_penalty_replays_as_a_graph(B, p_drop, autograd):
    """The penalty's passes captured in the step's hipGraph: three replayed steps equal three eager steps bit for bit, and the capture
    really is active.  autograd: the autograd passes of the operator set (dropout off and epsilon fixed: the only randomness of that pass
    is torch's); else the C call (B = 8: its unfused forms), also with dropout - its masks are the engine's counter-based ones, a function
    of the step counter."""
    from vit_gan_amd.engine import GanEngine
    g = torch.Generator().manual_seed(0)
    reals = [(torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda() for _ in range(3)]
    zs = [torch.randn(B, 1024, generator=g).cuda() for _ in range(3)]
    eps = torch.rand(B, 1, 1, 1, generator=g).cuda()
    out = []
    for use_graph in (False, True):
        D, G, _ = eu.build(B, "wasserstein")
        eng = GanEngine(D, G, batch=B, loss="wasserstein", gp_weight=10.0, clip_d=5.0, external_noise=True, use_graph=use_graph,
                        d_dropout=p_drop, g_dropout=p_drop, gp_autograd=autograd)
        assert eng.gp_c_call == (not autograd)
        eng.gp_epsilon = eps
        ls = [eng.step(r, z).clone() for r, z in zip(reals, zs)]
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None
        out.append((torch.stack(ls).cpu(), D.vit._flat.flat.detach().cpu().clone(), float(eng.gp_loss)))
        eng.close()
    assert torch.equal(out[0][0], out[1][0]), (out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][2] > 0


@pytest.mark.parametrize("B", [8, 32])
def test_deferred_grouped_weight_gradients_equal_autograd(B):
    """ops2.deferred_weight_grads: the block Linears' two weight-gradient contributions each, queued and sent as one grouped split-K
    launch + one fold per block and contribution (vg_linear_wgrad_group), against the same backward through plain autograd (one
    launch, fold and AccumulateGrad per contribution).  Same products, another K partition and summation order: fp32 round-off apart."""
    from vit_gan_amd import ops2
    from vit_gan_amd.penalty import gradient_penalty
    D, _, _ = eu.build(B, "wasserstein")
    fl = D.vit._flat
    g = torch.Generator().manual_seed(B)
    real = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda()
    fake = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda()
    eps = torch.rand(B, 1, 1, 1, generator=g).cuda()
    out = []
    for deferred in (False, True):
        fl.attach_grads()
        fl.grad.zero_()
        pen = gradient_penalty(D, real, fake, epsilon=eps)
        if deferred:
            with ops2.deferred_weight_grads(fl.grad) as q:
                pen.backward()
                assert len(q.items) == 2 * 4 * len(D.vit.encoder)  # two contributions to each of a block's four weights
        else:
            pen.backward()
        torch.cuda.synchronize()
        out.append(fl.grad.detach().clone())
    a, b = out
    assert float(a.abs().max()) > 0
    for name, (off, shape) in fl.slots.items():
        n = int(torch.tensor(shape).prod())
        ga, gb = a[off:off + n], b[off:off + n]
        scale = float(ga.abs().max())
        if name.endswith("weight") and ".encoder." in "." + name and ("attention" in name or "fc" in name):
            assert float((ga - gb).abs().max()) <= 2e-5 * scale + 1e-9, name   # regrouped fp32 sums of the same bf16 products
        else:
            assert torch.equal(ga, gb), name                                    # everything else took the same path


def _penalty_c_call(D, real, fake, eps, weight, p_drop=0.0, seed=11, step=None):
    """vg_vit_penalty straight through the C ABI: (penalty, flat gradient) of ``weight * penalty`` accumulated into a zeroed buffer."""
    import ctypes as C
    from vit_gan_amd import _lib
    L = _lib.lib()
    vit = D.vit
    fl = vit._flat
    fl.refresh_shadow()
    fl.grad.zero_()
    B = real.shape[0]
    d = vit._dims
    ws = torch.empty(L.vg_vit_ws_bytes(C.byref(d), B), dtype=torch.uint8, device="cuda")
    wp = torch.empty(L.vg_vit_penalty_ws_bytes(C.byref(d), B), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    net = _lib.VgVitNet(d, fl.flat.data_ptr(), fl.shadow.data_ptr(), fl.grad.data_ptr(), p_drop, seed, None if step is None else step.data_ptr(), None, 0, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rb, fb = real.to(torch.bfloat16).contiguous(), fake.to(torch.bfloat16).contiguous()
    e = eps.reshape(-1).float().contiguous()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.vg_vit_penalty(C.byref(net), B, p(rb), p(fb), p(e), float(weight), p(ws), p(wp), p(out), st), "vg_vit_penalty")
    torch.cuda.synchronize()
    return float(out), fl.grad.detach().clone()


@pytest.mark.parametrize("B,layers,geo", [(16, 2, "c2"), (32, 3, "c2"), (256, 6, "c2"), (16, 2, "c4"), (16, 2, "c2-10-classes"), (48, 1, "c2-mlp4"),
                                          (8, 2, "c2"), (8, 2, "e128"), (8, 1, "c5")])
def test_penalty_c_call_matches_the_operator_set(B, layers, geo):
    """vg_vit_penalty (forward, input-gradient backward, its double backward and the second backward as ONE C call) against the
    operator-set form through torch autograd (penalty.gradient_penalty, itself pinned to the reference's fixture above): dropout off,
    the same epsilon.  Both are bf16 pipelines with different fusion (the C call's second backward runs the fused full-row kernels):
    per tensor within 2^-6 of max|.|, the penalty within 2^-7."""
    from vit_gan_amd import ops2
    from vit_gan_amd.penalty import gradient_penalty
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    # c2: 32 x 32, patch 4, E = 384, 4 heads; c4: BASELINE configs[3]'s geometry (64 x 64, patch 8, E = 512, 8 heads of 64: the N = 512
    # instantiation of the full-row kernels and of their penalty variant); 10 classes: the classifier's second-order kernel with more than
    # one logit; mlp4: forward_mul 4
    kw = dict(embeddings_dimension=384, classes_count=1, dropout_rate=0.0, batch_size=B, transformer_blocks_count=layers)
    img = 32
    if geo == "c4":
        kw.update(embeddings_dimension=512, attention_heads_count=8, patch_size=8, image_size=64)
        img = 64
    elif geo == "c2-10-classes":
        kw.update(classes_count=10)
    elif geo == "c2-mlp4":
        kw.update(mlp_ratio=4)
    elif geo == "e128":    # no full-row kernel at this width: the GEMM + LayerNorm pairs (B = 8 at c2: rows not whole units of 16 - the same)
        kw.update(embeddings_dimension=128, attention_heads_count=4)
    elif geo == "c5":      # BASELINE configs[4]'s geometry with bf16 attention: 128 x 128, patch 16, E = 768, 12 heads
        kw.update(embeddings_dimension=768, attention_heads_count=12, patch_size=16, image_size=128)
        img = 128
    torch.manual_seed(3)
    D = ViTDiscriminator(Config(**kw)).cuda()
    D.train()
    fl = D.vit._flat
    g = torch.Generator().manual_seed(B)
    real = (torch.rand(B, 3, img, img, generator=g) * 2 - 1).cuda().to(torch.bfloat16).float()
    fake = (torch.rand(B, 3, img, img, generator=g) * 2 - 1).cuda().to(torch.bfloat16).float()
    eps = torch.rand(B, 1, 1, 1, generator=g).cuda()
    w = 10.0
    fl.attach_grads()
    fl.grad.zero_()
    pen = gradient_penalty(D, real, fake, epsilon=eps)
    with ops2.deferred_weight_grads(fl.grad):
        (w * pen).backward()
    torch.cuda.synchronize()
    ref_pen, ref = float(pen.detach()), fl.grad.detach().clone()
    got_pen, got = _penalty_c_call(D, real, fake, eps, w)
    print(f"penalty: C call {got_pen:.6f}  operator set {ref_pen:.6f}")
    assert abs(got_pen - ref_pen) <= 2.0 ** -7 * abs(ref_pen) + 1e-5
    # (tensors whose gradient is round-off of an exact zero - the key bias, which the softmax cancels - are held to the buffer's scale)
    floor = 2.0 ** -10 * float(ref.abs().max())
    worst, bad = [], []
    for name, (off, shape) in fl.slots.items():
        n = int(torch.tensor(shape).prod())
        a, b = got[off:off + n], ref[off:off + n]
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        worst.append((err / max(scale, floor), name, err, scale))
        if not err <= 2.0 ** -6 * scale + floor:
            bad.append((name, err, scale))
    print("largest deviations:", [(k, f"{v:.2e}", f"{e:.2e}/{sc:.2e}") for v, k, e, sc in sorted(worst, reverse=True)[:8]])
    assert not bad, bad


@pytest.mark.parametrize("B,layers", [(16, 2), (256, 6)])
def test_penalty_c_call_with_dropout_is_the_gradient_of_its_own_value(B, layers):
    """Train-mode dropout (the reference's discriminator is in train mode inside gradient_penalty): the five passes of the call must draw
    the same masks.  A mask mismatch between any two passes leaves the value fine and the gradient wrong, so: the directional derivative
    of the call's penalty VALUE along its own gradient, by central differences on the fp32 master weights (same seed and step counter =
    same masks), against |gradient|^2."""
    D, _, _ = eu.build(B, "wasserstein", layers=layers)   # (256, 6): the benchmarked configuration
    D.train()
    fl = D.vit._flat
    g = torch.Generator().manual_seed(5)
    real = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda()
    fake = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda()
    eps = torch.rand(B, 1, 1, 1, generator=g).cuda()
    step = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    pen0, grad = _penalty_c_call(D, real, fake, eps, 1.0, p_drop=0.1, step=step)
    pen0_off, _ = _penalty_c_call(D, real, fake, eps, 1.0, p_drop=0.0)
    assert pen0 != pen0_off  # the masks are really on
    w0 = fl.flat.detach().clone()
    gn2 = float((grad.double() ** 2).sum())
    assert gn2 > 0
    # a step that moves the penalty by a few percent: far above the bf16 noise of its evaluation, still in the linear range
    h = 0.04 * pen0 / gn2
    vals = []
    for sgn in (+1.0, -1.0):
        with torch.no_grad():
            fl.flat.copy_(w0 + sgn * h * grad)
        vals.append(_penalty_c_call(D, real, fake, eps, 1.0, p_drop=0.1, step=step)[0])
    with torch.no_grad():
        fl.flat.copy_(w0)
    fl.refresh_shadow()
    fd = (vals[0] - vals[1]) / (2 * h)
    print(f"penalty {pen0:.5f}; directional derivative: finite differences {fd:.5e}  |grad|^2 {gn2:.5e}  ratio {fd / gn2:.3f}")
    assert 0.8 < fd / gn2 < 1.25


def test_penalty_step_replay_does_not_depend_on_host_synchronisation():
    """Regression (round 4): the penalty call zero-filled one buffer with hipMemsetAsync.  As a memset node of the step's hipGraph it went
    wrong once the host had queued about a hundred replays ahead of the device: the replayed step then depended on how often the host
    synchronised (tools/micro/gp_determinism.py: identical for 80 steps, a different - collapsed - trajectory by step 140; a soak run
    went non-finite at step 2 700).  The fill is a kernel now.  Full-size configuration (where it showed), 200 replayed steps, a sync
    after every step against none at all: bit-identical weights (the memset build fails this)."""
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    B = 256
    out = []
    for sync_every_step in (False, True):
        torch.manual_seed(0)
        D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, batch_size=B)).cuda().train()
        G = SirenGenerator().cuda().train()
        eng = GanEngine(D, G, batch=B, use_graph=True, loss="wasserstein", gp_weight=10.0, clip_d=5.0, clip_g=0.5)
        assert eng.gp_c_call
        gen = torch.Generator(device="cuda").manual_seed(1)
        reals = [torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1 for _ in range(4)]
        keep = []
        for i in range(200):
            l = eng.step(reals[i % 4])
            if i % 20 == 0:
                keep.append(l.clone())  # (ordinary stream work between the replays, as a training loop has)
            if sync_every_step or i == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert eng.graph_active
        out.append((D.vit._flat.flat.detach().clone(), G._flat.flat.detach().clone(), float(eng.gp_loss)))
        eng.close()
    assert torch.isfinite(out[0][0]).all() and out[0][2] > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
