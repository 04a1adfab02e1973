"""The R1 penalty on the GPU: the one-call form vg_vit_r1 against the operator-set form (penalty.r1_penalty through torch autograd),
both against the float64 restatement of tests/r1_ref.py, the dropout masks of its passes, and the engine around it - gradient, lazy
schedule and call trace, hipGraph replay with two captured graphs, resume, trainer.  Small shapes throughout."""
import ctypes as C
import functools
import os

import pytest
import torch

import engine_util as eu

pytestmark = pytest.mark.gpu


def _r1_c_call(D, x, weight, p_drop=0.0, seed=11, step=None):
    """vg_vit_r1 straight through the C ABI: (penalty as a device float, flat gradient of ``weight * penalty`` accumulated into a zeroed buffer)"""
    from vit_gan_amd import _lib
    L = _lib.lib()
    vit = D.vit
    fl = vit._flat
    fl.refresh_shadow()
    fl.grad.zero_()
    B, d = x.shape[0], vit._dims
    ws = torch.empty(L.vg_vit_ws_bytes(C.byref(d), B), dtype=torch.uint8, device="cuda")
    wp = torch.empty(L.vg_vit_penalty_ws_bytes(C.byref(d), B), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    net = _lib.VgVitNet(d, fl.flat.data_ptr(), fl.shadow.data_ptr(), fl.grad.data_ptr(), p_drop, seed, None if step is None else step.data_ptr(), None, 0, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    xb = x.to(torch.bfloat16).contiguous()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.vg_vit_r1(C.byref(net), B, p(xb), float(weight), p(ws), p(wp), p(out), st), "vg_vit_r1")
    torch.cuda.synchronize()
    return out, fl.grad.detach().clone()


def _operator_set(D, x, weight):
    """(penalty, flat gradient of ``weight * penalty``) through penalty.r1_penalty, autograd and the grouped weight gradients"""
    from vit_gan_amd import ops2
    from vit_gan_amd.penalty import r1_penalty
    fl = D.vit._flat
    fl.attach_grads()
    fl.grad.zero_()
    pen = r1_penalty(D, x)
    with ops2.deferred_weight_grads(fl.grad):
        (weight * pen).backward()
    torch.cuda.synchronize()
    return float(pen.detach()), fl.grad.detach().clone()


def _disc(B, layers, geo):
    """the geometries of test_gp_gpu.test_penalty_c_call_matches_the_operator_set"""
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    kw = dict(embeddings_dimension=384, classes_count=1, dropout_rate=0.0, batch_size=B, transformer_blocks_count=layers)
    img = 32
    if geo == "c4":
        kw.update(embeddings_dimension=512, attention_heads_count=8, patch_size=8, image_size=64)
        img = 64
    elif geo == "c2-10-classes":
        kw.update(classes_count=10)
    elif geo == "c2-17-classes":
        kw.update(classes_count=17)
    elif geo == "e128":
        kw.update(embeddings_dimension=128, attention_heads_count=4)
    torch.manual_seed(3)
    return ViTDiscriminator(Config(**kw)).cuda().train(), img


@pytest.mark.parametrize("B,layers,geo", [(16, 2, "c2"), (8, 2, "c2"), (8, 2, "e128"), (16, 2, "c4"), (16, 2, "c2-10-classes"), (16, 2, "c2-17-classes")])
def test_r1_c_call_matches_the_operator_set(B, layers, geo):
    """(16, c2): the fused full-row forms; (8, c2) and e128: the GEMM + LayerNorm pairs; c4: the N = 512 instantiation; 10 classes: the
    head's second-order kernel with more than one logit; 17 classes: the head's first backward on its separate dz kernel (Kc > 16).  Dropout off, weight 5.  Tolerances of the gradient penalty's own test: the
    penalty within 2^-7 relative + 1e-5, every tensor within 2^-6 max|ref| + 2^-10 max|whole buffer|."""
    D, img = _disc(B, layers, geo)
    fl = D.vit._flat
    x = (torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(B)) * 2 - 1).cuda().to(torch.bfloat16).float()
    w = 5.0
    ref_pen, ref = _operator_set(D, x, w)
    out, got = _r1_c_call(D, x, w)
    got_pen = float(out)
    print(f"R1: C call {got_pen:.6f}  operator set {ref_pen:.6f}")
    assert ref_pen > 0 and abs(got_pen - ref_pen) <= 2.0 ** -7 * abs(ref_pen) + 1e-5
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


@functools.lru_cache(maxsize=None)
def _fp64_case():
    """GP_CASE weights, bf16-rounded images, and the float64 oracle on them - computed once for both forms"""
    import r1_ref
    from make_golden import GP_CASE as c
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    d = r1_ref.case_dims(c)
    st = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    x = torch.from_numpy(make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"], "uniform")).to(torch.bfloat16).float()
    pen, grads = r1_ref.r1_oracle(st, d, x, torch.float64)
    return c, st, x, pen, grads


@pytest.mark.parametrize("form", ["operator_set", "c_call"])
def test_r1_matches_the_float64_oracle(form):
    """A tier that does not share the kernels' rounding assumptions.  Tolerances of test_gradient_penalty_matches_the_reference_fixture:
    penalty 2^-6 relative + 1e-4, gradients 2^-4 of max|ref| with floor 1e-5.  Skipped: only a tensor the reference gives NO gradient
    (the head's fc2.bias: d sum(logits) / dx does not depend on it) - 1 of 42, the cap is 2.  The two key biases have a float64
    reference gradient that is round-off of an exact zero (3e-18 and 8e-18: the softmax cancels a key bias), under the 1e-7 below which
    that test skips; skipping them too would make 3 of 42, over the cap, whatever the code under test does.  So they are NOT skipped:
    they are held to 2^-10 of max|whole reference buffer|, the floor test_r1_c_call_matches_the_operator_set (and the gradient
    penalty's test before it) gives exactly these tensors - a bf16 pipeline's sum of cancelling terms is round-off at the scale of the
    terms, not of the result."""
    import gpu_util as u
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    c, st_np, x, ref_pen, ref = _fp64_case()
    D = ViTDiscriminator(Config(attention_heads_count=c["heads"], classes_count=1, dropout_rate=0.0, embeddings_dimension=c["embed"],
                                transformer_blocks_count=c["layers"], batch_size=c["batch"]))
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    D = D.cuda().train()
    fl = D.vit._flat
    if form == "c_call":
        out, flat_grad = _r1_c_call(D, x.cuda(), 1.0)
        pen = float(out)
    else:
        pen, flat_grad = _operator_set(D, x.cuda(), 1.0)
    got = {"vit." + k: flat_grad[off:off + int(torch.tensor(shape).prod())].view(shape) for k, (off, shape) in fl.slots.items()}
    print(f"R1 ({form}): HIP {pen:.6f}  float64 oracle {ref_pen:.6f}")
    assert abs(pen - ref_pen) < 2.0 ** -6 * ref_pen + 1e-4
    assert set(got) == set(ref) and len(ref) == 42
    skipped, worst = [], []
    zero_floor = 2.0 ** -10 * max(float(g.abs().max()) for g in ref.values() if g is not None)
    for k, g in ref.items():
        if g is None:
            skipped.append(k)
            continue
        if float(g.abs().max()) < 1e-7:  # an exact zero in the reference
            print(f"  {k}: reference max {float(g.abs().max()):.2e}, HIP max {float(got[k].abs().max()):.3e}, held to {zero_floor:.3e}")
            assert float(got[k].abs().max()) <= zero_floor, k
            continue
        worst.append((u.assert_close(got[k], g.float(), 2.0 ** -4, f"d penalty / d {k}", floor=1e-5), k))
    print("skipped:", skipped, " largest deviations:", [(k, f"{v:.2e}") for v, k in sorted(worst, key=lambda t: -(t[0] or 0))[:5]])
    assert len(skipped) <= 2, skipped


def test_r1_c_call_at_17_classes_matches_the_float64_oracle():
    """Above 16 classes the seed of the input gradient, vg_head_bwd_launch(ones, ...), runs the head's separate dz kernel.  vg_vit_r1 on
    the smallest network the layout takes (16 x 16 images, 4 x 4 patches, E 128, 2 blocks, B 8) against r1_ref.r1_oracle in float64, at
    the tolerances of test_r1_matches_the_float64_oracle: penalty 2^-6 relative + 1e-4, gradients 2^-4 of max|ref| with floor 1e-5, a
    reference that is round-off of an exact zero held to 2^-10 of max|whole reference buffer|, only fc2.bias without a gradient."""
    import gpu_util as u
    import r1_ref
    from oracle import vit_oracle as vo
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    from weights import make_input, make_state
    B = 8
    d = vo.VitDims(channels=3, image=16, patch=4, embed=128, heads=4, layers=2, mlp_ratio=2, classes=17)
    st_np = make_state(vo.vit_param_shapes(d), 61, "vit")
    x = torch.from_numpy(make_input((B, 3, 16, 16), 62, "uniform")).to(torch.bfloat16).float()
    ref_pen, ref = r1_ref.r1_oracle(st_np, d, x, torch.float64)
    D = ViTDiscriminator(Config(attention_heads_count=4, classes_count=17, dropout_rate=0.0, embeddings_dimension=128, transformer_blocks_count=2,
                                batch_size=B, image_size=16, patch_size=4))
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    D = D.cuda().train()
    fl = D.vit._flat
    out, flat_grad = _r1_c_call(D, x.cuda(), 1.0)
    pen = float(out)
    got = {"vit." + k: flat_grad[off:off + int(torch.tensor(shape).prod())].view(shape) for k, (off, shape) in fl.slots.items()}
    print(f"R1 at 17 classes: HIP {pen:.6f}  float64 oracle {ref_pen:.6f}")
    assert ref_pen > 0 and abs(pen - ref_pen) < 2.0 ** -6 * ref_pen + 1e-4
    assert set(got) == set(ref)
    zero_floor = 2.0 ** -10 * max(float(g.abs().max()) for g in ref.values() if g is not None)
    skipped = []
    for k, g in ref.items():
        if g is None:
            skipped.append(k)
        elif float(g.abs().max()) < 1e-7:
            assert float(got[k].abs().max()) <= zero_floor, k
        else:
            u.assert_close(got[k], g.float(), 2.0 ** -4, f"d penalty / d {k}", floor=1e-5)
    assert skipped == ["vit.classifier.fc2.bias"], skipped


def test_r1_c_call_with_dropout_is_the_gradient_of_its_own_value():
    """The five passes must draw the same masks: a mismatch leaves the value fine and the gradient wrong.  The directional derivative of
    the call's VALUE along its own gradient, central differences on the fp32 master (same seed and step counter = same masks), against
    |gradient|^2 - the gradient penalty's test on vg_vit_r1, in the project's band (0.8, 1.25)."""
    B = 16
    D, _, _ = eu.build(B, "ns", layers=2)
    D.train()
    fl = D.vit._flat
    x = (torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    step = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    val = lambda **kw: float(_r1_c_call(D, x, 1.0, **kw)[0])  # noqa: E731
    out, grad = _r1_c_call(D, x, 1.0, p_drop=0.1, step=step)
    pen0 = float(out)
    assert pen0 != val(p_drop=0.0)  # the masks are really on
    w0 = fl.flat.detach().clone()
    gn2 = float((grad.double() ** 2).sum())
    assert gn2 > 0
    h = 0.04 * pen0 / gn2  # moves the penalty by a few percent: far above the bf16 noise of its evaluation, still in the linear range
    vals = []
    for sgn in (+1.0, -1.0):
        with torch.no_grad():
            fl.flat.copy_(w0 + sgn * h * grad)
        vals.append(val(p_drop=0.1, step=step))
    with torch.no_grad():
        fl.flat.copy_(w0)
    fl.refresh_shadow()
    fd = (vals[0] - vals[1]) / (2 * h)
    print(f"R1 {pen0:.5f}; directional derivative: finite differences {fd:.5e}  |grad|^2 {gn2:.5e}  ratio {fd / gn2:.3f}")
    assert 0.8 < fd / gn2 < 1.25


def test_engine_step_adds_the_r1_gradient():
    """One eager step of two engines on identical modules and inputs, R1 on (gamma 10) and off.  D's own pass of the first step does
    not see the penalty: the discriminator's two losses are bit-equal.  (The generator's loss is taken through the UPDATED D, training.py:
    199-211, which has the penalty's gradient in its AdamW step: 0.8556 against 1.8117 here - it must differ.)  ``r1_loss`` is bit-equal to a direct vg_vit_r1 call on the engine's own real rows with its
    dropout key, and D.grad(on) - D.grad(off) is that call's gradient r up to fp32 accumulation round-off, bounded as follows.

    Every element of D.grad is a left-to-right fp32 sum: the step zeroes the buffer, the penalty call (when on) adds r - exactly, to a
    zero - and D's own backward then adds its addends t_1 .. t_k in a fixed order (vg_slab_reduce_kernel adds the split-K slices
    to the destination one by one, at most VIT_SPLIT_CAP = 16 per block weight and EMB_SPLIT_CAP = 32 for the patch embedding;
    vg_colsum_f32_kernel and the GEMMs that accumulate in place add one pre-summed term per launch, at most 2 launches per element).
    The t_i are the same bits in both engines (same forward, same logits), so on = fl(..fl(r + t_1).. + t_k) and
    off = fl(..fl(t_1 + t_2).. + t_k) differ from r + sum t and sum t by at most k and k - 1 roundings of 2^-24 relative to the
    running sum each, k <= 32 + 2.  With the running sums held to S = max|r| + max|off| over the tensor (partial sums over fewer
    rows or slices of the same batch are gradients of the same kind; they are given no more room than the totals),
        |(on - off) - r| <= (2 k - 1) 2^-24 S <= 67 * 2^-24 * S ~ 4.0e-6 S.   The difference itself is taken in float64."""
    from vit_gan_amd.engine import GanEngine
    B = 16
    (real, z), = eu.batches(B, 1, seed=0)
    res = {}
    for gamma in (10.0, 0.0):
        D, G, _ = eu.build(B, "ns")
        eng = GanEngine(D, G, batch=B, loss="ns", external_noise=True, d_dropout=0.0, g_dropout=0.0, r1_gamma=gamma, seed=2)
        w_before = D.vit._flat.flat.detach().clone()
        losses = eng.step(real, z).clone()
        torch.cuda.synchronize()
        res[gamma] = (losses, D.vit._flat.grad.detach().clone())
        if gamma:
            assert eng.ws_gp is not None and eng.r1_loss.is_cuda and eng.r1_loss.dtype == torch.float32
            r1_loss, x_seen = eng.r1_loss.clone(), eng.d_in_half[0].clone()
            fl, slots = D.vit._flat, D.vit._flat.slots
            with torch.no_grad():  # the call ran before D's AdamW: on the weights the step began with
                fl.flat.copy_(w_before)
            step = torch.ones(1, dtype=torch.int32, device="cuda")
            direct, r = _r1_c_call(D, x_seen, 0.5 * gamma, p_drop=0.0, seed=eng.seed * 8 + 3, step=step)
        else:
            assert eng.r1_loss is None and not hasattr(eng, "ws_gp")
        eng.close()
    assert torch.equal(res[10.0][0][:2], res[0.0][0][:2]), (res[10.0][0], res[0.0][0])
    assert not torch.equal(res[10.0][0][2], res[0.0][0][2])  # the penalty reached D's update
    assert torch.equal(r1_loss, direct) and float(direct) > 0, (r1_loss, direct)
    on, off = res[10.0][1].double(), res[0.0][1].double()
    assert float(r.abs().max()) > 0
    bad = []
    for name, (o, shape) in slots.items():
        n = int(torch.tensor(shape).prod())
        err = float(((on[o:o + n] - off[o:o + n]) - r[o:o + n].double()).abs().max())
        S = float(r[o:o + n].abs().max()) + float(off[o:o + n].abs().max())
        if not err <= 67 * 2.0 ** -24 * S:
            bad.append((name, err, S))
    assert not bad, bad


def _renumber(calls):
    """the allocation indices of a list of calls renumbered by first appearance in it (a pointer is [allocation, byte offset])"""
    index = {}

    def walk(v):
        if isinstance(v, list):
            if len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) for e in v):
                return [index.setdefault(v[0], len(index)), v[1]]
            return [walk(e) for e in v]
        return v
    return [[name, walk(args)] for name, args in calls]


def _steps_of(calls):
    starts = [i for i, c in enumerate(calls) if c[0] == "vg_step_inputs"] + [len(calls)]
    return [calls[a:b] for a, b in zip(starts, starts[1:])]


def test_lazy_schedule_in_the_call_trace():
    """r1_interval = 2 over two eager steps: the first step is the plain first step plus exactly one vg_vit_r1 where the gradient
    penalty's call sits in the recorded ``gp`` trace, weight 0.5 * 10 * 2; the second step is the plain second step.  gamma 0 is the
    plain trace.  (The call brings two allocations of its own, so the plain calls are compared after renumbering each step's.)"""
    import json
    import step_trace as stt
    plain, ext0 = stt.trace()
    got, ext = stt.trace(r1_gamma=10, r1_interval=2)
    assert ext == 0 and ext0 == 0
    off, ext_off = stt.trace(r1_gamma=0)
    assert ext_off == 0 and off == plain
    (p1, p2), (g1, g2) = _steps_of(plain), _steps_of(got)
    where = [i for i, c in enumerate(g1) if c[0] == "vg_vit_r1"]
    with open(stt.FIXTURE) as f:
        gp1 = _steps_of(json.load(f)["traces"]["gp"])[0]
    assert where == [i for i, c in enumerate(gp1) if c[0] == "vg_vit_penalty"] and len(where) == 1
    call = g1[where[0]][1]
    assert call[1] == stt.B and call[3] == 10.0 and call[-1] == "s0"
    assert _renumber(g1[:where[0]] + g1[where[0] + 1:]) == _renumber(p1)
    assert not any(c[0] == "vg_vit_r1" for c in g2) and _renumber(g2) == _renumber(p2)


def test_r1_loss_changes_on_due_steps_only():
    from vit_gan_amd.engine import GanEngine
    B = 8
    D, G, _ = eu.build(B, "ns")
    eng = GanEngine(D, G, batch=B, external_noise=True, r1_gamma=10.0, r1_interval=4)
    seen = [eng.r1_loss.clone()]
    for real, z in eu.batches(B, 6, seed=0):
        eng.step(real, z)
        seen.append(eng.r1_loss.clone())
    torch.cuda.synchronize()
    eng.close()
    changed = [i for i in range(1, 7) if not torch.equal(seen[i], seen[i - 1])]
    assert changed == [1, 5], (changed, [float(s) for s in seen])


def _run(B, n, use_graph, p_drop=0.1, first=None, **kw):
    """n steps (after loading ``first`` = (engine state, D weights, G weights, steps done)) -> (losses, D master, G master, r1_loss, engine)"""
    from vit_gan_amd.engine import GanEngine
    D, G, _ = eu.build(B, "ns")
    eng = GanEngine(D, G, batch=B, external_noise=True, use_graph=use_graph, d_dropout=p_drop, g_dropout=p_drop, seed=1, **kw)
    skip = 0
    if first is not None:
        state, d_sd, g_sd, skip = first
        D.load_state_dict(d_sd)
        G.load_state_dict(g_sd)
        eng.load_state_dict(state)
    ls = [eng.step(real, z).clone() for real, z in eu.batches(B, n, skip=skip, seed=0)]
    torch.cuda.synchronize()
    return torch.stack(ls).cpu(), D.vit._flat.flat.detach().cpu().clone(), G._flat.flat.detach().cpu().clone(), eng.r1_loss.cpu().clone(), eng, D, G


@pytest.mark.parametrize("B,interval,n,kw", [(16, 1, 7, {}), (16, 3, 7, {}), (8, 3, 7, {}),
                                             (16, 2, 4, dict(diffaug="color,translation,cutout", ema_decay=0.999, spectral_norm="all"))])
def test_graph_replay_equals_eager_bitwise(B, interval, n, kw):
    """Two kinds of step, two captured graphs, each warmed up and captured when its kind first occurs (step 1: due; step 2: plain):
    losses, both masters and r1_loss equal the eager run's bit for bit; dropout 0.1 (the masks follow the device step counter)."""
    out = []
    for use_graph in (False, True):
        *res, eng, _, _ = _run(B, n, use_graph, r1_gamma=10.0, r1_interval=interval, **kw)
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None and int(eng.step_t) == n
        assert sorted(eng._graphs) == ([] if not use_graph else [True] if interval == 1 else [False, True])
        eng.close()
        out.append(res)
    for a, b, what in zip(out[0], out[1], ("losses", "D master", "G master", "r1_loss")):
        assert torch.equal(a, b), what
    assert float(out[0][3]) > 0


def test_resume_continues_the_lazy_schedule():
    """Interval 3: 4 steps, state_dict + the modules' weights into a fresh engine, 3 more steps (step 7 is due) - bit-equal to 7
    uninterrupted steps.  Other (gamma, interval) refuse a strict load; strict=False loads."""
    from vit_gan_amd.engine import GanEngine
    B = 8
    whole = _run(B, 7, False, r1_gamma=10.0, r1_interval=3)
    whole[4].close()
    *_, eng, D, G = _run(B, 4, False, r1_gamma=10.0, r1_interval=3)
    state = eng.state_dict()
    assert state["r1"] == (10.0, 3) and state["steps"] == 4
    first = (state, {k: v.clone() for k, v in D.state_dict().items()}, {k: v.clone() for k, v in G.state_dict().items()}, 4)
    eng.close()
    rest = _run(B, 3, False, first=first, r1_gamma=10.0, r1_interval=3)
    rest[4].close()
    assert torch.equal(rest[0], whole[0][4:]), "losses of steps 5-7"
    for i, what in ((1, "D master"), (2, "G master"), (3, "r1_loss")):
        assert torch.equal(rest[i], whole[i]), what
    for other in (dict(r1_gamma=10.0, r1_interval=2), dict(r1_gamma=5.0, r1_interval=3), {}):
        e2 = GanEngine(D, G, batch=B, external_noise=True, **other)
        with pytest.raises(ValueError, match="r1"):
            e2.load_state_dict(state)
        e2.load_state_dict(state, strict=False)
        assert e2.steps == 4
        e2.close()


def test_trainer_logs_and_saves_the_r1_options(tmp_path):
    from vit_gan_amd.training import train_model
    cfg = {"epochs": 1, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}
    out = train_model(cfg, r1_gamma=10, r1_interval=2, max_epochs=1, steps_per_epoch=3, output_base=str(tmp_path))
    d = out["dirs"]
    log = open(os.path.join(d.save, "training.log")).read()
    epoch_lines = [line for line in log.splitlines() if "Epoch [0/1]" in line]
    assert len(epoch_lines) == 1 and "| R1: " in epoch_lines[0], log
    assert "R1 penalty on real images: gamma 10" in log
    state = torch.load(os.path.join(d.save, "engine_state.pth"), map_location="cpu")
    assert state["r1"] == (10.0, 2) and state["steps"] == 3
    assert float(out["engine"].r1_loss) > 0
