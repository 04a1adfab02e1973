"""Adaptive discriminator augmentation on the GPU: the gated augmentation kernels against the existing ones - bit for bit, image by
image, under each image's effective policy as tests/ada_ref.py restates it - the controller kernel against its numpy float32
restatement, and the engine with a fixed and with an adapted probability: trajectory, hipGraph replay, resume, and the defaults, which
must stay what they were.

No tolerance anywhere but one: r_last is one fp32 division (1 ulp)."""

import numpy as np
import pytest
import torch

import ada_ref as ar
import diffaug_ref as dr
import engine_util as eu
import gpu_util as u

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMETRIES = [(7, 3, 32), (5, 1, 32), (5, 3, 36), (5, 8, 9)]  # B, C, IH; 8 x 9 x 9: planes of 81 elements, the 2-byte access path
POLICY = "color,translation,cutout"


def _images(B, Cc, IH, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, Cc, IH, IH, generator=g) * 2 - 1).to(BF).cuda()


def _step(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _prob(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def _fwd(x, policy, seed, site, step, prob=None):
    """(y, params) of vg_diffaug_fwd, or of vg_diffaug_p_fwd when ``prob`` (a device tensor) is given; no synchronisation"""
    B, Cc, IH, _ = x.shape
    y = torch.full_like(x, float("nan"))
    params = torch.full((B, 8), float("nan"), dtype=torch.float32, device=x.device)
    if prob is None:
        u.call("vg_diffaug_fwd", u.ptr(x), u.ptr(y), u.ptr(params), B, Cc, IH, policy, seed, site, u.ptr(step), None)
    else:
        u.call("vg_diffaug_p_fwd", u.ptr(x), u.ptr(y), u.ptr(params), B, Cc, IH, policy, seed, site, u.ptr(step), u.ptr(prob), None)
    return y, params


def _bwd(dy, policy, seed, site, step, prob=None, into=None):
    B, Cc, IH, _ = dy.shape
    dx = torch.full_like(dy, float("nan")) if into is None else into.clone()
    if prob is None:
        u.call("vg_diffaug_bwd", u.ptr(dy), u.ptr(dx), int(into is not None), B, Cc, IH, policy, seed, site, u.ptr(step), None)
    else:
        u.call("vg_diffaug_p_bwd", u.ptr(dy), u.ptr(dx), int(into is not None), B, Cc, IH, policy, seed, site, u.ptr(step), u.ptr(prob), None)
    return dx


def _bits(t):
    return t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- the gated kernels
@pytest.mark.parametrize("B,Cc,IH", GEOMETRIES)
def test_p_one_is_the_existing_kernel_and_p_zero_a_copy(B, Cc, IH):
    x, w, old = _images(B, Cc, IH, 1), _images(B, Cc, IH, 2), _images(B, Cc, IH, 3)
    one, zero = _prob(1.0), _prob(0.0)
    plain_add = _bwd(w, 0, 31, 0, None, into=old)  # the existing kernel's bf16(old + dy)
    for policy in range(8):
        step = _step(10 + policy)
        y0, p0 = _fwd(x, policy, 31, 0, step)
        y1, p1 = _fwd(x, policy, 31, 0, step, one)
        assert _same(y1, y0) and torch.equal(p1, p0), f"forward, policy {policy}"
        assert _same(_bwd(w, policy, 31, 0, step, one), _bwd(w, policy, 31, 0, step)), f"adjoint, policy {policy}"
        assert _same(_bwd(w, policy, 31, 0, step, one, into=old), _bwd(w, policy, 31, 0, step, into=old)), f"accumulating adjoint, policy {policy}"
        yz, pz = _fwd(x, policy, 31, 0, step, zero)
        assert _same(yz, x), f"p = 0 is a bitwise copy, policy {policy}"
        assert np.array_equal(pz.cpu().numpy(), dr.draw(31, 0, 10 + policy, B, IH, 0))
        assert _same(_bwd(w, policy, 31, 0, step, zero), w) and _same(_bwd(w, policy, 31, 0, step, zero, into=old), plain_add)
    for bad in (float("nan"), -3.0):  # clamp: NaN and negatives switch everything off, anything above 1 everything on
        assert _same(_fwd(x, 7, 31, 0, _step(3), _prob(bad))[0], x)
    assert _same(_fwd(x, 7, 31, 0, _step(3), _prob(9.0))[0], _fwd(x, 7, 31, 0, _step(3))[0])


def _check_against_effective_policies(x, w, old, policy, seed, site, stepv, p):
    """every image of the gated launch == the same image of the existing kernel run under that image's effective policy"""
    B, _, IH, _ = x.shape
    step = None if stepv is None else _step(stepv)
    prob = _prob(p)
    y, params = _fwd(x, policy, seed, site, step, prob)
    dx, acc = _bwd(w, policy, seed, site, step, prob), _bwd(w, policy, seed, site, step, prob, into=old)
    eff = ar.gates(seed, site, stepv, B, policy, p)
    what = (policy, seed, site, stepv, B)
    assert np.array_equal(params.cpu().numpy()[:, 7], eff.astype(np.float32)), what
    assert np.array_equal(params.cpu().numpy(), ar.draw_p(seed, site, stepv, B, IH, policy, p)), what
    for q in np.unique(eff):
        rows = torch.from_numpy(eff == q).cuda()
        yq, _ = _fwd(x, int(q), seed, site, step)
        assert _same(y[rows], yq[rows]), (what, int(q), "forward")
        assert _same(dx[rows], _bwd(w, int(q), seed, site, step)[rows]), (what, int(q), "adjoint")
        assert _same(acc[rows], _bwd(w, int(q), seed, site, step, into=old)[rows]), (what, int(q), "accumulating adjoint")
    return eff


@pytest.mark.parametrize("B,Cc,IH", GEOMETRIES)
def test_p_half_every_policy(B, Cc, IH):
    x, w, old = _images(B, Cc, IH, 4), _images(B, Cc, IH, 5), _images(B, Cc, IH, 6)
    seen = set()
    for policy in range(8):
        seen |= set(_check_against_effective_policies(x, w, old, policy, 31, 0, 20 + policy, 0.5).tolist())
    assert len(seen) > 2  # really a mixture


@pytest.mark.parametrize("B", [1, 7, 256])
def test_p_half_seeds_sites_counters(B):
    x, w, old = _images(B, 3, 32, 7), _images(B, 3, 32, 8), _images(B, 3, 32, 9)
    counts = np.zeros(8, dtype=np.int64)
    for seed in (1, 0xDEADBEEFCAFEF00D):
        for site in (0, 1):
            for stepv in (1, 2, 70000):
                counts += np.bincount(_check_against_effective_policies(x, w, old, 7, seed, site, stepv, 0.5), minlength=8)
    _check_against_effective_policies(x, w, old, 5, 9, 1, None, 0.5)  # no device counter: the host key alone
    if B == 256:
        assert (counts > 0).all()  # 3072 images: every one of the eight effective policies occurs


def test_captured_launch_follows_the_device_probability():
    """ONE captured launch; prob_dev is rewritten between the replays and the effective policies follow it"""
    B, Cc, IH = 64, 3, 32
    x = _images(B, Cc, IH, 10)
    y, params = torch.empty_like(x), torch.zeros(B, 8, dtype=torch.float32, device="cuda")
    step, prob = _step(5), _prob(0.0)

    def launch():
        st = u.stream()
        u.call("vg_diffaug_p_fwd", u.ptr(x), u.ptr(y), u.ptr(params), B, Cc, IH, 7, 77, 0, u.ptr(step), u.ptr(prob), st)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()  # warm-up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    seen = []
    for p, stepv in ((0.0, 5), (0.5, 5), (1.0, 5), (0.25, 6), (0.5, 5)):
        prob.fill_(p)
        step.fill_(stepv)
        graph.replay()
        got = params.cpu().numpy()
        assert np.array_equal(got, ar.draw_p(77, 0, stepv, B, IH, 7, p)), (p, stepv)
        ref, _ = _fwd(x, 7, 77, 0, step, _prob(p))
        assert _same(y, ref)
        seen.append(got[:, 7].copy())
    assert (seen[0] == 0).all() and (seen[2] == 7).all() and np.array_equal(seen[1], seen[4]) and not np.array_equal(seen[1], seen[3])


# ---------------------------------------------------------------------------------------------------- the controller kernel
def _ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return bool(abs(int(a.view(np.int32)) - int(b.view(np.int32))) <= 1) or a == b


@pytest.mark.parametrize("n", [1, 7, 256, 1000])
def test_controller_kernel_equals_the_restatement(n):
    rng = np.random.default_rng(n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    target, spi, interval = np.float32(0.6), np.float32(1.0 / 4096), 4
    cases = 0
    for trial in range(6):
        lg = rng.standard_normal(n).astype(np.float32) + np.float32(rng.choice([-0.5, 0.0, 0.8]))
        k = min(n, len(special))
        lg[rng.choice(n, size=k, replace=False)] = special[:k]
        for stepv in (1, 3, 4, 8, 70000, 70001):  # firing (4, 8, 70000) and not
            st0 = np.array([rng.random(), rng.integers(-50, 50), rng.integers(50, 100), rng.standard_normal()], dtype=np.float32)
            if trial == 0:
                st0[0] = np.float32([0.0, 1.0, 0.999, 0.001, 0.5, 0.25][cases % 6])  # the clamps from both sides
            state, logits, step = torch.from_numpy(st0.copy()).cuda(), torch.from_numpy(lg).cuda(), _step(stepv)
            u.call("vg_ada_update", u.ptr(logits), n, u.ptr(state), float(target), float(spi), interval, u.ptr(step), None)
            got, want = state.cpu().numpy(), ar.controller(st0, lg, target, spi, interval, stepv)
            assert np.array_equal(got[:3].view(np.int32), want[:3].view(np.int32)), (n, trial, stepv, st0, got, want)
            assert _ulp_apart(got[3], want[3]), (n, trial, stepv, got, want)
            fired = stepv % interval == 0
            assert (got[1] == 0 and got[2] == 0) == fired or (st0[2] + n == 0)
            if not fired:
                assert got[0] == st0[0] and got[3] == st0[3]
            cases += 1
    # exactly on target: one multiply and one subtract see 0 where a fused multiply-add would not
    st0 = np.array([0.5, 0, 0, 0], dtype=np.float32)
    lg = np.array([1.0] * 4 + [-1.0], dtype=np.float32)  # acc_sign 3, acc_count 5, target 0.6f: fl(0.6f * 5) = 3 exactly
    state = torch.from_numpy(st0.copy()).cuda()
    u.call("vg_ada_update", u.ptr(torch.from_numpy(lg).cuda()), 5, u.ptr(state), float(target), float(spi), 1, u.ptr(_step(1)), None)
    want = ar.controller(st0, lg, target, spi, 1, 1)
    assert want[0] == np.float32(0.5) and np.array_equal(state.cpu().numpy()[:3], want[:3])


# --------------------------------------------------------------------------------------------------------------- the engine
B_ENG, KIMG, TARGET = 8, 0.064, 0.6  # 16 real images per update, 1 / (1000 * 0.064) per image: p moves by 0.25 per update
ADA = dict(diffaug=POLICY, aug_p=0.5, ada_target=TARGET, ada_interval=2, ada_kimg=KIMG)


def _data(i, B):
    g = torch.Generator().manual_seed(1000 + i)
    return (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda(), torch.randn(B, 1024, generator=g).cuda()


def _steps(eng, n, B, first=0, each=None):
    losses = []
    for i in range(first, first + n):
        losses.append(eng.step(*_data(i, B)).clone())
        if each is not None:
            torch.cuda.synchronize()
            each(i)
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), [t.detach().clone().cpu() for t in eng._state_tensors()]


def _engine(**kw):
    return eu.bench_like(B_ENG, **kw)


def test_engine_trajectory_is_the_restatement():
    """(a) six steps: D's site draws its gates at the p in force when the step began, the generator's site at the p behind the
    controller's launch of the same step, and (p, acc_sign, acc_count) follow ada_ref.controller fed the engine's own real logits"""
    eng, _, _, _ = _engine(**ADA)
    B = B_ENG
    spi = np.float32(eng.ada_step_per_image)
    assert spi * np.float32(2 * B) == np.float32(0.25)
    st = np.array([0.5, 0, 0, 0], dtype=np.float32)
    assert np.array_equal(eng.ada_state.cpu().numpy(), st) and eng.ada_p == 0.5
    ps = []

    def each(i):
        nonlocal st
        t = i + 1  # the device counter of this step
        assert int(eng.step_t) == t
        p_before = st[0]
        st = ar.controller(st, eng.logits[:B].cpu().numpy(), np.float32(TARGET), spi, 2, t)
        got = eng.ada_state.cpu().numpy()
        assert np.array_equal(got[:3].view(np.int32), st[:3].view(np.int32)), (t, got, st)
        assert _ulp_apart(got[3], st[3]), (t, got, st)
        st[3] = got[3]
        assert np.array_equal(eng.aug_params["d"].cpu().numpy(), ar.draw_p(eng._aug_seed, 0, t, 2 * B, 32, 7, p_before)), t
        assert np.array_equal(eng.aug_params["g"].cpu().numpy(), ar.draw_p(eng._aug_seed, 1, t, B, 32, 7, st[0])), t
        assert np.array_equal(eng.aug_params["d"].cpu().numpy()[:, 7], ar.gates(eng._aug_seed, 0, t, 2 * B, 7, p_before).astype(np.float32))
        ps.append(float(st[0]))
    losses, _ = _steps(eng, 6, B, each=each)
    assert torch.isfinite(losses).all()
    assert ps[0] == 0.5 and ps[1] != 0.5 and ps[1] == ps[2] and len(set(ps)) >= 2, ps  # moves on steps 2, 4, 6 only
    assert all(abs(b - a) in (0.0, 0.25) for a, b in zip(ps, ps[1:])), ps
    assert eng.ada_p == ps[-1] and -1.0 <= eng.ada_rt <= 1.0


def test_engine_graph_replay_equals_eager():
    """(b) three replays == three eager steps, bit for bit, the probability moving in between (no recapture, no host round trip)"""
    runs = {}
    for name, use_graph in (("eager", False), ("graph", True)):
        eng, _, _, _ = _engine(use_graph=use_graph, **ADA)
        ps = []
        runs[name] = _steps(eng, 3, B_ENG, each=lambda i: ps.append(eng.ada_p)) + (ps,)
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None and int(eng.step_t) == 3
    assert torch.isfinite(runs["eager"][0]).all() and runs["eager"][2][0] != runs["eager"][2][1], runs["eager"][2]
    assert runs["graph"][2] == runs["eager"][2]
    assert torch.equal(runs["graph"][0], runs["eager"][0])
    for i, (a, b) in enumerate(zip(runs["graph"][1], runs["eager"][1])):
        assert torch.equal(a, b), f"state tensor {i} of the replayed steps differs from the eager run"


def test_engine_resume_equals_the_uninterrupted_run():
    """(c) 3 steps, save, rebuild, load, 3 more == 6 uninterrupted, the controller's state included"""
    eng, _, _, _ = _engine(**ADA)
    whole = _steps(eng, 6, B_ENG)
    eng.close()
    a, D1, G1, _ = _engine(**ADA)
    first = _steps(a, 3, B_ENG)
    nets, st = (D1.state_dict(), G1.state_dict()), a.state_dict()
    assert tuple(st["ada"]) == (0.5, TARGET, 2, KIMG) and st["ada_state"][2] == B_ENG  # mid-window: one step accumulated
    a.close()
    b, D2, G2, _ = _engine(seed=99, **ADA)  # other initial weights: everything comes from the saved state
    D2.load_state_dict(nets[0]), G2.load_state_dict(nets[1])
    b.load_state_dict(st)
    second = _steps(b, 3, B_ENG, first=3)
    assert torch.equal(torch.cat([first[0], second[0]]), whole[0])
    for i, (x, y) in enumerate(zip(second[1], whole[1])):
        assert torch.equal(x, y), f"state tensor {i}"
    # other options are refused under strict, as bCR's are
    for other in ((0.5, TARGET, 4, KIMG), None):
        with pytest.raises(ValueError, match="ada_target"):
            b.load_state_dict({**st, "ada": other})
    b.load_state_dict({**st, "ada": (0.5, TARGET, 4, KIMG)}, strict=False)
    off, _, _, _ = _engine(diffaug=POLICY)
    with pytest.raises(ValueError, match="ada_target"):
        off.load_state_dict({**off.state_dict(), "ada": st["ada"], "ada_state": st["ada_state"]})


def _weights(eng):
    return eng.vit._flat.flat.detach().clone().cpu(), eng.gen._flat.flat.detach().clone().cpu()


def test_fixed_probabilities_one_and_zero_and_the_defaults():
    """(d) aug_p = 1 without ADA == the plain diffaug engine; (e) aug_p = 0 == the engine without diffaug; (f) the defaults hold no
    state of the feature and save the keys they saved before"""
    def run(**kw):
        eng, _, _, _ = _engine(**kw)
        losses, _ = _steps(eng, 2, B_ENG)
        return eng, losses, _weights(eng)
    plain, l_plain, w_plain = run(diffaug=POLICY)
    one, l_one, w_one = run(diffaug=POLICY, aug_p=1.0)
    assert one.gated and not one.ada and plain.ada_state is None
    assert torch.equal(l_one, l_plain) and torch.equal(w_one[0], w_plain[0]) and torch.equal(w_one[1], w_plain[1])
    bare, l_bare, w_bare = run()
    zero, l_zero, w_zero = run(diffaug=POLICY, aug_p=0.0)
    assert torch.equal(l_zero, l_bare) and torch.equal(w_zero[0], w_bare[0]) and torch.equal(w_zero[1], w_bare[1])
    assert not torch.equal(w_plain[0], w_bare[0])  # the augmentation is in the step at all
    for eng in (plain, bare):  # (f)
        assert eng.ada_state is None and not eng.gated and not eng.ada and not hasattr(eng, "logits_g")
        assert set(eng.state_dict()) == {"format_version", "steps", "noise_seed", "m_d", "v_d", "m_g", "v_g", "step_t"}
        with pytest.raises(RuntimeError, match="aug_p"):
            eng.ada_p
    assert set(one.state_dict()) - set(plain.state_dict()) == {"ada", "ada_state"}


def test_ada_with_consistency_regularisation():
    """(g) bCR + ADA: two eager steps == two replays, all losses finite; the partner T_1(x) is the gated transform: the one site-0
    launch, drawn at the probability in force when the step began, written behind x in the 4B buffer.  (The generator's pass of the
    same step reuses those rows for T_2(fake) and its gradient, so after a step the partner is checked by its recorded parameters,
    as test_bcr_gpu.py does for the plain diffaug partner; that an image with all gates off is a bitwise copy is the kernel tests'.)"""
    kw = dict(bcr=(10.0, 10.0), **{**ADA, "ada_interval": 1})
    runs = {}
    B = B_ENG
    for name, use_graph in (("eager", False), ("graph", True)):
        eng, _, _, _ = _engine(use_graph=use_graph, **kw)
        assert eng.imgs_aug.data_ptr() == eng.imgs4[2 * B:].data_ptr() and eng.imgs.data_ptr() == eng.imgs4.data_ptr()
        assert "c" not in eng.aug_params  # no launch of the partner's own
        cr, ps = [], [np.float32(0.5)]

        def each(i):
            cr.append(eng.bcr_losses.cpu().clone())
            assert np.array_equal(eng.aug_params["d"].cpu().numpy(), ar.draw_p(eng._aug_seed, 0, i + 1, 2 * B, 32, 7, ps[-1])), (name, i)
            ps.append(np.float32(eng.ada_p))
        runs[name] = _steps(eng, 2, B, each=each) + (torch.stack(cr),)
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None
        assert eng.logits.shape == (4 * B, 1) and abs(float(ps[1]) - 0.5) == 0.125, ps  # interval 1: the first step moves p, by 8 images' worth
    assert torch.isfinite(runs["eager"][0]).all() and torch.isfinite(runs["eager"][2]).all()
    assert torch.equal(runs["graph"][0], runs["eager"][0]) and torch.equal(runs["graph"][2], runs["eager"][2])
    for i, (a, b) in enumerate(zip(runs["graph"][1], runs["eager"][1])):
        assert torch.equal(a, b), f"state tensor {i}"


def test_autograd_operator_with_p():
    from vit_gan_amd import ops
    B, Cc, IH = 6, 3, 32
    x, w = _images(B, Cc, IH, 11).requires_grad_(True), _images(B, Cc, IH, 12)
    step, prob = _step(5), _prob(0.5)
    y = ops.diff_augment(x, POLICY, 12, 1, step, p=prob)
    assert _same(y.detach(), _fwd(x.detach(), 7, 12, 1, step, prob)[0])
    want = _bwd(w, 7, 12, 1, step, _prob(0.5))
    prob.fill_(1.0)  # the backward uses the probability of its forward
    (gx,) = torch.autograd.grad(y, x, w)
    assert _same(gx, want)
    assert _same(ops.diff_augment(x.detach(), POLICY, 12, 1, step, p=0.5), y.detach())
    assert _same(ops.diff_augment(x.detach(), POLICY, 12, 1, step, p=None), _fwd(x.detach(), 7, 12, 1, step)[0])
