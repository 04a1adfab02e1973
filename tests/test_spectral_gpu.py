"""Spectral normalisation on the GPU: vg_spectral_update / vg_spectral_project against the float64 restatement of tests/spectral_ref.py
inside its derived bounds, containment and reproducibility, and the engine with the option off and on - the normalised
trajectory, the step against a reference step composed from the step oracle's pieces, graph replay, resume, a one-rank RCCL group, the
exported checkpoint and the module-forward path.

Every test prints the worst observed fraction of its bounds with pytest -s.  These tests had not run on an MI355X when they were
written ("Spectral normalisation", says so): no device figures are recorded yet.
"""
import contextlib

import pytest
import torch

import engine_util as eu
import gpu_util
import spectral_ref as sr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EXTRA = [(10, 75), (7, 45)]  # K % 4 != 0: the 4-byte access path


def _pack(scale, start, seed=0):
    """Every shape in one flat buffer, with gaps between the matrices (one of them odd, so the last four matrices start off the
    16-byte grid).  Returns (state, flat, entries, u_in list, sigma0 list)."""
    from vit_gan_amd.spectral import SpectralState
    shapes = list(sr.SHAPES) + EXTRA
    entries, off, mats = [], 8, []
    for i, (N, K) in enumerate(shapes):
        entries.append((off, N, K))
        mats.append(sr.make_matrix(N, K, scale, seed))
        off += N * K + (5 if i == len(shapes) - 5 else 8)
    total = (off + 3) // 4 * 4
    flat = torch.zeros(total)
    for (o, N, K), W in zip(entries, mats):
        flat[o:o + N * K] = W.reshape(-1)
    st = SpectralState(entries, total, "cuda")
    assert st.entries == entries
    g = torch.Generator().manual_seed(11 + seed)
    us, s0s = [], []
    for i, W in enumerate(mats):
        uc, smax, _ = sr.top_pair(W)
        u = uc.float() if start == "converged" else torch.nn.functional.normalize(torch.randn(W.shape[0], generator=g), dim=0)
        st.u(i).copy_(u)
        st.sigma0(i).fill_(1.25 * smax)
        us.append(u)
        s0s.append(float(st.sigma0(i)))
    return st, flat.cuda(), mats, us, s0s


def _outside(st, total):
    keep = torch.ones(total, dtype=torch.bool)
    for off, N, K in st.entries:
        keep[off:off + N * K] = False
    return keep


@pytest.mark.parametrize("start", ["converged", "random"])
@pytest.mark.parametrize("scale", ["init", "trained"])
def test_operators_match_the_float64_restatement_and_touch_nothing_else(scale, start):
    st, flat, mats, us, s0s = _pack(scale, start)
    total = flat.numel()
    g = torch.Generator().manual_seed(3)
    guard_sh = torch.randint(-32768, 32767, (total + 64,), generator=g, dtype=torch.int16).cuda()
    grad_h = torch.randn(total + 64, generator=g) * 1e-3
    grad_h[32:32 + total] += 0.05 * flat.cpu()
    runs, state0 = [], st.state.clone()
    for _ in range(2):
        st.state.copy_(state0)
        st.scratch.fill_(float("nan"))  # nothing may depend on what the scratch held
        shadow = guard_sh.clone()
        grad = grad_h.cuda()
        sh_view = shadow[32:32 + total].view(BF)
        st.update(flat, sh_view)
        st.project(grad[32:32 + total], flat)
        torch.cuda.synchronize()
        runs.append((st.state.clone().cpu(), shadow.cpu(), grad.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), "two runs differ"
    state, shadow, grad = runs[0]
    # containment: the guards around the buffers and every element between the matrices are bit-identical
    keep = torch.ones(total + 64, dtype=torch.bool)
    keep[32:32 + total] = _outside(st, total)
    assert torch.equal(shadow[keep], guard_sh.cpu()[keep]), "the update wrote outside the normalised ranges of the shadow"
    assert torch.equal(grad[keep].view(torch.int32), grad_h[keep].view(torch.int32)), "the projection wrote outside the normalised ranges"
    worst = {}
    for i, ((off, N, K), W) in enumerate(zip(st.entries, mats)):
        d = st.table[i]
        v, u = state[d.v_off:d.v_off + K], state[d.u_off:d.u_off + N]
        sigma = float(state[d.s_off])
        assert float(state[d.s_off + 1]) == s0s[i]
        sh = shadow[32 + off:32 + off + N * K].view(BF).float().view(N, K)
        fr = sr.check_update(W, us[i], s0s[i], v, sigma, u, sh, f"{N}x{K} {scale} {start}")
        if N == 1:
            assert abs(sigma - float(W.double().norm())) <= 16 * sr.U32 * sigma
        # the shadow is bit for bit the bf16 cast of fp32(s * W) formed with torch's own (IEEE) division and product
        s = torch.tensor(s0s[i]) / torch.clamp(torch.tensor(sigma), min=1e-12)
        assert torch.equal((s * W).to(BF).view(torch.int16), sh.to(BF).view(torch.int16)), f"{N}x{K}: shadow != bf16(fp32(s) * W)"
        G = grad_h[32 + off:32 + off + N * K].view(N, K)
        fr["proj"] = sr.check_project(G, W, u, v, sigma, s0s[i], grad[32 + off:32 + off + N * K].view(N, K), f"{N}x{K} {scale} {start}")
        for k, f in fr.items():
            worst[k] = max(worst.get(k, 0.0), f)
    print(f"\n{scale} / {start}: worst fraction of each bound {({k: round(f, 3) for k, f in worst.items()})}")


def test_single_matrix_ops():
    from vit_gan_amd import ops
    W = sr.make_matrix(384, 192, "trained")
    u = torch.nn.functional.normalize(torch.randn(384, generator=torch.Generator().manual_seed(1)), dim=0)
    sigma, u1, v1 = ops.spectral_sigma(W.cuda(), u.cuda())
    G = torch.randn(384, 192, generator=torch.Generator().manual_seed(2))
    sh, sigma_b, u_b, v_b, proj = ops.spectral_normalize(W.cuda(), u.cuda(), 2.5, grad=G.cuda())
    assert torch.equal(sigma, sigma_b) and torch.equal(u1, u_b) and torch.equal(v1, v_b)
    sr.check_update(W, u, 2.5, v1.cpu(), float(sigma), u1.cpu(), sh.float().cpu(), "ops")
    sr.check_project(G, W, u1.cpu(), v1.cpu(), float(sigma), 2.5, proj.cpu(), "ops")
    refresh = torch.empty_like(sh)
    # iterate = 0: the same cast from the stored sigma
    from vit_gan_amd.ops import _spectral_one
    st = _spectral_one(W.cuda(), u1, 2.5)
    st.v(0).copy_(v1), st.sigma(0).copy_(sigma)
    before = st.state.clone()
    st.update(W.cuda().reshape(-1), refresh.reshape(-1), iterate=False)
    assert torch.equal(refresh.view(torch.int16), sh.view(torch.int16)) and torch.equal(before, st.state)


# ------------------------------------------------------------------------------------------------------------- the engine
def _engine(B, which, layers=2, full=False, seed=5, **kw):
    opts = dict(external_noise=True)
    opts.update(kw)
    if which is not None:
        opts["spectral_norm"] = which
    return eu.train_engine(B, seed, d_layers=layers, full=full, **opts)[:3]


def _steps(eng, n, B, each=None):
    return eu.run_steps(eng, eu.batches(B, n), each=each)


def test_option_off_is_the_plain_step():
    B, n = 4, 3
    a, _, _ = _engine(B, None)
    b, _, _ = _engine(B, "")
    assert b.spec is None and b.vit._flat.spectral is None and "spectral_state" not in b.state_dict()
    eu.assert_same_run(_steps(a, n, B), _steps(b, n, B), "spectral_norm=''")


@pytest.mark.parametrize("which,B,full", [("all", 16, False), ("qkv", 16, False), ("all", 256, True), ("qkv", 256, True)])
def test_engine_keeps_the_normalised_weights_inside_the_operator_bounds(which, B, full):
    """After each step: sigma and the shadow against the restatement fed the engine's own master and previous u; and
    sigma_max(shadow matrix) / sigma0 - 1 (true float64 SVD) against the restatement's own deviation under the same one-iteration
    schedule plus the shadow bound."""
    from vit_gan_amd.spectral import vit_matrix_keys
    eng, D, G = _engine(B, which, full=full, loss="wasserstein", clip_d=5.0, lr_d=2e-3 if not full else 5e-4)
    sp, fd = eng.spec, eng.vit._flat
    assert sp is not None and sp.n == len(vit_matrix_keys(eng.vit._dims.L, which)) and fd.spectral is sp
    # at construction: s = 1 exactly, the shadow is the plain cast
    assert torch.equal(fd.shadow.view(torch.int16), fd.flat.to(BF).view(torch.int16))
    plain_ranges = _outside(sp, fd.total)
    prev = {"u": [sp.u(i).cpu().clone() for i in range(sp.n)]}
    worst = {"sigma": 0.0, "shadow": 0.0, "dev_kernel": 0.0, "dev_ref": 0.0}

    def each(step):
        flat, shadow = fd.flat.detach().cpu(), fd.shadow.detach().cpu()
        assert torch.equal(shadow[plain_ranges].view(torch.int16), flat[plain_ranges].to(BF).view(torch.int16)), "biases / LayerNorm / pos / cls keep AdamW's cast"
        for i, (off, N, K) in enumerate(sp.entries):
            W = flat[off:off + N * K].view(N, K)
            sh = shadow[off:off + N * K].float().view(N, K)
            sigma, sigma0 = float(sp.sigma(i)), float(sp.sigma0(i))
            u_before = prev["u"][i]
            fr = sr.check_update(W, u_before, sigma0, sp.v(i).cpu(), sigma, sp.u(i).cpu(), sh, f"step {step} {sp.names[i]}")
            worst["sigma"], worst["shadow"] = max(worst["sigma"], fr["sigma"]), max(worst["shadow"], fr["shadow"])
            prev["u"][i] = sp.u(i).cpu().clone()
            # the normalisation itself.  The restatement, one iteration from the same previous u: its effective matrix has
            # sigma_max / sigma0 = smax / sig_ref.  The kernel's sigma differs from sig_ref by at most its own bound plus smax |v - v_ref|_2
            # (both in check_update.last), and the shadow from the exact effective matrix by the shadow bound, whose 2-norm is at most
            # (2^-8 + 2u) sigma_max(|W_eff|) (Weyl).
            _, sig_ref, _ = sr.power_step(W, u_before)
            smax = float(torch.linalg.svdvals(W.double())[0])
            dev_ref = abs(smax / sig_ref - 1.0)
            dev = abs(float(torch.linalg.svdvals(sh.double())[0]) / sigma0 - 1.0)
            ab = sr.check_update.last
            pert = (2.0 ** -8 + 2 * sr.U32) * float(torch.linalg.svdvals(sr.effective(W, sigma, sigma0).abs())[0]) / sigma0
            bound = dev_ref + smax * (ab["bs"] + smax * ab["bv2"]) / (sigma * sig_ref) + pert
            assert dev <= bound, (step, sp.names[i], dev, dev_ref, bound)
            worst["dev_kernel"], worst["dev_ref"] = max(worst["dev_kernel"], dev), max(worst["dev_ref"], dev_ref)

    assert torch.isfinite(_steps(eng, 3 if full else 4, B, each=each).losses).all()
    print(f"\n{which} B={B} full={full}: worst fraction of the sigma / shadow bound {worst['sigma']:.3f} / {worst['shadow']:.3f}; "
          f"|sigma_max(shadow) / sigma0 - 1| kernel {worst['dev_kernel']:.3e}, restatement {worst['dev_ref']:.3e}")
    eng.close()
    assert fd.spectral is None


class _Normalised:
    """StepHooks.weights of the normalised step.  oracle.d holds the RAW weights; D is evaluated on the effective ones (raw scaled in place
    around each pass), the restatement projects the accumulated gradients, AdamW acts on the raw weights, one restated power iteration
    follows, and the generator's pass sees the new effective weights.  ``s``: the scale in force, per key."""

    def __init__(self, keys, state):
        self.keys, self.state = keys, state
        self.s = {k: state[k]["sigma0"] / state[k]["sigma"] for k in keys}
        assert all(s == 1.0 for s in self.s.values())  # the first step: the effective weights ARE the raw ones, no rescaling error in the reference

    @contextlib.contextmanager
    def scaled(self, d):
        with torch.no_grad():
            for k, s in self.s.items():
                d[k].mul_(s)
        try:
            yield
        finally:
            with torch.no_grad():
                for k, s in self.s.items():
                    d[k].div_(s)

    def project(self, d):
        with torch.no_grad():
            for k in self.keys:  # dL/dW_eff -> dL/dW
                p, stt = d[k], self.state[k]
                N = p.shape[0]
                g2 = sr.project(p.grad.reshape(N, -1), p.detach().reshape(N, -1), stt["u"], stt["v"], stt["sigma"], stt["sigma0"])
                p.grad.copy_(g2.reshape(p.shape).to(p.dtype))

    def remeasure(self, d):
        for k in self.keys:
            p = d[k].detach()
            _, sigma, _ = sr.power_step(p.reshape(p.shape[0], -1), self.state[k]["u"])
            self.s[k] = self.state[k]["sigma0"] / sigma


@pytest.mark.parametrize("gp", [False, True])
def test_normalised_engine_step_matches_the_reference_step(gp):
    """losses and the first AdamW update at the tolerances of test_wasserstein_losses_and_gradient_clipping (its configuration plus the
    normalisation); with gp_weight = 10 and a fixed epsilon at those of test_engine_step_with_gradient_penalty (its configuration)"""
    from vit_gan_amd.engine import GanEngine
    B = 8
    D, G, oracle = eu.build(B, "wasserstein")
    if gp:
        oracle.gp_weight, oracle.clip_d = 10.0, 5.0
        eng = GanEngine(D, G, batch=B, loss="wasserstein", gp_weight=10.0, clip_d=5.0, external_noise=True, d_dropout=0.0, g_dropout=0.0,
                        spectral_norm="all")
    else:
        oracle.clip_d, oracle.clip_g, oracle.diversity_weight = 0.05, 0.02, 0.0
        eng = GanEngine(D, G, batch=B, loss="wasserstein", clip_d=0.05, clip_g=0.02, external_noise=True, d_dropout=0.0, g_dropout=0.0,
                        spectral_norm="all")
    sp = eng.spec
    keys = ["vit." + k for k in sp.names]
    state = {k: {"u": sp.u(i).cpu().double(), "v": sp.v(i).cpu().double(), "sigma": float(sp.sigma(i)), "sigma0": float(sp.sigma0(i))}
             for i, k in enumerate(keys)}
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    z = torch.randn(B, 1024, generator=g)
    eps = torch.rand(B, 1, 1, 1, generator=g)
    if gp:
        eng.gp_epsilon = eps.cuda()
    w0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    losses = eng.step(real.cuda(), z.cuda())
    torch.cuda.synchronize()
    from oracle.step_oracle import StepHooks
    weights = _Normalised(keys, state)
    ref = oracle.step(real.to(BF).float(), z, gp_epsilon=eps if gp else None, hooks=StepHooks(weights=weights))
    got = losses.cpu().tolist()
    print(f"normalised step (gp {gp}): engine {got} gp {float(eng.gp_loss):.5f}; reference {ref} gp {oracle.last_gp}")
    eu.assert_losses_match(got, ref, 2e-2)
    if gp:
        eu.assert_penalty_matches(float(eng.gp_loss), oracle.last_gp, 0.03, 1e-3)
    for k in ("vit.encoder.1.fc2.weight", "vit.encoder.0.attention.queries.weight"):
        eu.assert_first_update_matches(D, w0, oracle, k, 1.1e-3, 1e-4, 0.9)
    print("scale the generator's pass saw, engine - reference, worst:", max(abs(float(sp.scale(i)) - weights.s[k]) for i, k in enumerate(keys)))


def test_graph_replay_equals_eager_and_does_not_depend_on_host_synchronisation():
    """Three replays equal three eager steps bit for bit, state included.  And, as the hardening test of the gradient penalty asserts
    that its call left no memset node in the captured step: many replays with a host sync after every step against none at all give
    bit-identical weights - a memset or memcpy node in the graph is what broke that."""
    B, n = 4, 3

    def make(use_graph, which="all"):
        eng = _engine(B, which, use_graph=use_graph, loss="wasserstein", clip_d=5.0, gp_weight=10.0)[0]
        # a fixed epsilon: torch.rand's stream is not the same in a captured step (the graph-safe generator) as in an eager one
        eng.gp_epsilon = torch.rand(B, 1, 1, 1, generator=torch.Generator().manual_seed(2)).cuda()
        return eng
    runs, engines = eu.graph_against_eager(make, eu.batches(B, n))
    for eng in engines.values():
        assert any(t is eng.spec.state for t in eng._state_tensors())
        eng.close()
    assert not torch.equal(_steps(make(False, None), n, B).state[0], runs["eager"].state[0])  # the normalisation is really in the step
    out = []
    B = 64
    for sync_every_step in (False, True):
        eng, D, G = _engine(B, "all", use_graph=True, external_noise=False, loss="wasserstein", clip_d=5.0, gp_weight=10.0)
        gen = torch.Generator(device="cuda").manual_seed(1)
        reals = [torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1 for _ in range(4)]
        for i in range(150):
            eng.step(reals[i % 4])
            if sync_every_step or i == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert eng.graph_active
        out.append((eng.vit._flat.flat.detach().clone(), eng.vit._flat.shadow.detach().clone(), eng.spec.state.clone()))
        eng.close()
    assert torch.isfinite(out[0][0]).all()
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("use_graph", [False, True])
def test_resume_equals_the_uninterrupted_run(use_graph):
    B = 4
    kw = dict(use_graph=use_graph, loss="wasserstein", clip_d=5.0, ema_decay=0.999, diffaug="color,translation")
    _, _, _, st, made = eu.resume_against_whole(lambda **net: _engine(B, "all", **net, **kw), eu.batches(B, 6), 3)
    a, b = made[1][0], made[2][0]
    assert st["spectral_norm"] == "all" and st["spectral_state"].numel() == a.spec.state_floats
    # a state without the normalisation's: strict raises, non-strict measures again from the current weights
    bare = {k: v for k, v in st.items() if not k.startswith("spectral")}
    with pytest.raises(ValueError, match="spectral_state"):
        b.load_state_dict(bare)
    b.load_state_dict(bare, strict=False)
    assert all(float(b.spec.sigma(i)) == float(b.spec.sigma0(i)) for i in range(b.spec.n))
    assert torch.equal(b.vit._flat.shadow.view(torch.int16), b.vit._flat.flat.to(BF).view(torch.int16))
    off, _, _ = _engine(B, None)
    with pytest.raises(ValueError, match="spectral_norm off"):
        off.load_state_dict({**off.state_dict(), "spectral_norm": "all", "spectral_state": st["spectral_state"]})


def test_exported_checkpoint_and_module_forward():
    """effective_state_dict() in a plain ViTDiscriminator: the same shadow and the same eval logits, bit for bit; and a module forward
    of the engine's own discriminator leaves the normalised shadow in place (the refresh_shadow path)."""
    from vit_gan_amd import _lib
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    import ctypes as C
    B = 16
    eng, D, G = _engine(B, "all", loss="wasserstein", clip_d=5.0, lr_d=2e-3)
    _steps(eng, 4, B)
    fd = eng.vit._flat
    assert max(abs(float(eng.spec.scale(i)) - 1.0) for i in range(eng.spec.n)) > 1e-4  # the scales have moved
    trained = fd.shadow.clone()
    assert not torch.equal(trained.view(torch.int16), fd.flat.to(BF).view(torch.int16))
    imgs = (torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(BF).float().cuda()
    # the module-forward path: refresh_shadow() keeps the normalisation
    D.eval()
    with torch.no_grad():
        out_mod = D(imgs).float().clone()
    assert torch.equal(fd.shadow.view(torch.int16), trained.view(torch.int16)), "a module forward undid the normalisation"
    eng.sync_from_modules()
    assert torch.equal(fd.shadow.view(torch.int16), trained.view(torch.int16))
    D.load_state_dict(D.state_dict())  # the load_state_dict hook
    assert torch.equal(fd.shadow.view(torch.int16), trained.view(torch.int16))
    # the engine's own D forward on the same images (no dropout), through the C call the step uses
    ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(eng.vit._dims), B), dtype=torch.uint8, device="cuda")
    net = _lib.VgVitNet(eng.vit._dims, fd.flat.data_ptr(), fd.shadow.data_ptr(), fd.grad.data_ptr(), 0.0, 0, None, None, 0, 0)
    logits = torch.empty(B, 1, dtype=torch.float32, device="cuda")
    gpu_util.call("vg_vit_forward", C.byref(net), B, gpu_util.ptr(imgs), 0, gpu_util.ptr(ws), gpu_util.ptr(logits), gpu_util.stream())
    sd = eng.effective_state_dict()
    assert set(sd) == set(D.state_dict())
    plain = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, dropout_rate=0.1, batch_size=B, transformer_blocks_count=2)).cuda().eval()
    plain.load_state_dict(sd, strict=True)
    with torch.no_grad():
        out_plain = plain(imgs).float()
    assert plain.vit._flat.spectral is None
    assert torch.equal(plain.vit._flat.shadow.view(torch.int16), trained.view(torch.int16)), "bf16(effective) != the engine's shadow"
    torch.cuda.synchronize()
    assert torch.equal(out_plain.reshape(-1), logits.reshape(-1)) and torch.equal(out_mod.reshape(-1), logits.reshape(-1))
    # reset_optimizer measures again: the current weights become the reference point
    eng.sync_from_modules(reset_optimizer=True)
    assert torch.equal(fd.shadow.view(torch.int16), fd.flat.to(BF).view(torch.int16))


def _rccl_worker(rank, world):
    import vit_gan_amd  # noqa: F401
    B, res, ran = 16, [], []
    for use_graph, group in ((False, False), (False, True), (True, True)):
        kw = dict(exchange_single_rank=True) if group else {}
        eng, D, G = _engine(B, "all", use_graph=use_graph, loss="wasserstein", clip_d=5.0, **kw)
        assert eng.sync.active == group
        res.append(_steps(eng, 3, B))
        ran.append((eng.graph_active, eng.graph_fallback_reason))
        eng.close()
    for r in res[1:]:
        eu.assert_same_run(res[0], r, "one-rank group against no group")
    return ran[2]


@pytest.mark.timeout(300)
def test_one_rank_rccl_group_equals_the_single_process_engine():
    """exchange_single_rank=True (the staged backward and its all-reduces on a one-rank RCCL group), eager and captured, against the
    engine without a process group: bit-equal losses and state, the normalisation's included."""
    (val,) = eu.run_ranks(_rccl_worker, 1, 240, backend="nccl", gpu=True)
    assert val[0] and val[1] is None, val
