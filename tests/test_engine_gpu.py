"""GanEngine (fast path) and the nn.Module drop-in path against the fp32 CPU step oracle."""
import numpy as np
import pytest
import torch

import engine_util as eu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("loss", ["ns", "hinge"])
@pytest.mark.parametrize("fuse", [True, False])
def test_engine_step_matches_oracle(loss, fuse):
    from vit_gan_amd.engine import GanEngine

    B = 8
    D, G, oracle = eu.build(B, loss)
    eng = GanEngine(D, G, batch=B, loss=loss, fuse_real_fake=fuse)
    # hinge: not seed 0 - with it every fake logit of step 0 sits below -1, the fake half's gradient is EXACTLY zero, most of D's first
    # AdamW step is lr * sign(rounding noise), and the step-1 generator loss is decided by that noise: 0.017-0.052 off the oracle across
    # schedules and kernel versions (tools/micro/step_dev.py), against 0.001-0.005 for every other seed and for the ns loss
    g = torch.Generator().manual_seed(0 if loss == "ns" else 1)
    for it in range(2):
        real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
        losses = eng.step(real.cuda())
        torch.cuda.synchronize()
        z = eng.z.detach().cpu().clone()  # the noise the engine drew
        ref = oracle.step(real, z)
        got = losses.cpu().tolist()
        # step 0: same weights, bf16 vs fp32 forward -> |dloss| < 2e-2.  step 1: each net has taken one
        # AdamW step whose per-weight direction is sign(g) (noise-level gradients may flip) -> 4e-2.
        tol = 2e-2 if it == 0 else 4e-2
        assert abs(got[0] - ref["d_real"]) < tol and abs(got[1] - ref["d_fake"]) < tol and abs(got[2] - ref["g"]) < tol, (got, ref)
    # after two AdamW steps the weights must track the oracle: AdamW moves each weight by ~lr per
    # step whatever the gradient scale, so compare the UPDATE direction on well-conditioned tensors
    sd = {k: v.detach().cpu() for k, v in D.state_dict().items()}
    for k in ("vit.encoder.1.fc2.weight", "vit.encoder.0.attention.values.weight", "vit.classifier.fc1.weight"):
        ref_w = oracle.d[k].detach()
        # Adam's first steps move every weight by ~lr*sign(g): a sign flip on a noise-level gradient
        # costs 2*lr per step, so the bound is 2 steps * 2 * 5e-4; most weights must agree closely
        assert float((sd[k] - ref_w).abs().max()) < 2.1e-3, k
        agree = float(((sd[k] - ref_w).abs() < 2e-4).float().mean())
        assert agree > 0.9, (k, agree)


def test_module_path_matches_engine_path():
    """Drop-in nn.Module usage (the reference loop's calls) gives the same gradients as GanEngine's C calls."""
    import torch.nn.functional as F
    B = 4
    D, G, oracle = eu.build(B)
    real = (torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    z = torch.randn(B, 1024, generator=torch.Generator().manual_seed(2)).cuda()
    D.zero_grad()
    out = D(real)
    assert out.shape == (B, 1) and out.dtype == torch.float32
    F.binary_cross_entropy_with_logits(out, torch.ones_like(out)).backward()
    fake = G(z)
    assert fake.shape == (B, 3, 32, 32)
    F.binary_cross_entropy_with_logits(D(fake.detach()), torch.zeros(B, 1, device="cuda")).backward()
    gD = {k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()}
    G.zero_grad()
    F.binary_cross_entropy_with_logits(D(fake), torch.ones(B, 1, device="cuda")).backward()
    gG = {k: p.grad.detach().cpu().clone() for k, p in G.named_parameters()}
    # oracle gradients for the same two D passes / one G pass
    for p in oracle.d.values():
        p.grad = None
    F.binary_cross_entropy_with_logits(oracle.D(real.cpu()), torch.ones(B, 1)).backward()
    fk = oracle.G(z.cpu())
    F.binary_cross_entropy_with_logits(oracle.D(fk.detach()), torch.zeros(B, 1)).backward()
    for k in ("vit.encoder.1.fc1.weight", "vit.embedding.conv1.weight", "vit.encoder.0.norm1.weight", "vit.classifier.fc2.bias"):
        ref = oracle.d[k].grad
        err = float((gD[k] - ref).abs().max()) / float(ref.abs().max())
        assert err < 2.0 ** -4, (k, err)
    for p in oracle.d.values():
        p.grad = None
    F.binary_cross_entropy_with_logits(oracle.D(fk), torch.ones(B, 1)).backward()
    for k in ("output_network.1.linear.weight", "mapping_mlp.model.0.0.bias", "transformer_layers.1.mlp.model.0.0.weight"):
        ref = oracle.g[k].grad
        err = float((gG[k] - ref).abs().max()) / float(ref.abs().max())
        assert err < 0.15, (k, err)


def test_dropout_path_and_state_dict_roundtrip():
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator

    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=128, transformer_blocks_count=2)).cuda()  # dropout 0.1, K=10
    x = torch.randn(3, 3, 32, 32, device="cuda")
    D.train()
    y = D.vit.composed_forward(x)  # per-operator HIP path with torch's nn.Dropout
    assert y.shape == (3, 10) and torch.isfinite(y).all()
    y.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in D.parameters())
    D.eval()
    with torch.no_grad():
        y0 = D(x)  # fused engine path
    sd = {k: v.clone() for k, v in D.state_dict().items()}
    D2 = ViTDiscriminator(Config(embeddings_dimension=128, transformer_blocks_count=2)).cuda().eval()
    D2.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert torch.equal(D2(x), y0)
    # composed path in eval mode == fused path within bf16 tolerance
    from vit_gan_amd import ops
    v = D.vit
    h = v.embedding(x)
    for blk in v.encoder:
        h = blk(h)
    h = ops.layer_norm(h[:, :1, :], v.norm.weight, v.norm.bias, v.norm.eps)
    yc = v.classifier(h)
    assert float((yc - y0).abs().max()) < 2.0 ** -5 * float(y0.abs().max()) + 1e-3


def test_engine_graph_replay_equals_eager():
    """hipGraph replay (what bench.py times at N=1) against the eager enqueue of the same steps: every piece of training
    state - both master weight buffers, both bf16 shadows, all four AdamW moment buffers, the step counter - and the
    losses of all three steps must be BIT-equal (the kernels are deterministic; N calls of step() are N steps in both
    modes).  The schedule with the weight gradients on a side stream (eager and captured) must give the same bits as the
    single-stream one bench.py runs."""
    B, n = 4, 3
    runs = {}
    for name, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True)),
                     ("eager_side_stream", dict(use_graph=False, concurrent_wgrad=True)),
                     ("graph_side_stream", dict(use_graph=True, concurrent_wgrad=True))):
        eng, D, G, _ = eu.bench_like(B, **kw)
        assert eng.p_d == 0.1 and eng.p_g == 0.2 and eng.fuse
        runs[name] = eu.run_steps(eng, eu.batches(B, n))
        assert eng.steps == n and int(eng.step_t) == n, (name, eng.steps, int(eng.step_t))
    ref = runs["eager"]
    assert torch.isfinite(ref.losses).all() and float(ref.state[0].abs().sum()) > 0
    for name in ("graph", "eager_side_stream", "graph_side_stream"):
        eu.assert_same_run(runs[name], ref, f"{name} against the eager run")


def _step_masks(u, eng, B, step):
    """The dropout multipliers the engine's step `step` (1-based device counter) applies, extracted through
    vg_dropout_apply with the same (seed, site, step) key material: pass A = fused [real ; fake], C = G's pass through
    D, and the generator's own sites."""
    d, g = eng.vit._dims, eng.gen._dims
    S = (d.IH // d.P) ** 2 + 1
    st = torch.tensor([step], dtype=torch.int32, device="cuda")

    def mask(shape, p, seed, site):
        out = u.dropout_mask(shape, p, seed, site, st)
        # bf16(keep-scale) -> the exact fp32 multiplier 256 / (256 - round(256 p)) the fused epilogues apply
        return (out > 0).float() * (256.0 / (256.0 - round(p * 256)))

    def vit_masks(n_img, seed):
        m = {"embed": mask((n_img, S, d.E), eng.p_d, seed, 0)}
        for l in range(d.L):
            m[("attn", l)] = mask((n_img, S, d.E), eng.p_d, seed, 1 + 2 * l)
            m[("mlp", l)] = mask((n_img, S, d.E), eng.p_d, seed, 2 + 2 * l)
        return m
    gm = {}
    for l in range(g.L):
        gm[("attn", l)] = mask((B, g.T, g.E), eng.p_g, eng.seed * 8 + 7, 100 + 2 * l)
        gm[("mlp", l)] = mask((B, g.T, g.E), eng.p_g, eng.seed * 8 + 7, 101 + 2 * l)
    if eng.two_stream:  # separate real / fake passes (seeds +0 / +1), the generator's pass through D as two half-batches (+2 / +3)
        lo, hi = vit_masks(B // 2, eng.seed * 8 + 2), vit_masks(B // 2, eng.seed * 8 + 3)
        return {"d_real": vit_masks(B, eng.seed * 8 + 0), "d_fake": vit_masks(B, eng.seed * 8 + 1),
                "d_gen": {k: torch.cat([lo[k], hi[k]], dim=0) for k in lo}, "g": gm}
    a = vit_masks(2 * B, eng.seed * 8 + 0)
    return {"d_real": {k: v[:B] for k, v in a.items()}, "d_fake": {k: v[B:] for k, v in a.items()},
            "d_gen": vit_masks(B, eng.seed * 8 + 2), "g": gm}


def test_benchmarked_configuration_matches_the_step_model():
    """The step bench.py measures - hipGraph replay + fused real/fake pass + two-stream weight gradients + train-mode
    dropout - against the rounding-faithful step model (oracle.step_oracle, faithful=True) fed the SAME noise and the
    SAME dropout masks: losses of two consecutive steps and the weights after them."""
    import gpu_util as u
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo
    B = 8
    eng, D, G, (d_state, g_state) = eu.bench_like(B, use_graph=True)
    model = so.GanStepOracle(d_state, g_state, vo.VitDims(layers=2, classes=1), go.GenDims(layers=2), faithful=True)
    loose = so.GanStepOracle(d_state, g_state, vo.VitDims(layers=2, classes=1), go.GenDims(layers=2))
    g = torch.Generator().manual_seed(9)
    w0 = {k: v.clone() for k, v in d_state.items()}
    for it in range(2):
        real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
        z = torch.randn(B, 1024, generator=g)
        got = eng.step(real.cuda(), z.cuda()).cpu().tolist()
        torch.cuda.synchronize()
        masks = _step_masks(u, eng, B, it + 1)
        ref = model.step(real, z, masks=masks)
        ref32 = loose.step(real, z, masks=masks)
        print(f"step {it}: engine {[round(x, 5) for x in got]} model {ref} fp32 {ref32}")
        for x, k in zip(got, ("d_real", "d_fake", "g")):
            # step 0 starts from identical weights: the rounding-faithful model predicts the losses to ~2e-4 (the fp32
            # oracle to ~1e-3).  Step 1 follows one AdamW update of every weight by +-lr, in which any two bf16
            # implementations disagree on the sign of noise-level gradients: loose tier for both references.
            assert abs(x - ref[k]) < (1e-3 if it == 0 else 4e-2), (it, k, got, ref)
            assert abs(x - ref32[k]) < (2e-2 if it == 0 else 4e-2), (it, k, got, ref32)
    # after two AdamW steps: each weight moved by ~lr per step in the direction of its gradient's sign, so the engine and
    # the model agree except where a gradient is at rounding-noise level (a flipped sign costs 2 lr per step)
    sd = {k: v.detach().cpu() for k, v in D.state_dict().items()}
    for k in ("vit.encoder.1.fc2.weight", "vit.encoder.0.attention.values.weight", "vit.classifier.fc1.weight", "vit.embedding.conv1.weight"):
        ref_w = model.d[k].detach()
        diff = (sd[k] - ref_w).abs()
        moved = float((ref_w - w0[k]).abs().mean())
        assert moved > 2e-4, (k, moved)
        assert float(diff.max()) < 2.1e-3, k
        agree = float((diff < 5e-5).float().mean())
        print(f"{k}: {agree:.4f} of the weights within 5e-5 of the model after 2 steps (mean |update| {moved:.2e})")
        assert agree > 0.8, (k, agree)   # measured 0.87-0.93: the rest are sign flips of noise-level gradients


def test_load_state_dict_after_engine_construction_refreshes_the_shadows():
    """load_state_dict copies into the flat master buffers in place; without a refresh the next step's
    discriminator / generator passes would read the stale bf16 shadows.  One step after a late load must equal, bit for
    bit, the step of an engine built after the load."""
    from vit_gan_amd.modules import ViTGAN
    B = 4
    eng_a, D_a, G_a, _ = eu.bench_like(B, seed=5, use_graph=False)
    eng_b, D_b, G_b, (d_other, g_other) = eu.bench_like(B, seed=6, use_graph=False)   # different weights
    assert not torch.equal(D_a.vit._flat.flat, D_b.vit._flat.flat)
    D_a.load_state_dict(d_other, strict=True)       # late load: engine A existed already
    G_a.load_state_dict(g_other, strict=True)
    eu.assert_same_run(eu.run_steps(eng_a, eu.batches(B, 1)), eu.run_steps(eng_b, eu.batches(B, 1)), "late load")
    seed_before = eng_a._noise_seed
    eng_a.sync_from_modules(reset_optimizer=True)
    assert int(eng_a.step_t) == 0 and float(eng_a.m_d.abs().sum()) == 0.0
    assert eng_a._noise_seed != seed_before, "a restarted run would replay the first run's latent sequence (ADVICE r3)"


def _dp_worker(rank, world):
    """on gloo, which moves CUDA tensors through the host: lets two ranks share the one GPU of the test box"""
    import torch.distributed as dist
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    B = 4

    def run(dp_chunks, compress, shard=False, ref_master=None):
        torch.manual_seed(0)  # identical init on every rank (and for every exchange variant)
        D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, dropout_rate=0.1, batch_size=B,
                                    transformer_blocks_count=4)).cuda().train()
        G = SirenGenerator(embed=128, layers=3, siren_hidden=256).cuda().train()
        eng = GanEngine(D, G, batch=B, seed=100 + rank, compress_mapping_grad=compress, shard_mapping_update=shard)
        eng.dp_chunks = dp_chunks
        assert eng.world == world and eng.sync.overlap and eng.shard_map == shard
        torch.manual_seed(50 + rank)  # different data / noise per rank
        for _ in range(3):
            real = torch.rand(B, 3, 32, 32, device="cuda") * 2 - 1
            losses = eng.step(real)
        torch.cuda.synchronize()
        before = G._flat.flat.detach().cpu().clone()
        if shard:
            w0, w1 = eng._map_range()
            a_, b_ = eng.sync.share(w0, w1)
            own = torch.zeros(w1 - w0, dtype=torch.bool)
            own[a_ - w0:b_ - w0] = True
            # the shares this rank does not own are already current - equal to the replicated update's - with no gather_master() call
            assert torch.equal(before[w0:w1][~own], ref_master[w0:w1][~own]) and torch.equal(before[w0:w1][own], ref_master[w0:w1][own])
        eng.gather_master()  # a no-op kept for callers: it must change nothing
        assert torch.equal(before, G._flat.flat.detach().cpu())
        return (D.vit._flat.flat.detach().cpu(), G._flat.flat.detach().cpu(), D.vit._flat.grad.detach().cpu(), losses.cpu(),
                G._flat.grad.detach().cpu(), G._flat.shadow.detach().cpu())
    # hipGraph replay cannot capture a gloo exchange: the engine must say so and run eager, never silently
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.manual_seed(0)
        Dg = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, batch_size=B, transformer_blocks_count=1)).cuda().train()
        Gg = SirenGenerator(embed=128, layers=1, siren_hidden=256).cuda().train()
        eg = GanEngine(Dg, Gg, batch=B, use_graph=True)
    assert not eg.graph_active and "gloo" in (eg.graph_fallback_reason or ""), eg.graph_fallback_reason
    assert any("runs EAGER" in str(w_.message) for w_ in caught)
    assert torch.isfinite(eg.step(torch.rand(B, 3, 32, 32, device="cuda") * 2 - 1)).all()
    del eg, Dg, Gg
    w, gw, gsum, losses, ggrad, gsh = run(3, False)    # D and G backward in 3 pieces, exchange overlapped
    w1, gw1, _, _, ggrad1, _ = run(1, False)           # one all-reduce per network after its whole backward
    w2, gw2, _, _, ggrad2, _ = run(3, True)            # + mapping-layer gradient exchanged as bf16
    w3, gw3, _, _, _, gsh3 = run(3, False, shard=True, ref_master=gw)  # mapping layer: reduce-scatter, AdamW on this rank's share, all-gather of the master
    gather = [None] * world
    dist.all_gather_object(gather, (w, gw, gsum, losses, gw2, gsh3, gw3))
    if rank == 0:
        ok = all(torch.equal(gather[0][0], g[0]) and torch.equal(gather[0][1], g[1]) and torch.equal(gather[0][2], g[2])
                 and torch.equal(gather[0][4], g[4]) for g in gather[1:])
        fin = all(torch.isfinite(g[3]).all() for g in gather) and torch.isfinite(w).all()
        differ = not torch.equal(gather[0][3], gather[1][3])  # different shards -> different local losses
        staged_equal = torch.equal(w, w1) and torch.equal(gw, gw1) and torch.equal(ggrad, ggrad1)
        # sharded update: replicas' bf16 shadows bit-identical after 3 steps, the gathered fp32 master bit-identical between the ranks,
        # and equal to the replicated update's (two ranks: a + b is the same sum in either exchange) - weights of D untouched by it
        sharded_ok = (all(torch.equal(gather[0][5], g[5]) and torch.equal(gather[0][6], g[6]) for g in gather[1:])
                      and torch.equal(gw3, gw) and torch.equal(gsh3, gsh) and torch.equal(w3, w))
        # bf16 exchange of the mapping gradient: same update direction for all but noise-level entries
        rel = float((ggrad2 - ggrad).abs().max()) / float(ggrad.abs().max())
        compressed_close = rel < 2.0 ** -7 and float((gw2 - gw).abs().max()) < 3.1e-3 and not torch.equal(ggrad2, ggrad)
        return ok, bool(fin), differ, staged_equal, compressed_close, rel, sharded_ok


@pytest.mark.timeout(600)
def test_two_rank_data_parallel_engine_with_current_sharded_master_on_one_gpu():
    """world_size 2 through the real engine path (staged D and G backward + overlapped ranged all-reduce on a side
    stream + 1/world folded into AdamW): replicas must stay bit-identical, gradients must be the all-reduced sum; the
    staged exchange must equal one all-reduce per network bitwise; the bf16-compressed mapping gradient stays within
    2^-7 of the fp32 exchange; the sharded update of the mapping layer (reduce-scatter, AdamW on each rank's share, all-gather of the
    fp32 master) leaves bit-identical replicas and the replicated update's weights, and every rank's master of the
    shares it does not own is already current after the step, with no gather_master() call."""
    same, finite, differ, staged_equal, compressed_close, rel, sharded_ok = eu.run_ranks(_dp_worker, 2, 500, gpu=True)[0]
    assert same, "replicas diverged: weights / reduced gradients differ between ranks"
    assert finite and differ
    assert staged_equal, "staged (overlapped) D / G exchange must equal the single all-reduce bit for bit"
    assert compressed_close, f"bf16 exchange of the mapping gradient: relative deviation {rel}"
    assert sharded_ok, "sharded update of the mapping layer: replicas / the replicated update differ"


def _dp_coherence_worker(rank, world):
    import torch.distributed as dist
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    B = 4
    gen = torch.Generator().manual_seed(60 + rank)  # different data per rank
    reals = [(torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(3)]
    z = torch.randn(B, 1024, generator=torch.Generator().manual_seed(7)).cuda()

    def run(shard):
        torch.manual_seed(0)  # identical init on every rank
        D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, dropout_rate=0.0, batch_size=B,
                                    transformer_blocks_count=2)).cuda().train()
        G = SirenGenerator(embed=128, layers=3, siren_hidden=256, dropout=0.0).cuda().train()
        eng = GanEngine(D, G, batch=B, seed=100 + rank, shard_mapping_update=shard)
        assert eng.world == world and eng.shard_map == shard
        eng.step(reals[0])
        with torch.no_grad():
            G(z)                    # a module forward (sampling, FID): refresh_shadow() recasts the whole shadow from the master
        eng.step(reals[1])
        eng.sync_from_modules()     # the same recast, as after an in-place edit or a load_state_dict
        eng.step(reals[2])
        torch.cuda.synchronize()    # no gather_master() anywhere
        fd, fg = D.vit._flat, G._flat
        got = tuple(t.detach().cpu().clone() for t in (fd.flat, fd.shadow, fg.flat, fg.shadow))
        eng.close()
        return got

    rep, sh = run(False), run(True)
    gather = [None] * world
    dist.all_gather_object(gather, (rep, sh))
    if rank == 0:
        bits = lambda t: t.view(torch.int16)  # noqa: E731
        res = {
            "ranks_equal": all(torch.equal(gather[0][k][i], g[k][i]) for g in gather[1:] for k in (0, 1) for i in range(4)),
            "shard_equals_replicated": all(torch.equal(g[0][i], g[1][i]) for g in gather for i in range(4)),
            "shadow_is_rne": all(torch.equal(bits(g[k][i + 1]), bits(g[k][i].to(torch.bfloat16))) for g in gather for k in (0, 1)
                                 for i in (0, 2)),
            "finite": all(bool(torch.isfinite(g[k][i]).all()) for g in gather for k in (0, 1) for i in (0, 2)),
        }
        return res


@pytest.mark.timeout(600)
def test_two_rank_sharded_mapping_update_keeps_masters_coherent():
    """shard_mapping_update on two gloo ranks (one GPU): step, a module forward of G (which recasts the whole bf16 shadow from the fp32
    master), step, sync_from_modules(), step.  The replicas' D and G masters and shadows must be bit-identical across the ranks with no
    gather_master() call, bit-equal to the replicated update's, and every shadow the round-to-nearest-even of its master: a rank whose
    master of the mapping shares it does not own were stale would recast stale weights over the gathered ones and diverge."""
    val = eu.run_ranks(_dp_coherence_worker, 2, 500, gpu=True)[0]
    assert val["finite"], val
    assert val["shadow_is_rne"], val
    assert val["ranks_equal"], val
    assert val["shard_equals_replicated"], val


def test_engine_step_with_patch_grid_generator_at_c4_shape():
    """SURVEY 8f row f1 + config C4's geometry (64x64, patch 8, 8 heads): patch-grid generator feeding the ViT
    discriminator through GanEngine, against the fp32 step oracle (small widths so the CPU oracle stays in seconds)."""
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo

    B = 4
    torch.manual_seed(5)
    cfg = Config(embeddings_dimension=256, attention_heads_count=8, transformer_blocks_count=2, image_size=64, patch_size=8,
                 classes_count=1, dropout_rate=0.0, batch_size=B)
    D = ViTDiscriminator(cfg)
    G = SirenGenerator(latent=256, image_size=64, channels=3, embed=256, heads=4, layers=2, siren_hidden=256, dropout=0.0, patch_size=8)
    ddims = vo.VitDims(image=64, patch=8, embed=256, heads=8, layers=2, classes=1)
    gdims = go.GenDims(latent=256, tokens=64, embed=256, heads=4, layers=2, siren_hidden=256, image=64, patch=8)
    oracle = so.GanStepOracle({k: v.detach().clone() for k, v in D.state_dict().items()},
                              {k: v.detach().clone() for k, v in G.state_dict().items()}, ddims, gdims)
    eng = GanEngine(D.cuda(), G.cuda(), batch=B)
    real = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(0)) * 2 - 1
    losses = eng.step(real.cuda())
    torch.cuda.synchronize()
    ref = oracle.step(real, eng.z.detach().cpu().clone())
    got = losses.cpu().tolist()
    assert abs(got[0] - ref["d_real"]) < 2e-2 and abs(got[1] - ref["d_fake"]) < 2e-2 and abs(got[2] - ref["g"]) < 2e-2, (got, ref)


def test_wasserstein_losses_and_gradient_clipping():
    """The critic losses and clip_grad_norm_ limits of the reference's unreached Wasserstein step (training.py:72,78,
    97,104) through GanEngine vs the step oracle; the clip limits are set low enough to be active."""
    from vit_gan_amd.engine import GanEngine
    import vit_gan_amd  # noqa: F401
    from oracle import step_oracle as so

    B = 8
    D, G, oracle = eu.build(B, "wasserstein")
    oracle.clip_d, oracle.clip_g = 0.05, 0.02
    oracle.diversity_weight = 0.1
    eng = GanEngine(D, G, batch=B, loss="wasserstein", clip_d=0.05, clip_g=0.02, diversity_weight=0.1)
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    w_before = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    losses = eng.step(real.cuda())
    torch.cuda.synchronize()
    ref = oracle.step(real, eng.z.detach().cpu().clone())
    got = losses.cpu().tolist()
    assert abs(got[0] - ref["d_real"]) < 2e-2 and abs(got[1] - ref["d_fake"]) < 2e-2 and abs(got[2] - ref["g"]) < 2e-2, (got, ref)
    # the recorded norms are the pre-clip global norms and exceed the limits (clipping was active)
    from oracle.step_oracle import diversity_loss
    with torch.no_grad():
        want_div = float(diversity_loss(oracle.G(eng.z.detach().cpu())))  # oracle G was already stepped: compare loosely
    assert abs(float(eng.div_loss) - want_div) < 0.15 * abs(want_div) + 1e-3
    nd, ng = float(eng.clip_scratch[0, 0]), float(eng.clip_scratch[1, 0])
    assert nd > 0.05 and ng > 0.02, (nd, ng)
    k = "vit.encoder.1.fc2.weight"
    upd = (D.state_dict()[k].detach().cpu() - w_before[k])
    ref_upd = oracle.d[k].detach() - w_before[k]
    assert float((upd - ref_upd).abs().max()) < 1.1e-3  # first AdamW step: +-lr per weight, sign flips on noise-level entries only
    assert float(((upd - ref_upd).abs() < 1e-4).float().mean()) > 0.9


def test_instance_noise_on_the_discriminator_inputs():
    """training.py:83-90: D's own step sees real / fake + sigma * randn, the generator's pass through D the clean fake.
    The engine's noisy copies are handed to the step oracle."""
    from vit_gan_amd.engine import GanEngine
    B = 8
    D, G, oracle = eu.build(B, "ns")
    eng = GanEngine(D, G, batch=B, instance_noise=0.1)
    real = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1
    losses = eng.step(real.cuda())
    torch.cuda.synchronize()
    noisy = eng.imgs_noisy.float().cpu()
    clean = eng.imgs.float().cpu()
    sd = float((noisy - clean).std())
    assert 0.08 < sd < 0.12, sd
    ref = oracle.step(real, eng.z.detach().cpu().clone(), noisy_inputs=(noisy[:B], noisy[B:]))
    got = losses.cpu().tolist()
    assert abs(got[0] - ref["d_real"]) < 2e-2 and abs(got[1] - ref["d_fake"]) < 2e-2 and abs(got[2] - ref["g"]) < 2e-2, (got, ref)


def test_two_stream_schedule_is_the_unfused_step():
    """``two_stream=True`` runs D(real) beside [G, D(fake)] and the generator's pass through D as two half-batches side by
    side.  It is the reference's own pass structure (two separate D passes): against the single-stream unfused engine the
    first step's losses are bit-equal (same kernels on the same rows), later ones agree to fp32 reassociation of the two
    gradient buffers; eager and hipGraph replay of the two-stream step are bit-equal; and it matches the step model."""
    import gpu_util as u
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo
    B, n = 8, 3
    runs = {}
    for name, kw in (("unfused", dict(fuse_real_fake=False, use_graph=False, concurrent_wgrad=False)),
                     ("two_stream", dict(two_stream=True, use_graph=False)),
                     ("two_stream_graph", dict(two_stream=True, use_graph=True))):
        eng, D, G, _ = eu.bench_like(B, d_dropout=0.0, g_dropout=0.0, **kw)
        runs[name] = eu.run_steps(eng, eu.batches(B, n))
    (l_u, s_u, _), (l_t, s_t, _) = runs["unfused"], runs["two_stream"]
    eu.assert_same_run(runs["two_stream"], runs["two_stream_graph"], "graph replay != eager (two-stream)")
    assert torch.equal(l_t[0, :2], l_u[0, :2]), (l_t[0], l_u[0])       # D losses of step 0: identical arithmetic
    # Later losses: the two schedules add the real and the fake pass's weight gradients in a different order (1.5e-8 on gradients
    # of 0.5, checked below); AdamW's first steps are sign-like (m / sqrt(v) = +-1), so an ulp on a noise-level gradient is a
    # 2 lr difference in that parameter, and three GAN steps amplify it: measured 5.5e-3 on losses of 0.07-3.0 (round 2's
    # kernels: 4e-4; the one-byte gelu' grid is coarser than bf16 for small derivatives, so a flipped code moves more).
    assert float((l_t - l_u).abs().max()) < 1e-2, (l_t, l_u)
    close = float(((s_t[0] - s_u[0]).abs() < 2e-5).float().mean())
    assert close > 0.98 and float((s_t[0] - s_u[0]).abs().max()) < 3.1e-3, close   # sign flips of noise-level gradients only
    # the first step's D gradients themselves: the same up to fp32 reassociation of the two passes' sums
    gr = {}
    for name, kw in (("unfused", dict(fuse_real_fake=False, use_graph=False, concurrent_wgrad=False)), ("two_stream", dict(two_stream=True, use_graph=False))):
        eng, D, G, _ = eu.bench_like(B, d_dropout=0.0, g_dropout=0.0, **kw)
        eu.run_steps(eng, eu.batches(B, 1))
        gr[name] = eng.vit._flat.grad.clone().cpu()
    assert float((gr["unfused"] - gr["two_stream"]).abs().max()) < 1e-6 * float(gr["unfused"].abs().max())
    # with dropout on: the model with the two-stream passes' own masks (pass seeds 0 / 1, half-batch passes 2 / 3)
    eng, D, G, (d_state, g_state) = eu.bench_like(B, two_stream=True, use_graph=True)
    model = so.GanStepOracle(d_state, g_state, vo.VitDims(layers=2, classes=1), go.GenDims(layers=2), faithful=True)
    g = torch.Generator().manual_seed(9)
    real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    z = torch.randn(B, 1024, generator=g)
    got = eng.step(real.cuda(), z.cuda()).cpu().tolist()
    torch.cuda.synchronize()
    m = _step_masks(u, eng, B, 1)
    ref = model.step(real, z, masks=m)
    for x, k in zip(got, ("d_real", "d_fake", "g")):
        assert abs(x - ref[k]) < 1e-3, (k, got, ref)


def _rccl_worker(rank, world):
    import torch.distributed as dist
    flat = torch.arange(4096, dtype=torch.float32, device="cuda")
    comm = torch.cuda.Stream()
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream())
    with torch.cuda.stream(comm):            # the exact call pattern of GradSync.reduce_range (overlap path)
        comm.wait_event(ready)
        work = dist.all_reduce(flat[1024:3072], op=dist.ReduceOp.SUM, async_op=True)
        half = flat[:1024].to(torch.bfloat16)
        dist.all_reduce(half, op=dist.ReduceOp.SUM)
    work.wait()
    torch.cuda.current_stream().wait_stream(comm)
    torch.cuda.synchronize()
    ok = torch.equal(flat.cpu(), torch.arange(4096, dtype=torch.float32)) and torch.equal(half.float().cpu(), torch.arange(1024).float().to(torch.bfloat16).float())
    # the whole step with its (one-rank) RCCL all-reduces captured in a hipGraph: replay == eager, bit for bit, 3 steps
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    B = 16
    res = []
    # (eager, graph) with the bf16 mapping exchange, then (eager, graph) with the sharded update of the mapping layer: on one rank
    # the reduce-scatter / all-gather are identities, but they are RCCL's calls, on the side stream, inside the capture
    for use_graph, shard in ((False, False), (True, False), (False, True), (True, True)):
        torch.manual_seed(0)
        D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, batch_size=B, transformer_blocks_count=3)).cuda().train()
        G = SirenGenerator(embed=128, layers=2, siren_hidden=256).cuda().train()
        eng = GanEngine(D, G, batch=B, seed=4, use_graph=use_graph, external_noise=True, exchange_single_rank=True,
                        compress_mapping_grad=not shard, shard_mapping_update=shard)
        assert eng.sync.active and eng.sync.overlap and eng.shard_map == shard
        ls = [eng.step(real, z).clone() for real, z in eu.batches(B, 3, seed=9)]
        torch.cuda.synchronize()
        res.append((torch.stack(ls).cpu(), D.vit._flat.flat.detach().cpu().clone(), G._flat.flat.detach().cpu().clone(),
                    eng.graph_active, eng.graph_fallback_reason))
        eng.close()
    graph_ok = res[1][3] and res[1][4] is None and res[3][3] and res[3][4] is None
    same = all(torch.equal(a, b) for a, b in zip(res[0][:3], res[1][:3])) and all(torch.equal(a, b) for a, b in zip(res[2][:3], res[3][:3]))
    return ok and graph_ok and same, dist.get_backend(), res[1][4]


@pytest.mark.timeout(300)
def test_rccl_backend_executes_the_exchange_calls_on_one_rank():
    """The driver's multi-GPU run uses backend "nccl" (= RCCL).  A one-GPU box cannot host two RCCL ranks, but a
    one-rank RCCL group executes the same calls - communicator creation, an asynchronous fp32 range all-reduce and a bf16
    all-reduce on the side stream, stream joins - so that path is not first exercised on the 8-GPU node.  It also runs the
    engine's step with those collectives (staged D and G exchange, bf16 mapping gradient) CAPTURED in a hipGraph: three
    replayed steps must equal three eager steps bit for bit (what bench.py does on more than one GPU since round 3)."""
    (val,) = eu.run_ranks(_rccl_worker, 1, 240, backend="nccl", gpu=True)
    assert val[0] and val[1] == "nccl", val  # val[2]: the engine's graph fallback reason, if the capture was refused
