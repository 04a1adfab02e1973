"""The generator's weight EMA on the GPU: vg_adamw_ema_step / vg_ema_update against vg_adamw_step (bit-equal weights, moments and
shadow) and the float64 average of tests/ema_ref.py; the engine's average along a trajectory, under hipGraph replay, on the two-stream
and the sharded schedule; sampling from the average; carrying an engine across a restart; the trainer's artefacts."""
import os

import pytest
import torch

import engine_util as eu
from ema_ref import check_ema_step, check_ema_trajectory, copies
import gpu_util as u

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HYP = (5e-4, 0.9, 0.999, 1e-8, 1e-3)  # lr, b1, b2, eps, wd
STEPS = [1, 2, 3, 10, 100, 10 ** 4, 10 ** 6]
DECAYS = (0.0, 0.5, 0.999, 0.9999)


def _state(n, seed):
    """gpu_util.adamw_state and the average before the step: equal to p, 1e-6 and 1e-3 of p away, of p's order, and (every 8th element of
    the upper half) unrelated to p."""
    p, m, v, g, gen = u.adamw_state(n, seed)
    rel = torch.tensor([0.0, 1e-6, 1e-3, 1.0])[torch.randperm(n, generator=gen) % 4]
    e = p - p * rel * torch.randn(n, generator=gen)
    e[n // 2::8] = 10.0 ** (torch.rand(len(e[n // 2::8]), generator=gen) * 5 - 4)
    return p, m, v, g, e


def _kernel_case(t, start, decay, device_counter, n, lo, total, seed):
    p0, m0, v0, g, e0 = _state(total, seed)
    s = slice(lo, lo + n)
    if copies(t, start):  # a copying step must not even look at the old average
        e0[s] = float("nan")
    step_dev = torch.tensor([t], dtype=torch.int32, device="cuda") if device_counter else None
    host_t = 0 if device_counter else t
    what = f"t={t} ema_start={start} decay={decay} {'device' if device_counter else 'host'} counter [{lo}, {lo + n}) of {total}"
    # the reference bits: plain AdamW on the same inputs
    Pr, Mr, Vr, Gr = (u.dev(x.clone()) for x in (p0, m0, v0, g))
    SHr = torch.full((total,), -7.0, dtype=BF, device="cuda")
    u.call("vg_adamw_step", u.off(Pr, lo), u.off(Gr, lo), u.off(Mr, lo), u.off(Vr, lo), u.off(SHr, lo), n, *HYP, host_t, u.ptr(step_dev), 0.5,
           u.stream())
    # the fused kernel
    P, M, V, G_, E = (u.dev(x.clone()) for x in (p0, m0, v0, g, e0))
    SH = torch.full((total,), -7.0, dtype=BF, device="cuda")
    u.call("vg_adamw_ema_step", u.off(P, lo), u.off(G_, lo), u.off(M, lo), u.off(V, lo), u.off(SH, lo), u.off(E, lo), n, *HYP, host_t,
           u.ptr(step_dev), 0.5, decay, start, u.stream())
    # the average alone, from the fused kernel's weights
    E2 = u.dev(e0.clone())
    u.call("vg_ema_update", u.off(E2, lo), u.off(P, lo), n, decay, start, host_t, u.ptr(step_dev), u.stream())
    u.sync()
    if device_counter:
        assert int(step_dev[0]) == t, f"{what}: the counter was written"
    for name, a, b in (("p", P, Pr), ("m", M, Mr), ("v", V, Vr)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: {name} differs from vg_adamw_step's"
    assert torch.equal(SH.view(torch.int16), SHr.view(torch.int16)), f"{what}: shadow differs from vg_adamw_step's"
    assert torch.equal(G_.cpu(), g), f"{what}: the gradient was written"
    frac = check_ema_step(e0[s], P.cpu()[s], t, decay, start, E.cpu()[s], what)
    assert torch.equal(E2.cpu()[s].view(torch.int32), E.cpu()[s].view(torch.int32)), f"{what}: vg_ema_update differs from the fused kernel"
    out = torch.ones(total, dtype=torch.bool)
    out[s] = False
    for name, buf, ref in (("p", P, p0), ("m", M, m0), ("v", V, v0), ("ema", E, e0), ("ema (vg_ema_update)", E2, e0)):
        assert torch.equal(buf.cpu()[out], ref[out]), f"{what}: {name} written outside its range"
    assert bool((SH.cpu()[out] == -7.0).all()), f"{what}: shadow written outside its range"
    return frac


@pytest.mark.parametrize("device_counter", [True, False])
@pytest.mark.parametrize("t", STEPS)
def test_fused_kernel_matches_adamw_bits_and_the_fp64_average(t, device_counter):
    worst = 0.0
    for start in sorted({0, t - 1, t, t + 1}):
        for decay in DECAYS:
            worst = max(worst, _kernel_case(t, start, decay, device_counter, n=8196, lo=0, total=8196, seed=7 * t + start))
    # an interior range of larger buffers: lo a multiple of 4 but not of 1024, n not a multiple of 1024 (what the sharded step issues)
    for start in sorted({0, t - 1, t, t + 1}):
        worst = max(worst, _kernel_case(t, start, 0.999, device_counter, n=3 * 1024 + 12, lo=1028, total=1028 + 3 * 1024 + 12 + 2052,
                                        seed=11 * t + start))
    print(f"\nema t={t} {'device' if device_counter else 'host'} counter: worst {worst:.4f} of the bound")


def test_rejected_calls_launch_nothing():
    from vit_gan_amd import _lib
    n = 4096
    bufs = [torch.full((n,), 0.25, device="cuda") for _ in range(5)]
    SH = torch.zeros(n, dtype=BF, device="cuda")
    P, G_, M, V, E = bufs
    step_dev = torch.ones(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    for nn_, decay, start, want in ((n - 2, 0.999, 0, -3), (n, 1.0, 0, -2), (n, -0.5, 0, -2), (n, 0.999, -1, -2)):
        assert L.vg_adamw_ema_step(u.ptr(P), u.ptr(G_), u.ptr(M), u.ptr(V), u.ptr(SH), u.ptr(E), nn_, *HYP, 0, u.ptr(step_dev), 1.0, decay, start,
                                   u.stream()) == want
        assert L.vg_ema_update(u.ptr(E), u.ptr(P), nn_, decay, start, 0, u.ptr(step_dev), u.stream()) == want
    assert L.vg_adamw_ema_step(u.ptr(P), u.ptr(G_), u.ptr(M), u.ptr(V), u.ptr(SH), None, n, *HYP, 0, u.ptr(step_dev), 1.0, 0.999, 0, u.stream()) == -1
    u.sync()
    assert all(bool((x == 0.25).all()) for x in bufs) and bool((SH == 0).all()), "a rejected call launched a kernel"


# ---- engine ---------------------------------------------------------------------------------------------------------------------------
def _engine(seed=5, **kw):
    """The small train-mode configuration with dropout, fused real+fake pass, B = 4; the noise comes from the caller unless told otherwise."""
    opts = dict(external_noise=True)
    opts.update(kw)
    return eu.train_engine(4, seed, **opts)[:3]


def _run(eng, n, skip=0, masters=None):
    losses = []
    for real, z in eu.batches(eng.B, n, skip=skip):
        losses.append(eng.step(real, z if eng.external_noise else None).clone())
        if masters is not None:
            masters.append(eng.gen._flat.flat.detach().clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu()


def _snapshot(eng):
    """Every piece of training state but the average, then the average (None without one)."""
    fd, fg = eng.vit._flat, eng.gen._flat
    base = [t.detach().clone().cpu() for t in (fd.flat, fd.shadow, fg.flat, fg.shadow, eng.m_d, eng.v_d, eng.m_g, eng.v_g, eng.step_t)]
    return base, None if eng.ema_g is None else eng.ema_g.detach().clone().cpu()


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: state tensor {i} differs"


def test_engine_average_follows_the_trajectory_and_leaves_training_alone():
    """12 eager steps: ema_g against the float64 recursion over the masters the engine itself wrote (ema_start 0 and 5), and every
    other piece of state and every loss bit-equal to the same engine without the average."""
    plain, _, _ = _engine()
    assert plain.ema_g is None and len(plain._state_tensors()) == 9
    l0 = _run(plain, 12)
    s0, _ = _snapshot(plain)
    for start in (0, 5):
        eng, D, G = _engine(ema_decay=0.999, ema_start=start)
        assert eng.ema_g.dtype == torch.float32 and eng.ema_g.shape == G._flat.flat.shape and torch.equal(eng.ema_g, G._flat.flat)
        assert any(t is eng.ema_g for t in eng._state_tensors())
        masters = []
        l1 = _run(eng, 12, masters=masters)
        s1, ema = _snapshot(eng)
        assert torch.equal(l1, l0), (start, l1, l0)
        _same(s1, s0, f"ema_start={start} against ema_decay=0")
        masters = [m.cpu() for m in masters]
        assert not torch.equal(masters[0], masters[-1])
        frac = check_ema_trajectory(masters, 0.999, start, ema, f"ema_start={start}")
        assert not torch.equal(ema, masters[-1]), "after 12 steps the average cannot equal the last iterate"
        print(f"\nengine trajectory, ema_start={start}: worst {frac:.4f} of the summed bound")


@pytest.mark.parametrize("two_stream", [False, True])
def test_graph_replay_equals_eager_with_the_average(two_stream):
    runs = {}
    for use_graph in (False, True):
        eng, _, _ = _engine(ema_decay=0.999, ema_start=2, use_graph=use_graph, two_stream=two_stream)
        losses = _run(eng, 5)
        assert eng.graph_active == use_graph and eng.steps == 5 and int(eng.step_t) == 5
        runs[use_graph] = (losses, *_snapshot(eng))
    assert torch.equal(runs[True][0], runs[False][0])
    _same(runs[True][1], runs[False][1], "graph against eager")
    assert torch.equal(runs[True][2], runs[False][2]), "ema_g differs between replay and eager"
    assert not torch.equal(runs[False][2], runs[False][1][2]), "the average should have left the master behind after the warm-up"


def test_reset_optimizer_restarts_the_average():
    eng, _, G = _engine(ema_decay=0.999)
    _run(eng, 3)
    assert not torch.equal(eng.ema_g, G._flat.flat)
    before = eng.ema_g.clone()
    eng.sync_from_modules()  # a plain refresh leaves the average alone
    assert torch.equal(eng.ema_g, before)
    eng.sync_from_modules(reset_optimizer=True)
    _run(eng, 1, skip=3)
    assert torch.equal(eng.ema_g, G._flat.flat), "the step after a reset copies the weights"
    _run(eng, 1, skip=4)
    assert not torch.equal(eng.ema_g, G._flat.flat)


def test_sampling_from_the_live_and_the_averaged_generator():
    """sample(ema=False) is G.eval()(z); sample(ema=True) is a fresh generator loaded from ema_state_dict(), before and after a
    further replay of the captured step - and the replays do not notice the sampling in between."""
    from vit_gan_amd.generator import SirenGenerator
    ref, _, _ = _engine(ema_decay=0.999, use_graph=True)
    ref_l = _run(ref, 5)
    ref_s, ref_e = _snapshot(ref)

    eng, _, G = _engine(ema_decay=0.999, use_graph=True)
    with pytest.raises(ValueError):
        eng.sample(torch.zeros(3, 7, device="cuda"))
    l_a = _run(eng, 3)
    assert eng.graph_active
    z = torch.randn(6, 1024, generator=torch.Generator().manual_seed(1)).cuda()  # not the engine's batch of 4

    def fresh():
        m = SirenGenerator(layers=2, dropout=0.2)
        m.load_state_dict({k: v.cpu() for k, v in eng.ema_state_dict().items()}, strict=True)
        return m.cuda().eval()

    def check(tag):
        with torch.no_grad():
            live = eng.sample(z, ema=False)
            G.eval()
            want_live = G(z)
            G.train()
            avg = eng.sample(z)
            want_avg = fresh()(z)
        assert live.dtype == G.out_dtype and live.shape == (6, 3, 32, 32) and avg.shape == (6, 3, 32, 32)
        assert torch.equal(live, want_live), f"{tag}: sample(ema=False) != G.eval()(z)"
        assert torch.equal(avg, want_avg), f"{tag}: sample(ema=True) != a generator loaded from ema_state_dict()"
        assert not torch.equal(avg, live)
        assert torch.equal(eng.sample(z), avg), f"{tag}: a second sample (cached cast) differs"
        return avg

    a3 = check("after 3 steps")
    l_b = _run(eng, 1, skip=3)
    a4 = check("after a further replay")
    assert not torch.equal(a3, a4), "the cast of the average was not redone after a step"
    l_c = _run(eng, 1, skip=4)
    assert torch.equal(torch.cat([l_a, l_b, l_c]), ref_l), "sampling disturbed the replayed steps"
    s, e = _snapshot(eng)
    _same(s, ref_s, "with sampling in between")
    assert torch.equal(e, ref_e)
    # the exported average has the generator's keys and shapes, and loads back in place
    sd = eng.ema_state_dict()
    gsd = G.state_dict()
    assert set(sd) == set(gsd) and all(sd[k].shape == gsd[k].shape and sd[k].dtype == torch.float32 for k in sd)
    ptr = eng.ema_g.data_ptr()
    eng.load_ema_state_dict({k: v * 0.5 for k, v in sd.items()})
    assert eng.ema_g.data_ptr() == ptr and all(torch.equal(v, sd[k] * 0.5) for k, v in eng.ema_state_dict().items())
    assert not torch.equal(eng.sample(z), a4), "sample() served a stale cast after load_ema_state_dict"
    with pytest.raises(ValueError):
        eng.load_ema_state_dict({k: v for k, v in list(sd.items())[1:]})
    with pytest.raises(ValueError):
        eng.load_ema_state_dict({k: v.reshape(-1)[:4] for k, v in sd.items()})


def test_an_engine_without_the_average_says_so():
    eng, _, _ = _engine()
    z = torch.randn(2, 1024, device="cuda")
    with pytest.raises(RuntimeError, match="ema_decay"):
        eng.sample(z, ema=True)
    with pytest.raises(RuntimeError, match="ema_decay"):
        eng.sample(z)
    with pytest.raises(RuntimeError, match="ema_decay"):
        eng.ema_state_dict()
    assert eng.sample(z, ema=False).shape == (2, 3, 32, 32)
    assert "ema_g" not in eng.state_dict()


class _Gan(torch.nn.Module):
    def __init__(self, D, G):
        super().__init__()
        self.discriminator, self.generator = D, G


@pytest.mark.parametrize("use_graph,external_noise", [(False, True), (True, False), (True, True)])
def test_resume_continues_bit_for_bit(use_graph, external_noise, tmp_path):
    """3 steps, save gan.state_dict() and eng.state_dict(), rebuild everything, load both, 3 more steps == 6 uninterrupted steps:
    weights, shadows, moments, counter, the average and the losses.  With external_noise=False the latent batches are drawn on the
    device from (noise seed, step counter) - both are engine state."""
    kw = dict(ema_decay=0.999, ema_start=2, use_graph=use_graph, external_noise=external_noise)
    ref, _, _ = _engine(**kw)
    ref_l = _run(ref, 6)
    ref_s, ref_e = _snapshot(ref)

    first, D, G = _engine(**kw)
    l_a = _run(first, 3)
    torch.save(_Gan(D, G).state_dict(), tmp_path / "gan.pth")
    torch.save(first.state_dict(), tmp_path / "engine.pth")
    first.close()

    second, D2, G2 = _engine(seed=99, **kw)  # other initial weights: everything must come from the two files
    assert not torch.equal(G2._flat.flat, G._flat.flat)
    _Gan(D2, G2).load_state_dict(torch.load(tmp_path / "gan.pth"), strict=True)
    state = torch.load(tmp_path / "engine.pth")
    assert state["format_version"] == 1 and state["steps"] == 3 and int(state["step_t"]) == 3 and "ema_g" in state
    assert not any(k.startswith(("discriminator", "generator", "vit")) for k in state)
    second.load_state_dict(state)
    assert second.steps == 3 and int(second.step_t) == 3
    l_b = _run(second, 3, skip=3)
    assert torch.equal(torch.cat([l_a, l_b]), ref_l), (l_a, l_b, ref_l)
    s, e = _snapshot(second)
    _same(s, ref_s, "resumed against uninterrupted")
    assert torch.equal(e, ref_e), "ema_g differs after the resume"


def test_loading_engine_state_checks_what_it_is_given():
    eng, _, G = _engine(ema_decay=0.999, use_graph=True)
    _run(eng, 3)
    state = eng.state_dict()
    ptrs = [t.data_ptr() for t in eng._state_tensors()]
    eng.load_state_dict(state)
    assert ptrs == [t.data_ptr() for t in eng._state_tensors()], "load_state_dict must copy in place"
    no_ema = {k: v for k, v in state.items() if k != "ema_g"}
    with pytest.raises(ValueError, match="ema_g"):
        eng.load_state_dict(no_ema)
    with pytest.raises(ValueError, match="ema_g"):
        eng.load_state_dict(no_ema, strict=True)
    with pytest.raises(ValueError):
        eng.load_state_dict({**state, "m_g": state["m_g"][:-4]})
    with pytest.raises(ValueError):
        eng.load_state_dict({**state, "ema_g": state["ema_g"][:-4]})
    with pytest.raises(ValueError):
        eng.load_state_dict({**state, "format_version": 0})
    with pytest.raises(ValueError):
        eng.load_state_dict({k: v for k, v in state.items() if k != "v_d"})
    plain, _, _ = _engine()
    with pytest.raises(ValueError, match="ema_g"):
        plain.load_state_dict(state)
    # strict=False without an average: it restarts as a copy at the next step, then averages again
    eng.load_state_dict(no_ema, strict=False)
    _run(eng, 1, skip=3)
    assert int(eng.step_t) == 4 and torch.equal(eng.ema_g, G._flat.flat)
    _run(eng, 1, skip=4)
    assert not torch.equal(eng.ema_g, G._flat.flat)


def _shard_worker(rank, world):
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    B = 16
    res = []
    for use_graph, shard in ((False, False), (False, True), (True, True)):
        torch.manual_seed(0)
        D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, batch_size=B, transformer_blocks_count=3)).cuda().train()
        G = SirenGenerator(embed=128, layers=2, siren_hidden=256).cuda().train()
        eng = GanEngine(D, G, batch=B, seed=4, use_graph=use_graph, external_noise=True, ema_decay=0.999, ema_start=2,
                        exchange_single_rank=shard, shard_mapping_update=shard)
        assert eng.shard_map == shard and eng.sync.active == shard
        ls = [eng.step(real, z).clone() for real, z in eu.batches(B, 4, seed=9)]
        torch.cuda.synchronize()
        res.append((torch.stack(ls).cpu(), G._flat.flat.detach().cpu().clone(), eng.ema_g.detach().cpu().clone(), eng.graph_active,
                    eng.graph_fallback_reason))
        eng.close()
    plain, shard_eager, shard_graph = res
    report = {"graph": shard_graph[3] and shard_graph[4] is None,
              "averaged": not torch.equal(plain[2], plain[1]),
              "eager_master": torch.equal(shard_eager[1], plain[1]), "eager_ema": torch.equal(shard_eager[2], plain[2]),
              "graph_master": torch.equal(shard_graph[1], plain[1]), "graph_ema": torch.equal(shard_graph[2], plain[2]),
              "losses": torch.equal(shard_eager[0], plain[0]) and torch.equal(shard_graph[0], plain[0])}
    return report


@pytest.mark.timeout(300)
def test_sharded_mapping_update_holds_the_replicated_average():
    """shard_mapping_update on a one-rank RCCL group (the collectives are identities, the call sequence is the sharded one: the fused
    kernel on the two ranges outside the mapping Linear, plain AdamW on the share, vg_ema_update on the gathered layer), eager and
    captured, against the plain engine: master and average bit for bit."""
    (val,) = eu.run_ranks(_shard_worker, 1, 240, backend="nccl", gpu=True)
    assert all(val.values()), val


def test_trainer_samples_from_and_saves_the_average(tmp_path):
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.training import train_model
    cfg = {"epochs": 1, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}
    seen = []

    def fid(gan, epoch):
        seen.append((gan.generator, gan.discriminator, {k: v.clone() for k, v in gan.generator.state_dict().items()}))
        return 20.5

    out = train_model(cfg, ema_decay=0.999, max_epochs=1, steps_per_epoch=3, output_base=str(tmp_path), fid_fn=fid)
    d, eng, G_ema = out["dirs"], out["engine"], out["generator_ema"]
    assert isinstance(G_ema, SirenGenerator) and not G_ema.training and G_ema is not out["generator"]
    want = eng.ema_state_dict()
    got = G_ema.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert not all(torch.equal(got[k], v) for k, v in out["generator"].state_dict().items()), "the average equals the last iterate"
    # fid_fn saw the averaged generator beside the trained discriminator
    assert len(seen) == 1 and seen[0][0] is G_ema and seen[0][1] is out["discriminator"]
    assert all(torch.equal(seen[0][2][k], want[k]) for k in want)
    for path in (os.path.join(d.save, "generator_ema.pth"), os.path.join(d.checkpoints, "generator_ema.pth")):
        sd = torch.load(path, map_location="cpu")
        assert set(sd) == set(want) and all(torch.equal(sd[k], want[k].cpu()) for k in want), path
    state = torch.load(os.path.join(d.save, "engine_state.pth"), map_location="cpu")
    assert state["steps"] == 3 and torch.equal(state["ema_g"], eng.ema_g.cpu()) and torch.equal(state["m_g"], eng.m_g.cpu())
    # the gan checkpoint keeps the reference's keys
    assert set(torch.load(os.path.join(d.save, "final_model.ckpt"), map_location="cpu")) == set(out["gan"].state_dict())
    assert os.path.getsize(os.path.join(d.images, "samples_epoch_0.png")) > 100
