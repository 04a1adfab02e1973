"""The step's telemetry on the GPU: vg_grad_stats and vg_logit_stats against the float64 restatement (tests/telemetry_ref.py, whose
bound tests/test_telemetry_cpu.py shows admissible), the engine's record against what the step left behind, hipGraph replay against
eager, the ring's wrap-around, and the trainer's files and lines.  Every test fails on the parent commit (no exports, no option)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gpu_util as u
import telemetry_ref as tr
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib, ops
from vit_gan_amd.config import Config

pytestmark = pytest.mark.gpu


def _counts(slots):
    return np.asarray([tr.numel(shape) for _, shape in slots.values()], dtype=np.float64)


def _stats(g_dev, slots, gscale):
    out = ops.grad_stats(g_dev, slots, gscale)
    u.sync()
    return {"norms": out["norms"].cpu().numpy(), "sum_norms": float(out["sum_norms"]), "l2": float(out["l2"]), "nonfinite": float(out["nonfinite"]),
            "keys": out["keys"]}


def _check_against_ref(got, ref, n, gscale, what):
    bound = tr.norm_bound(ref["norms"], n, gscale)
    err = np.abs(got["norms"].astype(np.float64) - ref["norms"])
    print(f"{what}: max |norm - ref| / bound = {(err / bound).max():.3f}; l2 {got['l2']!r} ref {ref['l2']!r}; sum {got['sum_norms']!r} ref {ref['sum_norms']!r}")
    assert np.isfinite(got["norms"]).all(), f"{what}: a padding NaN was read"
    assert (err <= bound).all(), (what, (err / bound).max())
    assert abs(got["l2"] - ref["l2"]) <= tr.norm_bound(ref["l2"], n.sum(), gscale), what
    assert abs(got["sum_norms"] - ref["sum_norms"]) <= bound.sum() + tr.U * ref["sum_norms"], what
    assert got["nonfinite"] == ref["nonfinite"], what


@pytest.fixture(scope="module")
def case():
    g, slots = tr.grad_case()
    return g, slots, _counts(slots), torch.from_numpy(g).cuda()


@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_grad_stats_on_the_synthetic_segments(case, gscale):
    """Segment lengths 1 .. 1 000 003 at first-element offsets 0 .. 3 mod 4, NaN in every padding element."""
    g, slots, n, g_dev = case
    ref = tr.grad_stats_ref(g, slots, gscale)
    a, b = _stats(g_dev, slots, gscale), _stats(g_dev, slots, gscale)
    _check_against_ref(a, ref, n, gscale, f"synthetic, gscale {gscale}")
    assert a["norms"].tobytes() == b["norms"].tobytes() and (a["sum_norms"], a["l2"]) == (b["sum_norms"], b["l2"]), "two runs differ"
    emul = tr.grad_stats_emul(g, slots, gscale)  # the restated tree is the kernel's: not an approximation of it
    assert a["norms"].tobytes() == emul["norms"].tobytes() and np.float32(a["l2"]) == emul["l2"] and np.float32(a["sum_norms"]) == emul["sum_norms"]


def test_grad_stats_counts_planted_nan_and_inf_in_one_segment_only(case):
    g, slots, n, g_dev = case
    clean = _stats(g_dev, slots, 1.0)
    names = list(slots)
    hit = names.index("seg8.n1000003")
    off = slots[names[hit]][0]
    bad = g.copy()
    bad[off + 5] = np.nan
    bad[off + 4099] = np.inf
    bad[off + 999999] = -np.inf
    bad[off + 1000002] = np.nan
    bad[off] = np.nan
    got = _stats(torch.from_numpy(bad).cuda(), slots, 1.0)
    assert got["nonfinite"] == 5.0
    assert not np.isfinite(got["norms"][hit]) and not np.isfinite(got["l2"]) and not np.isfinite(got["sum_norms"])
    keep = np.arange(len(names)) != hit
    assert got["norms"][keep].tobytes() == clean["norms"][keep].tobytes(), "another segment changed"


def _nets(K=0, seed=0):
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(seed)
    D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=max(K, 1), batch_size=4, transformer_blocks_count=1)).cuda().train()
    G = SirenGenerator(layers=1, n_classes=K).cuda().train()
    return D, G


@pytest.mark.parametrize("K", [0, 3])
def test_grad_stats_on_real_slot_tables(K):
    D, G = _nets(K)
    gen = torch.Generator().manual_seed(11)
    for fp, what in ((D.vit._flat, "ViT E=128 L=1"), (G._flat, f"SIREN generator, layers=1, n_classes={K}")):
        g = np.full(fp.total, np.nan, dtype=np.float32)
        for off, shape in fp.slots.values():
            m = tr.numel(shape)
            g[off:off + m] = (torch.randn(m, generator=gen) * 1e-3).numpy()
        ref = tr.grad_stats_ref(g, fp.slots, 0.125)
        got = _stats(torch.from_numpy(g).cuda(), fp.slots, 0.125)
        assert got["keys"] == list(fp.slots)
        _check_against_ref(got, ref, _counts(fp.slots), 0.125, what)


def test_l2_agrees_with_the_clipping_kernels_norm():
    """vg_grad_clip leaves gscale |g|_2 in scratch[0] (it reads the whole buffer: the padding is zero here, as in the engine).  Its tree:
    the product and three adds inside a float4, ``it`` serial adds per thread, butterfly 6, cross-wave 2, then over the partials 4 serial,
    6, 2 - 23 + it roundings, halved by sqrtf, plus sqrtf's and the product's own: (23 + it) / 2 + 2 units.  Combined with vg_grad_stats'
    KAPPA that is the bound between the two."""
    D, _ = _nets()
    fp = D.vit._flat
    gen = torch.Generator().manual_seed(12)
    g = torch.zeros(fp.total)
    for off, shape in fp.slots.values():
        m = tr.numel(shape)
        g[off:off + m] = torch.randn(m, generator=gen) * 1e-2
    g_dev = g.cuda()
    scratch = torch.zeros(1 + 1024, device="cuda")
    gscale = 0.125
    u.call("vg_grad_clip", u.ptr(g_dev), C.c_longlong(fp.total), C.c_float(gscale), C.c_float(1e30), u.ptr(scratch), u.stream())
    got = _stats(g_dev, fp.slots, gscale)
    assert torch.equal(g_dev.cpu(), g), "max_norm 1e30 must not scale"
    clip_norm = float(scratch[0])
    blocks = min((fp.total // 4 + 255) // 256, 1024)
    it = -(-(fp.total // 4) // (256 * blocks))
    kappa = tr.KAPPA + (23 + it) / 2 + 2
    ref = tr.grad_stats_ref(g.numpy(), fp.slots, gscale)["l2"]
    print(f"l2 {got['l2']!r}, vg_grad_clip {clip_norm!r}, fp64 {ref!r}, bound {kappa * tr.U * ref:.3e}")
    assert abs(got["l2"] - clip_norm) <= kappa * tr.U * ref


@pytest.mark.parametrize("n", [1, 7, 256, 3 * 256, 16384])
def test_logit_stats(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    if n > 1:
        x[::5] = 0.0
        x[1::7] = -0.0
    y = -x[::-1].copy()
    for arr in (x, y):
        got = ops.logit_stats(torch.from_numpy(arr).cuda()).cpu().numpy()
        ref_mean, pos, neg = tr.logit_stats_ref(arr)
        assert got[1] == np.float32(pos) / np.float32(n) and got[2] == np.float32(neg) / np.float32(n), "exact zeros count in neither"
        assert abs(float(got[0]) - ref_mean) <= tr.KAPPA_MEAN * tr.U * float(np.mean(np.abs(arr.astype(np.float64)))) + 1e-45
        assert got.tobytes() == np.asarray(tr.logit_stats_emul(arr), dtype=np.float32).tobytes()
    # two row pointers in one launch: slots role and role + 1; the third slot stays what it was
    out = torch.full((3, 4), -7.0, device="cuda")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    u.call("vg_logit_stats", u.ptr(xd), u.ptr(yd), n, 0, u.ptr(out), u.stream())
    u.sync()
    o = out.cpu().numpy()
    assert o[0, :3].tobytes() == np.asarray(tr.logit_stats_emul(x), dtype=np.float32).tobytes() and o[0, 3] == n
    assert o[1, :3].tobytes() == np.asarray(tr.logit_stats_emul(y), dtype=np.float32).tobytes() and (o[2] == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------- engine
B = 4


def _engine(K=0, seed=0, **kw):
    from vit_gan_amd.engine import GanEngine
    D, G = _nets(K, seed)
    return GanEngine(D, G, batch=B, seed=3, n_classes=K, **kw), D, G


def _batches(n, K=0):
    gen = torch.Generator().manual_seed(21)
    out = []
    for _ in range(n):
        real, z = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, torch.randn(B, 1024, generator=gen)
        lab = (torch.randint(0, K, (B,), generator=gen).cuda().int(), torch.randint(0, K, (B,), generator=gen).cuda().int()) if K else ()
        out.append((real.cuda(), z.cuda()) + lab)
    return out


def _state(eng):
    fd, fg = eng.vit._flat, eng.gen._flat
    return [t.detach().clone() for t in (fd.flat, fd.shadow, fg.flat, fg.shadow, eng.m_d, eng.v_d, eng.m_g, eng.v_g, eng.step_t)]


def _last(rec, name):
    assert len(rec["step"]) >= 1
    return rec[name][-1]


def _f32(t):
    return t.detach().float().cpu().numpy()


def _check_norms(rec, keys, norms, module, what):
    """the newest record's per-tensor norms against a float64 recomputation from the parameters' .grad views"""
    named = dict(module.named_parameters())
    assert list(keys) == [k for k in module.state_dict() if k in named] and len(keys) == len(named)
    ref = np.asarray([float(named[k].grad.detach().double().norm()) for k in keys])
    n = np.asarray([named[k].numel() for k in keys], dtype=np.float64)
    bound = tr.norm_bound(ref, n)
    err = np.abs(norms.astype(np.float64) - ref)
    print(f"{what}: max |norm - ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (what, (err / bound).max())
    return ref, bound


def test_three_eager_steps_record_what_the_step_left_behind_and_change_nothing():
    data = _batches(3)
    plain, _, _ = _engine(external_noise=True)
    for real, z in data:
        plain.step(real, z)
    want = _state(plain)
    eng, D, G = _engine(external_noise=True, telemetry=8)
    for i, (real, z) in enumerate(data):
        eng.step(real, z)
        rec = eng.history()
        assert list(rec["step"]) == [i + 1] and rec["dropped"] == 0
        losses = _f32(eng.losses)
        assert (_last(rec, "loss_d_real"), _last(rec, "loss_d_fake"), _last(rec, "loss_g")) == tuple(losses), "losses bit for bit"
        ref_d, bound_d = _check_norms(rec, rec["keys_d"], rec["grad_norms_d"][-1], D, f"D, step {i + 1}")
        ref_g, bound_g = _check_norms(rec, rec["keys_g"], rec["grad_norms_g"][-1], G, f"G, step {i + 1}")
        for tag, ref, bound, module in (("d", ref_d, bound_d, D), ("g", ref_g, bound_g, G)):
            assert abs(float(_last(rec, f"gnorm_{tag}_sum")) - ref.sum()) <= bound.sum() + tr.U * ref.sum()
            total = float(torch.sqrt(sum(p.grad.detach().double().pow(2).sum() for p in module.parameters())))
            assert abs(float(_last(rec, f"gnorm_{tag}_l2")) - total) <= tr.norm_bound(total, sum(p.numel() for p in module.parameters()))
            assert _last(rec, f"nonfinite_{tag}") == 0.0
        # the plain step reuses logits[:B] for the generator's pass: rows [B, 2B) are D's fake rows, rows [0, B) the generator pass's
        lg = _f32(eng.logits)
        fake, gpass = lg[B:2 * B].reshape(-1), lg[:B].reshape(-1)
        assert _last(rec, "d_fake_acc") == np.float32(np.count_nonzero(fake < 0)) / np.float32(fake.size)
        assert _last(rec, "g_frac_pos") == np.float32(np.count_nonzero(gpass > 0)) / np.float32(gpass.size)
        assert _last(rec, "d_fake_mean") == tr.logit_stats_emul(fake)[0] and _last(rec, "g_mean") == tr.logit_stats_emul(gpass)[0]
        assert 0.0 <= _last(rec, "d_real_acc") <= 1.0
        for off in ("penalty", "bcr_real", "bcr_fake", "ada_p", "ada_rt", "lr_d", "lr_g", "diversity"):
            assert np.isnan(_last(rec, off)), f"{off}: an option that is off is NaN"
    for a, b, name in zip(want, _state(eng), ("D master", "D shadow", "G master", "G shadow", "m_d", "v_d", "m_g", "v_g", "step_t")):
        assert torch.equal(a, b), f"telemetry changed {name}"
    assert eng.first_nonfinite_step is None
    again = eng.history()
    assert len(again["step"]) == 0 and again["dropped"] == 0 and again["grad_norms_d"].shape == (0, len(rec["keys_d"]))
    with pytest.raises(RuntimeError, match="telemetry=0"):
        plain.history()


@pytest.mark.parametrize("mode", ["unfused", "conditional", "ada", "fixed_p"])
def test_accuracies_are_those_of_the_rows_the_step_judged(mode):
    K = 3 if mode == "conditional" else 0
    kw = {"unfused": dict(fuse_real_fake=False), "conditional": dict(), "ada": dict(diffaug="color,translation", ada_target=0.6, ada_interval=2),
          "fixed_p": dict(diffaug="color,translation", aug_p=0.5)}[mode]
    eng, D, G = _engine(K=K, external_noise=True, telemetry=4, **kw)
    for batch in _batches(2, K):
        eng.step(*batch)
        rec = eng.history()
        lg_all = _f32(eng.logits)
        if mode == "conditional":  # the label-selected logits of D's pair
            sel = _f32(eng.selected)
            real, fake = sel[:B], sel[B:]
        else:
            lg = _f32(eng.logits)
            real, fake = lg[:B].reshape(-1), lg[B:2 * B].reshape(-1)
        if mode in ("conditional", "ada"):  # (a plain step reuses the real rows [0, B) for the generator's pass)
            assert _last(rec, "d_real_acc") == np.float32(np.count_nonzero(real > 0)) / np.float32(real.size)
            assert _last(rec, "d_real_mean") == tr.logit_stats_emul(real)[0]
        assert _last(rec, "d_fake_acc") == np.float32(np.count_nonzero(fake < 0)) / np.float32(fake.size)
        assert _last(rec, "d_fake_mean") == tr.logit_stats_emul(fake)[0]
        if mode == "conditional":  # the generator's pass reuses rows [0, B): its statistics are those of the logits its fake labels select
            gp = lg_all[:B][np.arange(B), eng.fake_labels.cpu().numpy()]
            assert _last(rec, "g_frac_pos") == np.float32(np.count_nonzero(gp > 0)) / np.float32(B)
            assert _last(rec, "g_mean") == tr.logit_stats_emul(gp)[0]
        if mode == "fixed_p":  # a fixed probability is not the controller: ADA is off, its fields are NaN
            assert eng.ada_state is not None and np.isnan(_last(rec, "ada_p")) and np.isnan(_last(rec, "ada_rt"))
        if mode == "ada":  # the generator's pass has rows of its own there
            gp = _f32(eng.logits_g).reshape(-1)
            assert _last(rec, "g_frac_pos") == np.float32(np.count_nonzero(gp > 0)) / np.float32(gp.size)
            assert _last(rec, "ada_p") == _f32(eng.ada_state)[0] and _last(rec, "ada_rt") == _f32(eng.ada_state)[3]
        _check_norms(rec, rec["keys_g"], rec["grad_norms_g"][-1], G, f"G ({mode})")
        assert (_last(rec, "loss_d_real"), _last(rec, "loss_d_fake"), _last(rec, "loss_g")) == tuple(_f32(eng.losses))


def test_every_option_field_mirrors_its_engine_attribute():
    eng, D, G = _engine(external_noise=True, telemetry=8, diffaug="color,translation", ada_target=0.6, ada_interval=2, bcr=(1.0, 0.5),
                        lr_schedule="cosine", lr_warmup=1, lr_total=10, lr_final=0.1, r1_gamma=1.0, r1_interval=2, clip_d=5.0, clip_g=0.5,
                        diversity_weight=0.1)
    for i, (real, z) in enumerate(_batches(4)):
        eng.step(real, z)
        rec = eng.history()
        assert list(rec["step"]) == [i + 1]
        assert (_last(rec, "bcr_real"), _last(rec, "bcr_fake")) == tuple(_f32(eng.bcr_losses))
        assert (_last(rec, "ada_p"), _last(rec, "ada_rt")) == (_f32(eng.ada_state)[0], _f32(eng.ada_state)[3])
        assert (_last(rec, "lr_d"), _last(rec, "lr_g")) == tuple(_f32(eng.lr_now)) == tuple(np.float32(v) for v in eng.lr)
        assert _last(rec, "diversity") == _f32(eng.div_loss)[0]
        if i % 2 == 0:  # steps 1 and 3: R1 is due
            assert _last(rec, "penalty") == _f32(eng.r1_loss)[0] and np.isfinite(_last(rec, "penalty"))
        else:
            assert np.isnan(_last(rec, "penalty")), "a step on which lazy R1 is not due"
        # bCR on diffaug: D's pass is [x ; T_1(x)] and the adversarial rows are T_1(x)'s, logits[2B, 4B) - real first, then fake
        lg = _f32(eng.logits)
        assert lg.shape[0] == 4 * B
        real, fake = lg[2 * B:3 * B].reshape(-1), lg[3 * B:].reshape(-1)
        assert _last(rec, "d_real_acc") == np.float32(np.count_nonzero(real > 0)) / np.float32(real.size)
        assert _last(rec, "d_fake_acc") == np.float32(np.count_nonzero(fake < 0)) / np.float32(fake.size)
        assert _last(rec, "d_real_mean") == tr.logit_stats_emul(real)[0] and _last(rec, "d_fake_mean") == tr.logit_stats_emul(fake)[0]
        # the norms are taken behind the clipping: what AdamW consumes
        assert _last(rec, "gnorm_d_l2") <= 5.0 * (1 + 1e-5) and _last(rec, "gnorm_g_l2") <= 0.5 * (1 + 1e-5)
        _check_norms(rec, rec["keys_d"], rec["grad_norms_d"][-1], D, "D, every option on")
        assert (_last(rec, "loss_d_real"), _last(rec, "loss_d_fake"), _last(rec, "loss_g")) == tuple(_f32(eng.losses))


def _dataset():
    from vit_gan_amd.data import DeviceDataset
    g = torch.Generator().manual_seed(9)
    return DeviceDataset(torch.randint(0, 256, (3 * B + 1, 3, 32, 32), generator=g, dtype=torch.uint8), None, flip=True)


def test_run_under_graph_replay_records_every_step_once_and_as_eager_does():
    recs = {}
    for use_graph in (False, True):
        eng, _, _ = _engine(dataset=_dataset(), use_graph=use_graph, telemetry=8)
        eng.run(5)
        recs[use_graph] = eng.history()
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None
        assert list(recs[use_graph]["step"]) == [1, 2, 3, 4, 5] and recs[use_graph]["dropped"] == 0, "the first captured step appears once"
    for k, v in recs[False].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == recs[True][k].tobytes(), f"{k}: replay and eager differ"
    assert np.isfinite(recs[True]["loss_g"]).all() and (recs[True]["gnorm_d_sum"] > 0).all()


def test_ring_wraps_cursor_follows_the_counter_and_nonfinite_is_found():
    eng, D, _ = _engine(external_noise=True, telemetry=4)
    data = _batches(6)
    for real, z in data:
        eng.step(real, z)
    rec = eng.history()
    assert list(rec["step"]) == [3, 4, 5, 6] and rec["dropped"] == 2
    assert len(eng.history()["step"]) == 0, "history() twice in a row"
    assert "tel_ring" not in eng.state_dict() and not any("tel" in k for k in eng.state_dict()), "the rings are a log, not training state"
    saved, weights = eng.state_dict(), [{k: v.clone() for k, v in m.state_dict().items()} for m in (eng._disc, eng.gen)]
    eng.step(*data[0])
    eng.load_state_dict(saved)  # the counter goes back to 6: the record continues behind it
    eng.step(*data[1])
    assert list(eng.history()["step"]) == [7]
    eng.sync_from_modules(reset_optimizer=True)
    eng.step(*data[2])
    assert list(eng.history()["step"]) == [1]
    assert eng.first_nonfinite_step is None
    with torch.no_grad():  # an infinite weight: the next step's gradients are not finite
        D.vit._flat.flat[D.vit._flat.slots["norm.weight"][0]] = float("inf")
    eng.sync_from_modules()
    eng.step(*data[3])
    eng.step(*data[4])
    rec = eng.history()
    assert list(rec["step"]) == [2, 3] and rec["nonfinite_d"][0] > 0 and eng.first_nonfinite_step == 2
    del weights


# ---------------------------------------------------------------------------------------------------------------------------- trainer
CFG = {"epochs": 3, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_trainer_writes_the_record_and_leaves_a_run_without_it_alone(tmp_path):
    from vit_gan_amd.training import train_model
    on = train_model(CFG, max_epochs=2, steps_per_epoch=3, output_base=str(tmp_path / "on"), telemetry=True)
    off = train_model(CFG, max_epochs=2, steps_per_epoch=3, output_base=str(tmp_path / "off"))
    assert on["engine"].tel_cap == 3 and off["engine"].tel_cap == 0 and "telemetry" not in off
    z = np.load(os.path.join(on["dirs"].save, "telemetry.npz"))
    assert list(z["step"]) == [1, 2, 3, 4, 5, 6], "one row per step"
    for name in tr.TEL_FIELDS:
        assert z[name].shape == (6,) and z[name].dtype == np.float32, name
    assert z["grad_norms_d"].shape == (6, len(z["keys_d"])) and z["grad_norms_g"].shape == (6, len(z["keys_g"]))
    assert [str(k) for k in z["keys_d"]] == [k for k, _ in on["discriminator"].named_parameters()]
    assert np.isfinite(z["gnorm_d_sum"]).all() and (z["gnorm_g_sum"] > 0).all()
    log = open(os.path.join(on["dirs"].save, "training.log")).read()
    lines = [ln for ln in log.splitlines() if "Epoch [" in ln]
    assert len(lines) == 2
    for e, ln in enumerate(lines):
        last = 3 * e + 2
        tail = (f" | Disc Real Acc: {z['d_real_acc'][last]:.4f} | Disc Fake Acc: {z['d_fake_acc'][last]:.4f}"
                f" | Grad Norm Gen: {z['gnorm_g_sum'][last]:.4f} | Grad Norm Disc: {z['gnorm_d_sum'][last]:.4f}")
        assert tail in ln, ln
    assert "Non-finite gradient" not in log and "dropped" not in log
    # without the option: today's files, today's lines
    new = {"telemetry.npz", "gradient_norms.png", "accuracies.png"}
    f_on, f_off = _files(on["dirs"].save), _files(off["dirs"].save)
    assert not new & set(f_off) and sorted(set(f_on) - new) == f_off
    try:
        import matplotlib  # noqa: F401
        figures = ["losses.png"]
    except Exception:
        figures = []
    assert "telemetry.npz" in f_on and all((f in f_on) == bool(figures) for f in ("gradient_norms.png", "accuracies.png"))
    want = sorted(["engine_state.pth", "final_model.ckpt", "training.log"] + figures
                  + [f"{d}/{n}_epoch_{e}.png" for d, n in (("images", "samples"), ("input", "input"), ("noise", "noise")) for e in (0, 1)])
    assert f_off == want, f_off
    off_log = open(os.path.join(off["dirs"].save, "training.log")).read()
    assert "Disc Real Acc" not in off_log and "Grad Norm" not in off_log
    # with bCR on, the line carries the record's fields AND the consistency losses (every option combines)
    both = train_model(CFG, max_epochs=1, steps_per_epoch=2, output_base=str(tmp_path / "bcr"), telemetry=True, bcr=(1.0, 0.5), diffaug="color")
    zb = np.load(os.path.join(both["dirs"].save, "telemetry.npz"))
    line = [ln for ln in open(os.path.join(both["dirs"].save, "training.log")).read().splitlines() if "Epoch [0/1]" in ln]
    tail = (f" | Disc Real Acc: {zb['d_real_acc'][1]:.4f} | Disc Fake Acc: {zb['d_fake_acc'][1]:.4f}"
            f" | Grad Norm Gen: {zb['gnorm_g_sum'][1]:.4f} | Grad Norm Disc: {zb['gnorm_d_sum'][1]:.4f}")
    assert len(line) == 1 and tail in line[0] and " | Consistency real: " in line[0], line
    assert list(zb["step"]) == [1, 2] and np.isfinite(zb["bcr_real"]).all()
    with pytest.raises(ValueError, match="telemetry"):
        train_model(CFG, telemetry=0)
    with pytest.raises(ValueError, match="telemetry"):
        train_model(CFG, telemetry=1.5)
