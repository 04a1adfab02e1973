"""The device-side learning-rate schedule on the GPU: the controller kernel (vg_lr_schedule) against the float64 restatement of
tests/lr_ref.py; the device-rate AdamW kernels (vg_adamw_step_dlr / vg_adamw_ema_step_dlr) bit for bit against the float forms; the
engine with a schedule on - eager against a plain engine fed the read-back rates, under hipGraph replay, on the sharded schedule,
across a restart - and off; the trainer's log and its plateau rule.

Bound of the controller: the kernel evaluates base f scale in fp64 and rounds ONCE to fp32, the restatement evaluates the same in
Python float64, so |lr_out - lr_ref| <= 1 ulp32(lr_ref): half an ulp of rounding, and the two fp64 values (they differ only by the
cosine, ~1e-16 relative) can straddle one rounding boundary and no more.  Where the factor is an explicit branch (1, or ``final``) both
sides perform the same two IEEE fp64 products, so the result is fp32(lr_ref) bit for bit.  Everything else here is equality."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import engine_util as eu
import lr_ref
import step_trace as stt
from adamw_ref import check_adamw_step, f32, ulp32
import gpu_util as u

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LR_D, LR_G = 5e-4, 2e-4  # two base rates: a rate applied to the wrong network cannot go unseen
COS = dict(lr_schedule="cosine", lr_warmup=3, lr_total=8, lr_final=0.1)


def _within_one_ulp(got: float, want: float) -> bool:
    return abs(got - want) <= float(ulp32(torch.tensor(want, dtype=torch.float64)))


# ----------------------------------------------------------------------------------------------------------------- the controller
def test_controller_matches_the_fp64_restatement():
    """Every kind x warmup {0, 1, 3} x total {warmup + 1, 8} x final {0, 0.1, 1} x scale {1, 0.5, 1/3} at every t in [1, total + 2]:
    slot 0 carries the case on LR_D, slot 1 the same schedule on LR_G with the NEXT scale of the list, so the two slots of a launch
    never hold the same numbers."""
    from vit_gan_amd import ops
    scales = (1.0, 0.5, 1.0 / 3.0)
    ts = torch.arange(0, 16, dtype=torch.int32, device="cuda")
    pairs = [torch.tensor([scales[i], scales[(i + 1) % 3]], dtype=torch.float32, device="cuda") for i in range(3)]
    cases = []
    for kind in lr_ref.KINDS:
        for warmup in (0, 1, 3):
            for total in (warmup + 1, 8):
                for final in (0.0, 0.1, 1.0):
                    for i in range(3):
                        for t in range(1, total + 3):
                            cases.append((kind, warmup, total, final, i, t))
    out = torch.full((len(cases), 2), float("nan"), dtype=torch.float32, device="cuda")
    for row, (kind, warmup, total, final, i, t) in enumerate(cases):
        ops.lr_schedule(ts[t:t + 1], (LR_D, kind, warmup, total, final), (LR_G, kind, warmup, total, final), pairs[i], out[row])
    torch.cuda.synchronize()
    got = out.cpu().double().tolist()
    worst, n_exact, n_base = 0.0, 0, 0
    for (kind, warmup, total, final, i, t), row in zip(cases, got):
        for slot, (base, scale) in enumerate(((LR_D, scales[i]), (LR_G, scales[(i + 1) % 3]))):
            want = lr_ref.lr_now(base, kind, t, warmup, total, final, f32(scale))
            what = f"{kind} warmup={warmup} total={total} final={final} scale={scale} t={t} slot {slot}: got {row[slot]!r} want {want!r}"
            ulp = float(ulp32(torch.tensor(want, dtype=torch.float64)))
            if want == 0.0:
                assert row[slot] == 0.0, what
                continue
            worst = max(worst, abs(row[slot] - want) / ulp)
            assert abs(row[slot] - want) <= ulp, what
            if lr_ref.exact(kind, t, warmup, total):  # an explicit branch: the same two fp64 products on both sides
                n_exact += 1
                assert row[slot] == float(np.float32(want)), f"{what}: not bit-equal on an exact branch"
                if scale == 1.0 and lr_ref.factor(kind, t, warmup, total, final) == 1.0:
                    n_base += 1
                    assert row[slot] == f32(base), f"{what}: factor and scale 1 must give the base rate's bits"
    assert n_exact > 1000 and n_base > 100
    print(f"\ncontroller: {2 * len(cases)} rates, worst {worst:.3f} ulp32, {n_exact} on exact branches, {n_base} equal to the base rate")


def test_controller_counter_zero_counts_as_one_and_slots_keep_to_their_scale():
    """A counter below 1 (the counter before the first vg_zero_tick, a cleared one) is DEFINED: it counts as t = 1.  A slot reads its
    own scale only: a NaN in the other one does not reach it."""
    from vit_gan_amd import ops
    d, g = (LR_D, "cosine", 3, 8, 0.1), (LR_G, "linear", 2, 9, 0.25)
    step = lambda t: torch.tensor([t], dtype=torch.int32, device="cuda")  # noqa: E731
    one = ops.lr_schedule(step(1), d, g).cpu()
    for t in (0, -1, -2 ** 31):
        assert torch.equal(ops.lr_schedule(step(t), d, g).cpu().view(torch.int32), one.view(torch.int32)), t
    assert _within_one_ulp(float(one[0]), lr_ref.lr_now(LR_D, "cosine", 1, 3, 8, 0.1)) and _within_one_ulp(float(one[1]), lr_ref.lr_now(LR_G, "linear", 1, 2, 9, 0.25))
    nan = float("nan")
    both = ops.lr_schedule(step(5), d, g, torch.tensor([0.5, 0.75], device="cuda")).cpu()
    a = ops.lr_schedule(step(5), d, g, torch.tensor([0.5, nan], device="cuda")).cpu()
    b = ops.lr_schedule(step(5), d, g, torch.tensor([nan, 0.75], device="cuda")).cpu()
    assert float(a[0]) == float(both[0]) and bool(torch.isnan(a[1])) and float(b[1]) == float(both[1]) and bool(torch.isnan(b[0]))
    # the two slots run their own schedules
    assert _within_one_ulp(float(both[0]), lr_ref.lr_now(LR_D, "cosine", 5, 3, 8, 0.1, 0.5))
    assert _within_one_ulp(float(both[1]), lr_ref.lr_now(LR_G, "linear", 5, 2, 9, 0.25, 0.75))
    # a refused call writes nothing
    out = torch.full((2,), -7.0, device="cuda")
    with pytest.raises(RuntimeError, match="argument validation -2"):
        ops.lr_schedule(step(5), (LR_D, "cosine", 3, 3, 0.1), g, out=out)
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0]


# ----------------------------------------------------------------------------------------------------------- device-rate AdamW
GUARD = 1028  # elements in front of and behind every range: a multiple of 4, not of 1024


def _state(n, seed):
    """gpu_util.adamw_state and an average near and far from p"""
    p, m, v, g, gen = u.adamw_state(n, seed)
    e = p - p * 1e-3 * torch.randn(n, generator=gen)
    return p, m, v, g, e


@pytest.mark.parametrize("n", [4, 4096, 4100])
def test_device_rate_adamw_is_the_float_form_bit_for_bit(n):
    """n = 4: one thread; 4096: whole workgroups; 4100: a last workgroup with one live thread.  Three counter values, gscale 1 and 0.5,
    both slots of a rate pair that a controller launch has just written on the same stream."""
    from vit_gan_amd import ops
    total = n + 2 * GUARD
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 1e-3
    worst = 0.0
    for t in (1, 7, 1000):
        for gscale in (1.0, 0.5):
            for slot in (0, 1):
                what = f"n={n} t={t} gscale={gscale} slot {slot}"
                p0, m0, v0, g, e0 = _state(total, 13 * t + slot + n)
                step_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
                dl = {name: [u.dev(x.clone()) for x in (p0, g, m0, v0)] + [torch.full((total,), -7.0, dtype=BF, device="cuda"), u.dev(e0.clone())]
                      for name in ("adam", "ema")}
                rates = ops.lr_schedule(step_dev, (LR_D, "cosine", 3, 2000, 0.1), (LR_G, "linear", 0, 1500, 0.0))
                lr_dev = rates[slot:slot + 1]
                tail = (b1, b2, eps, wd, 0, u.ptr(step_dev), gscale)
                u.call("vg_adamw_step_dlr", *(u.off(x, GUARD) for x in dl["adam"][:5]), n, u.ptr(lr_dev), *tail, u.stream())
                u.call("vg_adamw_ema_step_dlr", *(u.off(x, GUARD) for x in dl["ema"]), n, u.ptr(lr_dev), *tail, 0.999, 0, u.stream())
                lr = float(lr_dev[0])  # (synchronises) the float the kernels read
                assert lr > 0 and _within_one_ulp(lr, lr_ref.lr_now(LR_G, "linear", t, 0, 1500, 0.0) if slot else lr_ref.lr_now(LR_D, "cosine", t, 3, 2000, 0.1))
                fl = {name: [u.dev(x.clone()) for x in (p0, g, m0, v0)] + [torch.full((total,), -7.0, dtype=BF, device="cuda"), u.dev(e0.clone())]
                      for name in ("adam", "ema")}
                u.call("vg_adamw_step", *(u.off(x, GUARD) for x in fl["adam"][:5]), n, lr, *tail, u.stream())
                u.call("vg_adamw_ema_step", *(u.off(x, GUARD) for x in fl["ema"]), n, lr, *tail, 0.999, 0, u.stream())
                u.sync()
                assert int(step_dev[0]) == t and float(lr_dev[0]) == lr, f"{what}: the counter or the rate was written"
                for name in ("adam", "ema"):
                    for buf, a, b in zip(("p", "g", "m", "v", "shadow", "average"), dl[name], fl[name]):
                        if name == "adam" and buf == "average":
                            assert torch.equal(a.cpu(), e0), f"{what}: vg_adamw_step_dlr has no average to write"
                            continue
                        bits = torch.int16 if a.dtype == BF else torch.int32
                        assert torch.equal(a.view(bits), b.view(bits)), f"{what}: {name} {buf} differs from the float form's"
                    P, G_, M, V, SH, E = (x.cpu() for x in dl[name])
                    s = slice(GUARD, GUARD + n)
                    frac, _ = check_adamw_step(p0[s], m0[s], v0[s], g[s], t, (lr, b1, b2, eps, wd), gscale, P[s], M[s], V[s], SH[s], f"{what} {name}")
                    worst = max(worst, frac)
                    outside = torch.ones(total, dtype=torch.bool)
                    outside[s] = False
                    for buf, x, ref in (("p", P, p0), ("m", M, m0), ("v", V, v0), ("average", E, e0)):
                        assert torch.equal(x[outside], ref[outside]), f"{what}: {name} {buf} written outside its range"
                    assert bool((SH[outside] == -7.0).all()) and torch.equal(G_, g), f"{what}: {name} wrote its guard band or the gradient"
    print(f"\ndevice-rate AdamW n={n}: worst {worst:.4f} of the fp64 bound")


def test_refused_device_rate_calls_launch_nothing():
    from vit_gan_amd import _lib
    n = 4096
    P, G_, M, V, E = (torch.full((n,), 0.25, device="cuda") for _ in range(5))
    SH = torch.zeros(n, dtype=BF, device="cuda")
    step_dev = torch.ones(1, dtype=torch.int32, device="cuda")
    lr = torch.full((1,), 1e-3, device="cuda")
    L = _lib.lib()
    hyp = (0.9, 0.999, 1e-8, 1e-3)
    four = (u.ptr(P), u.ptr(G_), u.ptr(M), u.ptr(V), u.ptr(SH))
    assert L.vg_adamw_step_dlr(*four, n - 2, u.ptr(lr), *hyp, 0, u.ptr(step_dev), 1.0, u.stream()) == -3
    assert L.vg_adamw_step_dlr(*four, n, None, *hyp, 0, u.ptr(step_dev), 1.0, u.stream()) == -1
    assert L.vg_adamw_step_dlr(*four, n, u.ptr(lr), *hyp, 0, None, 1.0, u.stream()) == -1
    for nn_, lrp, decay, start, want in ((n - 2, lr, 0.999, 0, -3), (n, None, 0.999, 0, -1), (n, lr, 1.0, 0, -2), (n, lr, 0.999, -1, -2)):
        assert L.vg_adamw_ema_step_dlr(*four, u.ptr(E), nn_, u.ptr(lrp), *hyp, 0, u.ptr(step_dev), 1.0, decay, start, u.stream()) == want
    assert L.vg_adamw_ema_step_dlr(*four, None, n, u.ptr(lr), *hyp, 0, u.ptr(step_dev), 1.0, 0.999, 0, u.stream()) == -1
    u.sync()
    assert all(bool((x == 0.25).all()) for x in (P, G_, M, V, E)) and bool((SH == 0).all()) and float(lr) == float(np.float32(1e-3)), \
        "a refused call launched a kernel"


# ------------------------------------------------------------------------------------------------------------------------ engine
def _run(eng, n, skip=0, before=None):
    """n steps; ``before(eng, k)`` runs ahead of step k (1-based over the whole run).  Returns the losses and, with a schedule on, the
    rates read back after each step."""
    losses, rates = [], []
    for k, (real, z) in enumerate(eu.batches(stt.B, n, skip=skip), start=skip + 1):
        if before is not None:
            before(eng, k)
        losses.append(eng.step(real, z).clone())
        if eng.lr_opts is not None:
            rates.append(eng.lr)
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), rates


def _snapshot(eng):
    fd, fg = eng.vit._flat, eng.gen._flat
    ts = [fd.flat, fd.shadow, fg.flat, fg.shadow, eng.m_d, eng.v_d, eng.m_g, eng.v_g, eng.step_t] + ([] if eng.ema_g is None else [eng.ema_g])
    return [t.detach().clone().cpu() for t in ts]


def _same(a, b, what):
    assert len(a) == len(b), what
    names = ("D master", "D shadow", "G master", "G shadow", "m_d", "v_d", "m_g", "v_g", "step_t", "ema_g")
    for name, x, y in zip(names, a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


def _check_rates(rates, scale_of, what):
    """the read-back pairs of steps 1.. against the restatement (COS on LR_D / LR_G), within the controller's bound"""
    for k, (d, g) in enumerate(rates, start=1):
        sd, sg = scale_of(k)
        for got, base, s in ((d, LR_D, sd), (g, LR_G, sg)):
            want = lr_ref.lr_now(base, "cosine", k, 3, 8, 0.1, s)
            assert _within_one_ulp(got, want), f"{what}: step {k}: rate {got!r}, restatement {want!r}"


@functools.lru_cache(maxsize=None)
def _plain_trace():
    return stt.trace()


def test_off_is_off():
    """The default engine allocates no rate buffers, and its two steps make the calls the fixture recorded for the plain step."""
    eng = stt.engine()
    try:
        assert eng.lr_opts is None and eng.lr_scale is None and eng.lr_now is None and len(eng._state_tensors()) == 9
        assert "lr" not in eng.state_dict() and "lr_scale" not in eng.state_dict() and eng.lr == (5e-4, 5e-4)
        with pytest.raises(RuntimeError, match="no learning-rate schedule"):
            eng.set_lr_scale(d=0.5)
    finally:
        eng.close()
    calls, ext = _plain_trace()
    with open(stt.FIXTURE) as f:
        want = json.load(f)["traces"]["plain"]
    assert ext == 0 and calls == want
    assert not any("dlr" in c[0] or c[0] == "vg_lr_schedule" for c in calls)
    off, ext = stt.trace(lr_schedule="", lr_warmup=0, lr_total=0, lr_final=0.0)
    assert ext == 0 and off == calls


def test_constant_schedule_is_the_plain_step_plus_one_launch():
    """constant, no warm-up, scale 1: the factor is exactly 1, so four steps are bit for bit the plain engine's; the call list is the
    plain one with one vg_lr_schedule behind each vg_zero_tick and the _dlr names, reading D's rate at lr_now[0] and G's at lr_now[1]."""
    plain = stt.engine()
    l0, _ = _run(plain, 4)
    s0 = _snapshot(plain)
    plain.close()
    eng = stt.engine(lr_schedule="constant")
    assert eng.lr_opts == ("constant", 0, 0, 0.0) and len(eng._state_tensors()) == 10
    l1, rates = _run(eng, 4)
    _same(_snapshot(eng), s0, "constant schedule against no schedule")
    eng.close()
    assert torch.equal(l1, l0) and rates == [(f32(5e-4), f32(5e-4))] * 4
    calls, ext = stt.trace(lr_schedule="constant")
    want, _ = _plain_trace()
    assert ext == 0
    names = [c[0] for c in calls]
    assert names.count("vg_lr_schedule") == stt.STEPS
    for i, nm in enumerate(names):
        if nm == "vg_lr_schedule":
            assert names[i - 1] == "vg_zero_tick", "the controller runs directly behind the tick"
    assert [nm[:-4] if nm.endswith("_dlr") else nm for nm in names if nm != "vg_lr_schedule"] == [c[0] for c in want]
    assert not any(nm in ("vg_adamw_step", "vg_adamw_ema_step") for nm in names) and names.count("vg_adamw_step_dlr") == 2 * stt.STEPS
    sched = [c[1] for c in calls if c[0] == "vg_lr_schedule"]
    lr_now = sched[0][4]
    assert lr_now[1] == 0 and all(s[4] == lr_now for s in sched)
    d_s, g_s = sched[0][0], sched[0][1]
    assert d_s == g_s == [f32(5e-4), 0, 0, 0, 0.0]
    adam = [c[1] for c in calls if c[0] == "vg_adamw_step_dlr"]
    assert [a[6] for a in adam] == [[lr_now[0], 0], [lr_now[0], 4]] * stt.STEPS, "D reads slot 0, G slot 1"


def test_cosine_schedule_is_the_plain_engine_fed_the_read_back_rates():
    """Ten eager steps of cosine / warm-up 3 / total 8 / final 0.1 on two different base rates: the rates in force against the
    restatement, and the whole trajectory bit-equal to a plain engine whose hyp["lr_d"] / hyp["lr_g"] are set, before each step, to
    the values read back - a rate on the wrong network or a step late cannot pass."""
    eng = stt.engine(lr_d=LR_D, lr_g=LR_G, **COS)
    l1, rates = _run(eng, 10)
    s1 = _snapshot(eng)
    eng.close()
    _check_rates(rates, lambda k: (1.0, 1.0), "eager")
    assert len({r[0] for r in rates[:8]}) == 8 and rates[7] == rates[8] == rates[9] and all(d != g for d, g in rates)
    assert rates[2] == (f32(LR_D), f32(LR_G)), "t = warmup: the base rates' bits"

    def feed(plain, k):
        plain.hyp["lr_d"], plain.hyp["lr_g"] = rates[k - 1]
    plain = stt.engine(lr_d=1.0, lr_g=1.0)  # (rates that would wreck the run if one were ever used)
    l0, _ = _run(plain, 10, before=feed)
    _same(_snapshot(plain), s1, "scheduled engine against the plain engine fed its rates")
    plain.close()
    assert torch.equal(l0, l1)


def test_two_stream_schedule_reads_the_rates_too():
    """The two-chain schedule of the step has its own tick and AdamW calls: four eager steps at the scheduled rates, bit-equal to the
    plain two-stream engine fed the read-back rates."""
    eng = stt.engine(two_stream=True, lr_d=LR_D, lr_g=LR_G, **COS)
    l1, rates = _run(eng, 4)
    s1 = _snapshot(eng)
    eng.close()
    _check_rates(rates, lambda k: (1.0, 1.0), "two_stream")

    def feed(plain, k):
        plain.hyp["lr_d"], plain.hyp["lr_g"] = rates[k - 1]
    plain = stt.engine(two_stream=True, lr_d=1.0, lr_g=1.0)
    l0, _ = _run(plain, 4, before=feed)
    _same(_snapshot(plain), s1, "two_stream: scheduled engine against the plain engine fed its rates")
    plain.close()
    assert torch.equal(l0, l1)


GRAPH_CONFIGS = {
    "plain": {},
    "ema": dict(ema_decay=0.999),
    "diffaug_spectral_r1": dict(diffaug=stt.AUG, spectral_norm="all", r1_gamma=1.0, r1_interval=2),
}


@pytest.mark.parametrize("name", list(GRAPH_CONFIGS))
def test_graph_replay_follows_the_schedule_and_the_multipliers(name):
    """Ten replays == ten eager steps bit for bit with a rate that moves from replay to replay, and set_lr_scale(d=0.5) before step 7
    takes effect on that replay with no new capture (lazy R1: two graphs, one schedule)."""
    kw = dict(lr_d=LR_D, lr_g=LR_G, **COS, **GRAPH_CONFIGS[name])

    def halve(eng, k):
        if k == 7:
            if eng.graph_active:
                halve.graphs = dict(eng._graphs)
            eng.set_lr_scale(d=0.5)
    eager = stt.engine(**kw)
    l0, r0 = _run(eager, 10, before=halve)
    s0 = _snapshot(eager)
    eager.close()
    graph = stt.engine(use_graph=True, **kw)
    l1, r1 = _run(graph, 10, before=halve)
    assert graph.graph_active and graph.graph_fallback_reason is None
    kinds = 2 if "r1_gamma" in kw else 1
    assert len(graph._graphs) == kinds and graph._graphs == halve.graphs and all(graph._graphs[k] is halve.graphs[k] for k in halve.graphs), \
        "set_lr_scale must not cost a capture"
    _same(_snapshot(graph), s0, f"{name}: replayed against eager")
    assert graph.lr_scales == (0.5, 1.0)
    graph.close()
    assert torch.equal(l1, l0) and r1 == r0
    _check_rates(r1, lambda k: (0.5 if k >= 7 else 1.0, 1.0), name)
    assert len({r[0] for r in r1[:8]}) == 8, "a fresh rate every replay"
    assert r1[8][0] == r1[7][0] and _within_one_ulp(r1[7][0], 0.5 * f32(LR_D) * f32(0.1))


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
                        exchange_single_rank=shard, shard_mapping_update=shard, lr_d=5e-4, lr_g=2e-4, lr_schedule="cosine", lr_warmup=2,
                        lr_total=5, lr_final=0.1)
        assert eng.shard_map == shard and eng.sync.active == shard
        ls, rates = [], []
        for real, z in eu.batches(B, 4, seed=9):
            ls.append(eng.step(real, z).clone())
            rates.append(eng.lr)
        torch.cuda.synchronize()
        res.append((torch.stack(ls).cpu(), G._flat.flat.detach().cpu().clone(), eng.ema_g.detach().cpu().clone(), eng.graph_active,
                    eng.graph_fallback_reason, rates))
        eng.close()
    plain, shard_eager, shard_graph = res
    report = {"graph": shard_graph[3] and shard_graph[4] is None,
              "scheduled": len({r[1] for r in plain[5]}) == 4 and plain[5] == shard_eager[5] == shard_graph[5],
              "eager_master": torch.equal(shard_eager[1], plain[1]), "eager_ema": torch.equal(shard_eager[2], plain[2]),
              "graph_master": torch.equal(shard_graph[1], plain[1]), "graph_ema": torch.equal(shard_graph[2], plain[2]),
              "losses": torch.equal(shard_eager[0], plain[0]) and torch.equal(shard_graph[0], plain[0])}
    return report


@pytest.mark.timeout(300)
def test_sharded_update_follows_the_schedule():
    """shard_mapping_update on a one-rank RCCL group with the schedule on (every piece of the generator's sharded AdamW is a _dlr call
    on slot 1), eager and captured, against the replicated scheduled engine: master and average bit for bit.  A fresh spawned process."""
    (val,) = eu.run_ranks(_shard_worker, 1, 240, backend="nccl", gpu=True)
    assert all(val.values()), val


class _Gan(torch.nn.Module):
    def __init__(self, D, G):
        super().__init__()
        self.discriminator, self.generator = D, G


@pytest.mark.parametrize("use_graph", [False, True])
def test_resume_continues_the_schedule_bit_for_bit(use_graph):
    """5 steps, state_dict(), a new engine on other initial weights, load both states, 5 more == 10 uninterrupted steps, with the
    generator's multiplier changed before step 3 carried across; mismatched options raise under strict."""
    kw = dict(lr_d=LR_D, lr_g=LR_G, use_graph=use_graph, **COS)

    def quarter(eng, k):
        if k == 3:
            eng.set_lr_scale(g=0.25)
    ref = stt.engine(**kw)
    ref_l, ref_r = _run(ref, 10, before=quarter)
    ref_s = _snapshot(ref)
    ref.close()
    _check_rates(ref_r, lambda k: (1.0, 0.25 if k >= 3 else 1.0), "uninterrupted")
    first = stt.engine(**kw)
    l_a, r_a = _run(first, 5, before=quarter)
    gan_state = {k: v.clone() for k, v in _Gan(first._disc, first.gen).state_dict().items()}
    state = first.state_dict()
    first.close()
    assert tuple(state["lr"]) == ("cosine", 3, 8, 0.1) and state["lr_scale"].tolist() == [1.0, 0.25] and int(state["step_t"]) == 5
    second = stt.engine(**kw)
    with torch.no_grad():
        for p in list(second._disc.parameters()) + list(second.gen.parameters()):
            p.add_(0.01)
    _Gan(second._disc, second.gen).load_state_dict(gan_state, strict=True)
    second.load_state_dict(state)
    assert second.lr_scales == (1.0, 0.25)
    l_b, r_b = _run(second, 5, skip=5)
    _same(_snapshot(second), ref_s, "resumed against uninterrupted")
    assert torch.equal(torch.cat([l_a, l_b]), ref_l) and r_a + r_b == ref_r
    # options: strict compares them like R1's; strict=False loads the multipliers all the same
    other = stt.engine(lr_d=LR_D, lr_g=LR_G, lr_schedule="cosine", lr_warmup=3, lr_total=9, lr_final=0.1)
    with pytest.raises(ValueError, match="learning-rate schedule"):
        other.load_state_dict(state)
    other.load_state_dict(state, strict=False)
    assert other.lr_scales == (1.0, 0.25)
    other.close()
    plain = stt.engine()
    with pytest.raises(ValueError, match="learning-rate schedule"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="learning-rate schedule"):
        second.load_state_dict(plain.state_dict())
    plain.load_state_dict(state, strict=False)
    plain.close()
    second.close()


# ----------------------------------------------------------------------------------------------------------------------- trainer
CFG = {"epochs": 3, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}


def test_trainer_logs_the_schedule_and_the_rates(tmp_path):
    from vit_gan_amd.config import Config
    from vit_gan_amd.training import train_model
    out = train_model(CFG, lr_schedule="cosine", lr_warmup=2, lr_final=0.1, max_epochs=1, steps_per_epoch=4, output_base=str(tmp_path))
    eng, c = out["engine"], Config(**CFG)
    assert eng.lr_opts == ("cosine", 2, 4, 0.1), "lr_total=None is epochs * len(loader)"
    log = open(os.path.join(out["dirs"].save, "training.log")).read()
    assert "Learning-rate schedule: cosine, 2 warm-up step(s), to 0.1 x base at step 4" in log
    m = re.findall(r"Epoch \[0/1\].*\| lr_d: (\S+), lr_g: (\S+)", log)
    assert len(m) == 1, log
    for got, base in zip(m[0], (c.discriminator_learning_rate, c.generator_learning_rate)):
        want = lr_ref.lr_now(base, "cosine", 4, 2, 4, 0.1)
        assert _within_one_ulp(float(got), want) and np.float32(float(got)) == np.float32(want), (got, want)  # (t >= total: an exact branch)
    assert tuple(np.float32(x) for x in eng.lr) == tuple(np.float32(float(x)) for x in m[0]), "the line carries the rates to float32 precision"


def test_trainer_plateau_rule_is_reduce_lr_on_plateau(tmp_path):
    from vit_gan_amd.training import train_model
    series = [20.0, 20.0, 20.0]
    out = train_model(CFG, lr_plateau=(0.5, 1), fid_fn=lambda gan, epoch: series[epoch], max_epochs=3, steps_per_epoch=2, output_base=str(tmp_path))
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=1)
    for m in series:
        sch.step(m)
    want = opt.param_groups[0]["lr"]
    eng = out["engine"]
    assert want == 0.5 and eng.lr_scales == (want, want) and eng.lr_opts == ("constant", 0, 0, 0.0)
    log = open(os.path.join(out["dirs"].save, "training.log")).read()
    assert log.count("FID plateau") == 1 and "Learning-rate schedule: constant" in log
