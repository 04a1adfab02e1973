"""The device-side learning-rate schedule without a GPU: the C ABI of the three exports and their host-side return codes, the option
parsers, every argument error of the engine and the trainer before the device check, and the invariants of the float64 restatement
(tests/lr_ref.py).  The ABI, parser and argument tests fail on the parent commit: the exports and the keyword arguments are this
feature's."""
import ctypes as C
import math
import os

import pytest
import torch

import lr_ref
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib, ops
from vit_gan_amd.config import Config

NEW = ("vg_lr_schedule", "vg_adamw_step_dlr", "vg_adamw_ema_step_dlr")


def test_exports_exist_with_abi_9():
    lib = _lib.lib()
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitgan_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib._SIGNATURES and f"int {name}(" in header, name
    assert "typedef struct VgLrSched" in header
    assert [f[0] for f in _lib.VgLrSched._fields_] == ["base", "kind", "warmup", "total", "final_ratio"] and C.sizeof(_lib.VgLrSched) == 20
    for name, value in (("VG_LR_CONSTANT", 0), ("VG_LR_LINEAR", 1), ("VG_LR_COSINE", 2)):
        assert f"#define {name} {value}" in header
    assert ops.LR_KINDS == {"constant": 0, "linear": 1, "cosine": 2}
    # the _dlr signatures are the float forms' with the pointer in the place of the float
    for a, b in (("vg_adamw_step", "vg_adamw_step_dlr"), ("vg_adamw_ema_step", "vg_adamw_ema_step_dlr")):
        fa, fb = _lib._SIGNATURES[a][1], _lib._SIGNATURES[b][1]
        diff = [i for i, (x, y) in enumerate(zip(fa, fb)) if x is not y]
        assert len(fa) == len(fb) and len(diff) == 1 and fa[diff[0]] is C.c_float and fb[diff[0]] is C.c_void_p


def _sched(base=5e-4, kind=2, warmup=3, total=8, final=0.1):
    return C.byref(_lib.VgLrSched(base, kind, warmup, total, final))


def test_return_codes_come_back_before_any_launch():
    lib, p = _lib.lib(), C.c_void_p(64)  # (a non-null dummy: never dereferenced on these paths; no device here)
    ok = _sched()
    for a in ((None, ok, p, p, p), (ok, None, p, p, p), (ok, ok, None, p, p), (ok, ok, p, None, p), (ok, ok, p, p, None)):
        assert lib.vg_lr_schedule(*a, None) == -1, "a null pointer (step_dev is required)"
    nan, inf = float("nan"), float("inf")
    bad = (dict(kind=3), dict(kind=-1), dict(warmup=-1), dict(kind=1, total=3), dict(kind=2, total=2), dict(kind=2, warmup=0, total=0),
           dict(final=-0.01), dict(final=1.01), dict(final=nan), dict(base=0.0), dict(base=-1e-3), dict(base=inf), dict(base=nan))
    for kw in bad:
        assert lib.vg_lr_schedule(_sched(**kw), ok, p, p, p, None) == -2, kw
        assert lib.vg_lr_schedule(ok, _sched(**kw), p, p, p, None) == -2, kw
    hyp = (0.9, 0.999, 1e-8, 1e-3)
    adam = lambda n=8, lr=p, bufs=(p,) * 5, step=0, sd=p: lib.vg_adamw_step_dlr(*bufs, n, lr, *hyp, step, sd, 1.0, None)  # noqa: E731
    ema = lambda n=8, lr=p, bufs=(p,) * 6, step=0, sd=p, d=0.999, s=0: lib.vg_adamw_ema_step_dlr(*bufs, n, lr, *hyp, step, sd, 1.0, d, s, None)  # noqa: E731
    assert adam(lr=None) == -1 and ema(lr=None) == -1, "lr_dev is required"
    assert adam(n=0) == -1 and ema(n=0) == -1 and adam(sd=None) == -1 and ema(sd=None) == -1, "no size, no step"
    for i in range(5):
        assert adam(bufs=tuple(None if j == i else p for j in range(5))) == -1
    for i in range(6):
        assert ema(bufs=tuple(None if j == i else p for j in range(6))) == -1
    assert adam(n=6) == -3 and ema(n=10) == -3, "n % 4"
    assert ema(d=1.0) == -2 and ema(d=-0.1) == -2 and ema(s=-1) == -2


def test_parse_lr_schedule():
    P = ops.parse_lr_schedule
    assert P("", 0, 0, 0.0) is None, "off"
    assert P("", 3, 0, 0.0) == ("constant", 3, 0, 0.0), "a warm-up alone means constant"
    assert P("constant", 0, 0, 0.0) == ("constant", 0, 0, 0.0)
    assert P("constant", 2, 100, 0.5) == ("constant", 2, 0, 0.0), "constant reads neither total nor final"
    assert P("linear", 0, 1, 0) == ("linear", 0, 1, 0.0) and P("cosine", 3, 8, 0.1) == ("cosine", 3, 8, 0.1) and P("cosine", 3, 4, 1) == ("cosine", 3, 4, 1.0)
    for kind in ("cos", "Cosine", "exponential", None, 2):
        with pytest.raises(ValueError, match="lr_schedule"):
            P(kind, 0, 10, 0.0)
    for w in (-1, 1.0, True, "3", None, 2 ** 31):
        with pytest.raises(ValueError, match="lr_warmup"):
            P("cosine", w, 10, 0.0)
    for t in (-1, 10.0, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="lr_total"):
            P("cosine", 0, t, 0.0)
    for f in (-0.1, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="lr_final"):
            P("cosine", 0, 10, f)
    for kind in ("linear", "cosine"):
        for w, t in ((0, 0), (3, 3), (5, 4)):
            with pytest.raises(ValueError, match="lr_total > lr_warmup"):
                P(kind, w, t, 0.0)
    for t, f in ((10, 0.0), (0, 0.5)):
        with pytest.raises(ValueError, match="without a schedule"):
            P("", 0, t, f)


def _nets():
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, dropout_rate=0.0, batch_size=4, transformer_blocks_count=1))
    return D, SirenGenerator(latent=64, embed=128, heads=4, layers=1, siren_hidden=128, dropout=0.0)


def test_engine_raises_option_errors_without_a_device():
    from vit_gan_amd import engine
    D, G = _nets()
    for kw, match in ((dict(lr_schedule="step"), "lr_schedule"), (dict(lr_schedule="cosine", lr_warmup=-1, lr_total=8), "lr_warmup"),
                      (dict(lr_schedule="cosine", lr_warmup=3, lr_total=3), "lr_total > lr_warmup"), (dict(lr_schedule="linear"), "lr_total > lr_warmup"),
                      (dict(lr_schedule="cosine", lr_total=8, lr_final=2.0), "lr_final"), (dict(lr_total=8), "without a schedule"),
                      (dict(lr_final=0.1), "without a schedule"), (dict(lr_schedule="cosine", lr_total=8, lr_d=0.0), "lr_d"),
                      (dict(lr_warmup=2, lr_g=float("inf")), "lr_g"), (dict(lr_schedule="constant", lr_g=-1e-4), "lr_g")):
        with pytest.raises(ValueError, match=match):
            engine.GanEngine(D, G, batch=4, **kw)
    # what is allowed gets as far as the device check - beside every other option and on both schedules of the step
    for kw in (dict(), dict(lr_schedule="constant"), dict(lr_warmup=3), dict(lr_schedule="cosine", lr_warmup=3, lr_total=8, lr_final=0.1),
               dict(lr_schedule="linear", lr_total=1), dict(lr_schedule="cosine", lr_total=8, two_stream=True),
               dict(lr_schedule="cosine", lr_total=8, ema_decay=0.99, diffaug="color", spectral_norm="all", r1_gamma=1.0, r1_interval=2),
               dict(lr_schedule="cosine", lr_total=8, exchange_single_rank=True, shard_mapping_update=True)):
        with pytest.raises(RuntimeError, match="cuda"):
            engine.GanEngine(D, G, batch=4, **kw)


def test_trainer_raises_option_errors_without_a_device():
    from vit_gan_amd.training import Plateau, train_model
    fid = lambda gan, epoch: 20.0  # noqa: E731
    for kw, match in ((dict(lr_schedule="step"), "lr_schedule"), (dict(lr_schedule="cosine", lr_warmup=10, lr_total=10), "lr_total > lr_warmup"),
                      (dict(lr_schedule="cosine", lr_final=-1), "lr_final"), (dict(lr_warmup=1.5), "lr_warmup"),
                      (dict(lr_total=10), "without a schedule"),
                      # lr_total=None is the whole run: 2 epochs of 3 steps cannot hold a warm-up of 6
                      (dict(lr_schedule="cosine", lr_warmup=6, max_epochs=2, steps_per_epoch=3), "lr_total=6, lr_warmup=6"),
                      (dict(lr_plateau=(0.5, 1)), "fid_fn"), (dict(lr_plateau=(1.5, 1), fid_fn=fid), "factor"),
                      (dict(lr_plateau=(0.5, -1), fid_fn=fid), "patience"), (dict(lr_plateau=0.5, fid_fn=fid), "pair")):
        with pytest.raises(ValueError, match=match):
            train_model(save_artifacts=False, **kw)
    # torch's rule on a series: ReduceLROnPlateau(mode="min", factor=0.5, patience=1) on a dummy optimizer at rate 1
    for series in ((20.0, 20.0, 20.0), (20.0, 19.0, 19.0, 19.0, 19.0, 19.0), (5.0, 4.0, 3.0), (3.0, float("nan"), float("nan"), 2.0, 2.0, 2.0)):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=1)
        rule, scale = Plateau(0.5, 1), 1.0
        for m in series:
            sch.step(m)
            if rule.step(m):
                scale *= 0.5
            assert scale == opt.param_groups[0]["lr"], (series, m)


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_restated_factor_invariants():
    F = lr_ref.factor
    for t in range(0, 40):
        assert F("constant", t, 0, 0, 0.0) == 1.0, "constant without warm-up is exactly 1"
    for kind in lr_ref.KINDS:
        for warmup in (1, 3, 7):
            assert F(kind, warmup, warmup, warmup + 5, 0.1) == 1.0, "the warm-up reaches exactly 1 at t = warmup"
            ramp = [F(kind, t, warmup, warmup + 5, 0.1) for t in range(1, warmup + 1)]
            assert ramp == [t / warmup for t in range(1, warmup + 1)] and F(kind, 0, warmup, warmup + 5, 0.1) == ramp[0], "t < 1 counts as 1"
    for kind in ("linear", "cosine"):
        for warmup, total in ((0, 1), (0, 8), (3, 4), (3, 8), (2, 33)):
            for final in (0.0, 0.1, 0.5, 1.0):
                fin = lr_ref.f32(final)
                for t in range(total, total + 4):
                    assert F(kind, t, warmup, total, final) == fin, "exactly final from total on"
                    assert lr_ref.exact(kind, t, warmup, total)
                tail = [F(kind, t, warmup, total, final) for t in range(max(warmup, 1), total + 3)]
                assert all(a >= b for a, b in zip(tail, tail[1:])), f"non-increasing after the warm-up: {kind} {warmup} {total} {final}"
                assert all(fin <= f <= 1.0 for f in tail)
    # linear and cosine meet at s = 0, 1/2 and 1
    for warmup, total in ((0, 8), (3, 11), (4, 6)):
        for final in (0.0, 0.1, 1.0):
            mid = (warmup + total) // 2
            for t, want in ((max(warmup, 1), None), (mid, 0.5 * (1.0 + lr_ref.f32(final))), (total, lr_ref.f32(final))):
                if warmup == 0 and want is None:
                    continue  # s = 0 is t = 0: before the first step
                lin, cos = F("linear", t, warmup, total, final), F("cosine", t, warmup, total, final)
                assert abs(lin - cos) <= 4 * 2.0 ** -53 and (want is None or abs(lin - want) <= 4 * 2.0 ** -53), (warmup, total, final, t)
            if warmup:
                assert F("linear", warmup, warmup, total, final) == F("cosine", warmup, warmup, total, final) == 1.0
    assert lr_ref.lr_now(5e-4, "constant", 9, 0, 0, 0.0, 1.0) == lr_ref.f32(5e-4)
    assert math.isclose(lr_ref.lr_now(5e-4, "cosine", 5, 0, 10, 0.0, 0.5), lr_ref.f32(5e-4) * 0.25, rel_tol=1e-15)
