"""Adaptive discriminator augmentation without a GPU: the three entry points are exported and declared, the gates of the restatement
(tests/ada_ref.py) are what the header says - nested in p, the existing draws at p = 1, nothing at p = 0, the claimed frequencies,
independent of each other and of the parameter draws - the fp32 controller follows the float64 textbook heuristic and four planted
mistakes do not, and the Python surface and the C entry points refuse what they do not take before any device is touched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ada_ref as ar
import diffaug_ref as dr
import engine_util as eu
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_diffaug_p_fwd", "vg_diffaug_p_bwd", "vg_ada_update")


# -------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "vitgan_hip.h")).read()
    for n in NEW:
        assert n in _lib._SIGNATURES and hasattr(lib, n), n
        assert f"int {n}(" in header, n
    assert lib.vg_abi_version() == 9 and _lib.ABI_VERSION == 9  # additive: the ABI number stays


def test_gated_entry_points_validate_before_any_launch():
    lib = _lib.lib()
    p = C.c_void_p(4096)  # never dereferenced: validation fails first
    fwd = lambda x=p, y=p, B=4, Cc=3, IH=32, pol=7, pr=p: lib.vg_diffaug_p_fwd(x, y, None, B, Cc, IH, pol, 1, 0, None, pr, None)  # noqa: E731
    bwd = lambda x=p, y=p, B=4, Cc=3, IH=32, pol=7, pr=p: lib.vg_diffaug_p_bwd(x, y, 0, B, Cc, IH, pol, 1, 0, None, pr, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(x=None) == -1 and f(y=None) == -1 and f(B=0) == -1 and f(pr=None) == -1
        assert f(pol=-1) == -2 and f(pol=8) == -2 and f(Cc=0) == -2 and f(IH=7) == -2 and f(IH=256) == -2
        assert f(Cc=3, IH=9) == -3 and f(Cc=1, IH=10) == -3


def test_controller_entry_point_validates_before_any_launch():
    lib = _lib.lib()
    p = C.c_void_p(4096)
    f = lambda lg=p, n=8, st=p, tgt=0.6, spi=1e-5, iv=4, step=p: lib.vg_ada_update(lg, n, st, tgt, spi, iv, step, None)  # noqa: E731
    assert f(lg=None) == -1 and f(st=None) == -1 and f(step=None) == -1 and f(n=0) == -1 and f(n=-5) == -1
    assert f(iv=0) == -2 and f(iv=-1) == -2
    assert f(tgt=1.0) == -2 and f(tgt=-1.0) == -2 and f(tgt=float("nan")) == -2 and f(tgt=2.0) == -2
    assert f(spi=0.0) == -2 and f(spi=-1e-5) == -2 and f(spi=float("inf")) == -2 and f(spi=float("nan")) == -2
    assert f(n=1 << 24) == -2
    assert f(st=C.c_void_p(4100)) == -3  # the state is one 16-byte vector


# ------------------------------------------------------------------------------------------------------------- the gates
SEED, SITE, STEPS, IMAGES, IH_STAT = 20240607, 0, 256, 256, 32  # 65 536 (step, image) pairs: test_diffaug_cpu.py's


def test_threshold():
    assert ar.threshold(1.0) == 1 << 24 and ar.threshold(0.0) == 0 and ar.threshold(0.5) == 1 << 23
    assert ar.threshold(7.0) == 1 << 24 and ar.threshold(-0.25) == 0 and ar.threshold(float("nan")) == 0
    assert ar.threshold(float("inf")) == 1 << 24 and ar.threshold(float("-inf")) == 0
    assert ar.threshold(np.float32(0.9)) == int(math.floor(float(np.float32(0.9)) * 2 ** 24))
    assert ar.threshold(2.0 ** -25) == 0 and ar.threshold(2.0 ** -24) == 1


@pytest.mark.parametrize("policy", range(8))
def test_p_one_is_the_existing_draw_and_p_zero_is_nothing(policy):
    for step in (1, 2, 70000, None):
        for B, IH in ((7, 32), (256, 36)):
            assert np.array_equal(ar.draw_p(SEED, 1, step, B, IH, policy, 1.0), dr.draw(SEED, 1, step, B, IH, policy))
            assert (ar.gates(SEED, 1, step, B, policy, 1.0) == policy).all()
            assert (ar.gates(SEED, 1, step, B, policy, 0.0) == 0).all()
            assert np.array_equal(ar.draw_p(SEED, 1, step, B, IH, policy, 0.0), dr.draw(SEED, 1, step, B, IH, 0))
            assert (ar.gates(SEED, 1, step, B, policy, float("nan")) == 0).all()


def test_the_gated_set_grows_with_p():
    ps = [0.0, 1e-3, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999, 1.0]
    sets = [ar.gates(SEED, 0, 3, 4096, 7, p) for p in ps]
    for lo, hi in zip(sets, sets[1:]):
        assert ((lo & ~hi) == 0).all()  # every member on at p is on at p' > p
    assert int((sets[4] != 0).sum()) > 0 and int((sets[4] != 7).sum()) > 0
    for q in range(8):  # only members of the policy are ever on
        assert ((ar.gates(SEED, 0, 3, 4096, q, 0.5) & ~q) == 0).all()
    # the rows of what is on are the existing draws, the rows of what is off the identities
    rows, eff = ar.draw_p(SEED, 0, 3, 64, 32, 7, 0.5), ar.gates(SEED, 0, 3, 64, 7, 0.5)
    full = dr.draw(SEED, 0, 3, 64, 32, 7)
    assert np.array_equal(rows[:, 7], eff.astype(np.float32))
    for m, cols, ident in ((0, [0, 1, 2], [0, 1, 1]), (1, [3, 4], [0, 0]), (2, [5, 6], [-32, -32])):
        on = (eff >> m) & 1 == 1
        assert on.any() and (~on).any()
        assert np.array_equal(rows[on][:, cols], full[on][:, cols]) and (rows[~on][:, cols] == np.array(ident, dtype=np.float32)).all()


def _stream(i, seed=SEED, site=SITE):
    return dr.k24(seed, site, np.arange(1, STEPS + 1)[:, None], np.arange(IMAGES)[None, :], i)  # [step, image]


def _corr(a, b):
    return float(np.corrcoef(a.ravel().astype(np.float64), b.ravel().astype(np.float64))[0, 1])


@pytest.mark.parametrize("p", [0.25, 0.5, 0.9])
def test_gate_frequencies_and_independence(p):
    """each member's frequency within 5 standard errors of p; the three gates uncorrelated with each other and with the seven parameter
    draws within 5 / sqrt(n) - test_diffaug_cpu.py's bounds"""
    T = np.uint64(ar.threshold(p))
    on = [ar.gate_draws(SEED, SITE, np.arange(1, STEPS + 1)[:, None], np.arange(IMAGES)[None, :], m) < T for m in range(3)]
    n = on[0].size
    assert n == 65536
    pq = ar.threshold(p) / 2.0 ** 24
    for m in range(3):
        assert abs(on[m].mean() - pq) <= 5 * math.sqrt(pq * (1 - pq) / n), (m, on[m].mean())
        # and what gates() reports is these compares
        eff = np.stack([ar.gates(SEED, SITE, s, IMAGES, 7, p) for s in (1, STEPS)])
        assert np.array_equal((eff >> m) & 1, on[m][[0, STEPS - 1]].astype(np.int64))
    lim = 5 / math.sqrt(n)
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(_corr(on[a], on[b])) <= lim, (a, b)
        for i in range(7):
            assert abs(_corr(on[a], _stream(i))) <= lim, (a, i)


# -------------------------------------------------------------------------------------------------------- the controller
def _batches(rs, n, rng):
    """per step n logits of which a fraction (1 + r) / 2 is positive: r_t of the step is r (n (1 + r) / 2 must be an integer)"""
    out = []
    for r in rs:
        pos = n * (1 + r) / 2
        assert pos == int(pos)
        lg = np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(0.1)
        lg[int(pos):] *= -1
        out.append(rng.permutation(lg))
    return out


def _run(batches, p0, target, spi, interval, mistake=None, first_step=1):
    st = np.array([p0, 0, 0, 0], dtype=np.float32)
    ps, rs = [], []
    for i, lg in enumerate(batches):
        st = ar.controller(st, lg, target, spi, interval, first_step + i, mistake=mistake)
        ps.append(float(st[0]))
        rs.append(float(st[3]))
    return np.array(ps), np.array(rs), st


N_IMG, INTERVAL = 16, 4
SPI = np.float32(1.0 / (1000.0 * 0.4))  # 64 images move p by 0.16: both clamps are reached within a few updates
SEQUENCES = {
    # name: (p0, target, r_t of every step)
    "rises":           (0.0, 0.5, [1.0] * 12),
    "falls":           (0.9, 0.5, [-1.0] * 12),
    "clamps_at_one":   (0.8, 0.25, [0.75] * 16),
    "clamps_at_zero":  (0.2, 0.25, [-0.5] * 16),
    "sits_on_target":  (0.4, 0.5, [0.5] * 12),                     # 12 of 16 positive: acc_sign = target acc_count exactly
    "rises_then_falls": (0.3, 0.5, [1.0] * 8 + [0.0] * 12 + [0.75, 0.25, 0.75, 0.25] * 2),  # the last two windows sit on target
    "odd_target":      (0.5, 0.6, [0.75, 0.5, 0.75, 0.5] * 3 + [0.5, 0.5, 0.75, 0.5] * 3),  # windows at 0.625 and 0.5625 around 0.6
}


def _check(name, mistake=None):
    p0, target, rs = SEQUENCES[name]
    batches = _batches(rs, N_IMG, np.random.default_rng(len(name)))
    got_p, got_r, st = _run(batches, p0, target, SPI, INTERVAL, mistake)
    want_p, want_r = ar.simulate64(float(np.float32(p0)), batches, float(np.float32(target)), float(SPI), INTERVAL)  # the state is fp32
    updates = np.arange(1, len(rs) + 1) // INTERVAL
    assert (np.abs(got_p - want_p) <= ar.trajectory_bound(updates) + 0.0).all(), (name, mistake, got_p, want_p)
    seen = ~np.isnan(want_r)
    assert (np.abs(got_r[seen] - want_r[seen]) <= 2.0 ** -23).all(), (name, mistake, got_r, want_r)
    return got_p, st


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_controller_follows_the_textbook_heuristic(name):
    got_p, st = _check(name)
    p0 = SEQUENCES[name][0]
    assert st[1] == 0 and st[2] == 0  # the last step of every sequence is an update: both accumulators are cleared
    if name == "rises":
        assert (np.diff(got_p) >= 0).all() and got_p[-1] > p0
    if name == "falls":
        assert (np.diff(got_p) <= 0).all() and got_p[-1] < p0
    if name == "clamps_at_one":
        assert got_p[-1] == 1.0 and got_p[-5] == 1.0
    if name == "clamps_at_zero":
        assert got_p[-1] == 0.0 and got_p[-5] == 0.0
    if name == "sits_on_target":
        assert (got_p == np.float32(p0)).all()
    # between two updates p does not move
    assert all(got_p[i] == got_p[i - 1] for i in range(1, len(got_p)) if (i + 1) % INTERVAL)


def test_controller_accumulates_between_updates():
    st = np.array([0.5, 0, 0, -7.0], dtype=np.float32)
    lg = np.array([1.5, -2.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 3.0], dtype=np.float32)  # signs +, -, 0, 0, 0, +, -, +: sum 1
    st = ar.controller(st, lg, 0.5, 0.01, 4, 1)
    assert st.tolist() == [0.5, 1.0, 8.0, -7.0]
    st = ar.controller(st, lg[:3], 0.5, 0.01, 4, 2)
    assert st.tolist() == [0.5, 1.0, 11.0, -7.0]
    st = ar.controller(st, lg[:1], 0.5, 0.01, 4, 4)  # fires: 2 of 12 against a target of 0.5 -> p falls by 12 * 0.01
    assert st[1] == 0 and st[2] == 0 and st[3] == np.float32(2.0) / np.float32(12.0)
    assert st[0] == np.float32(np.float32(0.5) - np.float32(np.float32(0.01) * np.float32(12)))


@pytest.mark.parametrize("mistake", ["every_step", "no_reset", "sign_flipped", "no_clamp"])
def test_planted_mistakes_are_caught(mistake):
    caught = []
    for name in SEQUENCES:
        _check(name)  # the controller as the header states it passes
        try:
            _check(name, mistake)
        except AssertionError:
            caught.append(name)
    assert caught, mistake
    want = {"every_step": "rises", "no_reset": "rises_then_falls", "sign_flipped": "falls", "no_clamp": "clamps_at_one"}[mistake]
    assert want in caught, (mistake, caught)


# --------------------------------------------------------------------------------------------------- the Python surface
def _nets():
    from vit_gan_amd.config import Config
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    return ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1)), SirenGenerator(layers=1)


def test_engine_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.engine import GanEngine
    D, G = _nets()
    mk = lambda **kw: GanEngine(D, G, batch=4, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="diffaug"):
        mk(aug_p=0.5)
    with pytest.raises(ValueError, match="diffaug"):
        mk(ada_target=0.6)
    with pytest.raises(ValueError, match="diffaug"):
        mk(aug_p=0.5, bcr=(1.0, 1.0), bcr_aug="color")  # the bcr_aug site is not gated
    for bad in (-0.1, 1.5, float("nan"), "half"):
        with pytest.raises(ValueError, match="aug_p"):
            mk(diffaug="color", aug_p=bad)
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="ada_target"):
            mk(diffaug="color", ada_target=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="ada_interval"):
            mk(diffaug="color", ada_target=0.6, ada_interval=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ada_kimg"):
            mk(diffaug="color", ada_target=0.6, ada_kimg=bad)
    with pytest.raises(ValueError, match="[Ww]asserstein"):
        mk(diffaug="color", ada_target=0.6, loss="wasserstein")
    # good arguments get as far as the device check - a fixed probability with the critic's loss among them
    for kw in (dict(aug_p=0.5), dict(ada_target=0.6), dict(aug_p=0.25, ada_target=0.6, ada_interval=1, ada_kimg=0.064),
               dict(aug_p=1.0, loss="wasserstein"), dict(aug_p=0.0, bcr=(10.0, 10.0))):
        with pytest.raises(RuntimeError, match="cuda|MI355X"):
            mk(diffaug="color,cutout", **kw)


def test_trainer_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.training import train_model
    tm = lambda **kw: train_model(save_artifacts=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="diffaug"):
        tm(aug_p=0.5)
    with pytest.raises(ValueError, match="diffaug"):
        tm(ada_target=0.6)
    with pytest.raises(ValueError, match="aug_p"):
        tm(diffaug="color", aug_p=1.5)
    with pytest.raises(ValueError, match="ada_target"):
        tm(diffaug="color", ada_target=1.0)
    with pytest.raises(ValueError, match="ada_interval"):
        tm(diffaug="color", ada_target=0.6, ada_interval=0)
    with pytest.raises(ValueError, match="ada_kimg"):
        tm(diffaug="color", ada_target=0.6, ada_kimg=0.0)
    with pytest.raises(ValueError, match="[Ww]asserstein"):
        tm(diffaug="color", ada_target=0.6, loss="wasserstein")


def _group_worker(rank, world):
    import torch.distributed as dist
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.engine import GanEngine
    D, G = _nets()
    res = []
    for kw in (dict(ada_target=0.6, exchange_single_rank=True), dict(aug_p=0.5, exchange_single_rank=True)):
        try:
            GanEngine(D, G, batch=4, diffaug="color", process_group=dist.group.WORLD, **kw)
            res.append("built")
        except Exception as e:
            res.append(f"{type(e).__name__}: {e}")
    return res


def test_engine_refuses_ada_with_an_active_process_group():
    """the controller's statistics are per process: refused where the exchange is active (a one-rank group that runs the exchange
    stands in for more ranks); a fixed aug_p gets as far as the device check"""
    (res,) = eu.run_ranks(_group_worker, 1, 120)
    assert res[0].startswith("ValueError") and "data parallelism" in res[0], res
    assert res[1].startswith("RuntimeError") and ("cuda" in res[1] or "MI355X" in res[1]), res


def test_diff_augment_with_p_has_no_cpu_fallback_and_checks_p():
    import torch
    from vit_gan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.diff_augment(torch.zeros(2, 3, 32, 32), "color", 0, 0, p=0.5)
    with pytest.raises(ValueError, match="aug_p"):
        ops.diff_augment(torch.zeros(2, 3, 32, 32), "color", 0, 0, p=1.5)
    with pytest.raises(ValueError, match="ONE fp32 element"):
        ops.diff_augment(torch.zeros(2, 3, 32, 32), "color", 0, 0, p=torch.zeros(2))
