"""The step's telemetry without a GPU: the option parser and the engine's two refusals before the device check, the three exports and
their host-side return codes, the chunk-table builder on real slot tables, and the ADMISSIBILITY of the bound the GPU test holds
vg_grad_stats to (tests/telemetry_ref.py derives it from the reduction tree): the fp32 emulation of the tree stays inside it on the GPU
test's inputs, and every planted defect lands outside.  The admissibility tests walk the chunk table the PRODUCT builds
(``ops.grad_chunks``) and the field table of the binding (``_lib.TEL_FIELDS``), so every test here fails on the parent commit: the
option, the exports, the builder and the tables are this feature's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import telemetry_ref as tr
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib, flat, ops
from vit_gan_amd.config import Config

NEW = ("vg_grad_stats", "vg_logit_stats", "vg_telemetry_commit")


def _nets():
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=1, dropout_rate=0.0, batch_size=4, transformer_blocks_count=1))
    return D, SirenGenerator(layers=1, dropout=0.0)


def test_exports_exist_with_abi_9():
    lib = _lib.lib()
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitgan_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib._SIGNATURES and f"int {name}(" in header, name
    assert "typedef struct VgTelemetrySrc" in header
    for i, name in enumerate(tr.TEL_FIELDS):  # the field indices are fixed in the header, and the binding and the restatement agree
        assert f"#define VG_TEL_{name.upper()} {i}\n" in header or f"#define VG_TEL_{name.upper()} {i} " in header, name
    assert f"#define VG_TEL_NF {tr.TEL_NF} " in header and _lib.TEL_NF == tr.TEL_NF and _lib.TEL_FIELDS == tr.TEL_FIELDS
    assert len(tr.TEL_FIELDS) < tr.TEL_NF and tr.TEL_NF % 4 == 0
    assert C.sizeof(_lib.VgTelemetrySrc) == 11 * 8 + 3 * 4 + 4  # eleven pointers, three ints, padded to the pointers' alignment


def test_parse_telemetry():
    assert ops.parse_telemetry(0) == 0 and ops.parse_telemetry(1) == 1 and ops.parse_telemetry(4096) == 4096
    for bad in (True, False, -1, 1.0, 2.5, "4", None, (4,), 2 ** 24):
        with pytest.raises(ValueError, match="telemetry"):
            ops.parse_telemetry(bad)


def test_engine_refuses_without_a_device(monkeypatch):
    from vit_gan_amd import engine
    D, G = _nets()
    for bad in (True, -2, 1.5, "on"):
        with pytest.raises(ValueError, match="telemetry"):
            engine.GanEngine(D, G, batch=4, telemetry=bad)
    with pytest.raises(ValueError, match="telemetry.*two_stream"):
        engine.GanEngine(D, G, batch=4, telemetry=4, two_stream=True)
    monkeypatch.setattr(engine, "world_size", lambda pg: 2)
    with pytest.raises(ValueError, match="telemetry.*more than one rank"):
        engine.GanEngine(D, G, batch=4, telemetry=4)
    monkeypatch.undo()
    # what is allowed gets as far as the device check: no argument error
    for kw in (dict(), dict(exchange_single_rank=True), dict(fuse_real_fake=False), dict(diffaug="color", ada_target=0.6),
               dict(r1_gamma=1.0, r1_interval=2), dict(lr_schedule="cosine", lr_total=10), dict(clip_d=5.0, clip_g=0.5)):
        with pytest.raises(RuntimeError, match="cuda"):
            engine.GanEngine(D, G, batch=4, telemetry=4, **kw)
    with pytest.raises(RuntimeError, match="cuda"):  # off is off
        engine.GanEngine(D, G, batch=4, telemetry=0, two_stream=True)


def test_return_codes_come_back_before_any_launch():
    lib, p = _lib.lib(), C.c_void_p(4096)  # (a non-null, 16-byte aligned dummy: never dereferenced on these paths; no device here)
    odd8, odd4 = C.c_void_p(4096 + 8), C.c_void_p(4096 + 4)
    gs = lambda g=p, n=64, ch=p, nc=4, sf=p, ns=2, sc=1.0, scr=p, nrm=p, tot=p: lib.vg_grad_stats(g, n, ch, nc, sf, ns, sc, scr, nrm, tot, None)  # noqa: E731
    for hole in ("g", "ch", "sf", "scr", "nrm", "tot"):
        assert gs(**{hole: None}) == -1, hole
    for kw in (dict(n=0), dict(n=1 << 31), dict(nc=0), dict(ns=0), dict(ns=5), dict(ns=2049, nc=4096), dict(sc=0.0), dict(sc=-1.0),
               dict(sc=float("nan")), dict(sc=float("inf"))):
        assert gs(**kw) == -2, kw
    assert gs(g=odd8) == -3 and gs(g=odd4) == -3 and gs(tot=odd8) == -3 and gs(scr=odd4) == -3
    ls = lambda x0=p, x1=None, n=8, role=0, out=p: lib.vg_logit_stats(x0, x1, n, role, out, None)  # noqa: E731
    assert ls(x0=None) == -1 and ls(out=None) == -1
    for kw in (dict(n=0), dict(n=16385), dict(role=-1), dict(role=3), dict(x1=p, role=2)):
        assert ls(**kw) == -2, kw
    assert ls(out=odd8) == -3

    def commit(src_kw=None, step=p, cap=4, rs=p, ring=p, rd=p, rg=p):
        kw = dict(losses=4096, seg_d=4096, seg_g=4096, n_seg_d=3, n_seg_g=3, penalty_due=0)
        kw.update(src_kw or {})
        return lib.vg_telemetry_commit(C.byref(_lib.VgTelemetrySrc(**kw)), step, cap, rs, ring, rd, rg, None)
    assert lib.vg_telemetry_commit(None, p, 4, p, p, p, p, None) == -1
    assert commit(step=None) == -1 and commit(rs=None) == -1 and commit(ring=None) == -1
    assert commit(rd=None) == -1 and commit(rg=None) == -1, "a source without its ring"
    assert commit(dict(seg_d=None, n_seg_d=0), rd=None, cap=0) == -2, "a missing source needs no ring: the null check passes"
    for kw, cap in ((dict(), 0), (dict(), -1), (dict(n_seg_d=-1), 4), (dict(penalty_due=2), 4)):
        assert commit(kw, cap=cap) == -2, (kw, cap)
    assert commit(dict(n_seg_g=0)) == -3


@pytest.mark.parametrize("geometry", ["small", "c2", "conditional"])
def test_chunk_table_covers_every_slot_element_once_and_no_padding(geometry):
    if geometry == "small":
        tables = [flat.vit_slots(_lib.VgVitDims(3, 32, 4, 128, 4, 1, 2, 1))]
        from vit_gan_amd.generator import SirenGenerator
        tables.append(SirenGenerator(layers=1)._flat.slots)
    elif geometry == "c2":
        from vit_gan_amd.generator import SirenGenerator
        tables = [flat.vit_slots(_lib.VgVitDims(3, 32, 4, 384, 4, 6, 2, 1)), flat.gen_slots(SirenGenerator()._dims)]
    else:
        from vit_gan_amd.generator import SirenGenerator
        G = SirenGenerator(layers=1, n_classes=3)
        assert flat.CLASS_TABLE_KEY in G._flat.slots
        tables = [G._flat.slots]
    for slots in tables:
        chunks, seg_first, keys = ops.grad_chunks(slots)
        assert chunks.dtype == np.int32 and seg_first.dtype == np.int32 and chunks.shape[1] == 3 and keys == list(slots)
        want, want_first = tr.chunk_table(slots)  # the restatement's own builder
        assert np.array_equal(chunks, want) and np.array_equal(seg_first, want_first)
        total = max(off + tr.numel(shape) for off, shape in slots.values())
        cover = np.zeros(total, dtype=np.int32)
        for first, count, seg in chunks:
            assert 1 <= count <= 4096
            cover[first:first + count] += 1
        inside = np.zeros(total, dtype=np.int32)
        for off, shape in slots.values():
            inside[off:off + tr.numel(shape)] += 1
        assert inside.max() == 1 and np.array_equal(cover, inside), "every slot element exactly once, no padding element"
        for s, (off, shape) in enumerate(slots.values()):  # a segment's chunks: adjacent, ascending, inside the slot
            cs = chunks[seg_first[s]:seg_first[s + 1]]
            assert len(cs) >= 1 and (cs[:, 2] == s).all() and cs[0, 0] == off and cs[-1, 0] + cs[-1, 1] == off + tr.numel(shape)
            assert (cs[1:, 0] == cs[:-1, 0] + cs[:-1, 1]).all()
    if geometry == "small":  # the SLN scalars are one element long and not 16-byte aligned: the case the kernel's peeling exists for
        g_slots = tables[1]
        b, g_ = g_slots["sln.beta"], g_slots["sln.gamma"]
        assert tr.numel(b[1]) == tr.numel(g_[1]) == 1 and b[0] == g_[0] + 1
    with pytest.raises(ValueError, match="limit"):
        ops.grad_chunks(tables[0], limit=4097)


@pytest.fixture(scope="module")
def case():
    g, slots = tr.grad_case()
    n = np.asarray([tr.numel(shape) for _, shape in slots.values()], dtype=np.float64)
    return g, slots, n, ops.grad_chunks(slots)[:2]  # the table the kernel is given: the product's builder, not the restatement's


def test_the_case_exercises_what_the_kernel_can_get_wrong(case):
    g, slots, n, table = case
    assert np.array_equal(table[0], tr.chunk_table(slots)[0]) and (table[0][:, 1] <= ops.GRAD_CHUNK).all() and ops.GRAD_CHUNK == tr.CHUNK
    offs = [off % 4 for off, _ in slots.values()]
    assert set(offs) == {0, 1, 2, 3} and sorted(set(int(v) for v in n)) == [1, 3, 4, 5, 7, 64, 4095, 4096, 4097, 1000003]
    inside = np.zeros(g.size, dtype=bool)
    for off, shape in slots.values():
        inside[off:off + tr.numel(shape)] = True
    assert np.isnan(g[~inside]).all() and (~inside).sum() >= 8 and np.isfinite(g[inside]).all()
    for off, shape in slots.values():  # the first and the last element carry a visible share: far above the bound
        m = tr.numel(shape)
        seg = g[off:off + m].astype(np.float64)
        assert seg[0] ** 2 / np.sum(seg * seg) > 1e3 * tr.KAPPA * tr.U and seg[-1] ** 2 / np.sum(seg * seg) > 1e3 * tr.KAPPA * tr.U


@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_the_emulated_tree_is_inside_the_bound(case, gscale):
    g, slots, n, table = case
    ref, got = tr.grad_stats_ref(g, slots, gscale), tr.grad_stats_emul(g, slots, gscale, table=table)
    bound = tr.norm_bound(ref["norms"], n, gscale)
    err = np.abs(got["norms"].astype(np.float64) - ref["norms"])
    assert (err <= bound).all(), (err / bound).max()
    assert abs(float(got["l2"]) - ref["l2"]) <= tr.norm_bound(ref["l2"], n.sum(), gscale)
    assert abs(float(got["sum_norms"]) - ref["sum_norms"]) <= bound.sum() + tr.U * ref["sum_norms"]
    assert got["nonfinite"] == ref["nonfinite"] == 0
    # the bound is tight enough to mean something: nowhere near a percent, and the tree really uses a part of it
    assert tr.KAPPA * tr.U < 1e-6 and err.max() > 0.0


@pytest.mark.parametrize("defect", tr.DEFECTS)
def test_every_planted_defect_lands_outside_the_bound(case, defect):
    g, slots, n, table = case
    gscale = 0.125
    ref = tr.grad_stats_ref(g, slots, gscale)
    got = tr.grad_stats_emul(g, slots, gscale, defect=defect, table=table)
    bound = tr.norm_bound(ref["norms"], n, gscale)
    err = np.abs(got["norms"].astype(np.float64) - ref["norms"])
    outside = ~(err <= bound)  # (a NaN - padding read by mistake - is outside)
    assert outside.any(), defect
    if defect == "drop_last_partial_chunk":  # exactly the segments that end in a partial chunk behind a full one
        assert list(np.flatnonzero(outside)) == [i for i, m in enumerate(n) if m > 4096 and m % 4096]
    if defect == "head_as_if_aligned":  # exactly the segments whose first element is not 16-byte aligned
        assert list(np.flatnonzero(outside)) == [i for i, (off, _) in enumerate(slots.values()) if off % 4]
    if defect in ("neighbour_element", "no_gscale"):
        assert outside.all()
    tot = abs(float(got["l2"]) - ref["l2"])
    assert not tot <= tr.norm_bound(ref["l2"], n.sum(), gscale), "the total sees it too"


def test_logit_tree_and_counts():
    rng = np.random.default_rng(3)
    for m in (1, 7, 256, 3 * 256, 16384):
        x = rng.standard_normal(m).astype(np.float32)
        x[::5] = 0.0
        x[1::7] = -0.0
        mean, fp, fn = tr.logit_stats_emul(x)
        ref_mean, pos, neg = tr.logit_stats_ref(x)
        assert abs(float(mean) - ref_mean) <= tr.KAPPA_MEAN * tr.U * float(np.mean(np.abs(x.astype(np.float64)))) + 1e-45
        assert fp == np.float32(pos) / np.float32(m) and fn == np.float32(neg) / np.float32(m)
        assert pos + neg + int(np.count_nonzero(x == 0)) == m
    assert tr.logit_stats_ref(np.asarray([0.0, -0.0, np.nan, 1.0, -2.0]))[1:] == (1, 1)
    # the operators themselves have no CPU path: a host tensor is refused, not computed some other way
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_stats(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_stats(torch.zeros(8), {"w": (0, (8,))})


def test_commit_restatement_is_idempotent_and_keyed_on_the_counter():
    cap = 4
    steps, ring = np.zeros(cap, dtype=np.int32), np.full((cap, tr.TEL_NF), np.nan, dtype=np.float32)
    F = _lib.TEL_FIELDS  # the binding's table: what GanEngine.history() names the columns by
    assert ring.shape[1] == _lib.TEL_NF
    tr.commit_ref(steps, ring, 0, cap, {"loss_g": 1.0}, order=F)
    assert not steps.any() and np.isnan(ring).all(), "no step has run: nothing is written"
    for t in (1, 1, 2, 3, 4, 5, 6):  # step 1 twice: the warm-up of a captured step and its first replay
        tr.commit_ref(steps, ring, t, cap, {"loss_g": float(t), "penalty": float("nan") if t % 2 == 0 else 0.5}, order=F)
    assert list(steps) == [5, 6, 3, 4] and list(ring[:, F.index("loss_g")]) == [5.0, 6.0, 3.0, 4.0]
    pen = ring[:, F.index("penalty")]
    assert np.isnan(pen[[1, 3]]).all() and (pen[[0, 2]] == 0.5).all() and np.isnan(ring[:, F.index("ada_p")]).all()
