"""The kernels at the two ends of the networks (csrc/elementwise.hip), each through its own C entry point, against the float64
restatements and the derived bounds of tests/ends_ref.py.

The classifier head forward and backward on both of its paths - the one-launch kernel (Kc <= 16, partial rows) and the separate
vg_head_bwd_dz_kernel + vg_head_bwd_w2_kernel (Kc > 16, and forced at Kc <= 16 by part = NULL) - at batch sizes across the 8-row
wave, the 32-row part and the 64-lane batch stride; the batch sum across its 32 batch lanes and its four-deep main loop; the
embedding's small gradients; the row movers, vg_fill_cls and their dropout masks; patchify and its inverse; the slab folds; the
position table; the SIREN gradient.  Every output lives in a buffer with sentinel rows behind it and must be written in full and
nowhere else; accumulated outputs start from non-zero contents.  Exact probes (integers and halves) must come back bit for bit,
random probes within gamma(n) sum|terms| (ends_ref), whose inputs make a dropped or doubled term fail by construction.  Nothing here
is tuned to what the GPU returns.  Each test prints the worst err / limit per output as a record (profiles/ends_kernels.txt).

The hardware cosine behind vg_sin_grad (__cosf) was measured once on an MI355X against float64 over this test's own arguments
(ends_ref.sin_inputs at n = 4, 1020, 4100: |w0 z| <= 120, the multiples of pi / 2 among them): its largest absolute error was
EPS_COS_MEASURED below (profiles/ends_kernels.txt).  The limit uses twice that, which ends_ref.sin_grad refuses above 2^-10."""
import ctypes as C

import pytest
import torch

import ends_ref as R
import exact_util as X
from exact_util import BF

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SEED, P_DROP = 0x5EED5, 0.1
EPS_COS_MEASURED = 1.06e-5  # max |__cosf(a) - cos(a)| over the 5124 arguments a = fl32(w0 z) of this test (1.0576e-05, reached at |a| = 117.9)


def _u():
    return X.gpu()


def _lib():
    from vit_gan_amd import _lib
    return _lib.lib()


def _vec(n, dtype=F32, guard=1):
    return X.guarded(1, n, dtype, "cuda", guard=guard)


def _whole(buf, rows, what):
    X.assert_guard(buf, rows, what)
    X.assert_written(buf, rows, what)


def _show(what, stats):
    print(what, {k: round(v, 3) for k, v in sorted(stats.items())}, "(worst err / limit)")


def _filled(values64, dtype, guard=2):
    """a guarded buffer whose in-range rows hold `values64` [rows, cols]: the non-zero start of an accumulated output"""
    rows, cols = values64.shape
    buf = X.guarded(rows, cols, dtype, "cuda", guard=guard)
    buf[:rows] = _u().dev(values64, dtype)
    return buf


# ------------------------------------------------------------------------------------------------------------ classifier head
HEAD_E, HEAD_KC, HEAD_B = [128, 384], [1, 2, 10, 16, 17, 40], [1, 7, 8, 9, 31, 32, 33, 65, 130]


def _head_fwd_run(inp, B, E, Kc):
    g = _u()
    t, W2, b2 = g.dev(inp["t"], BF), g.dev(inp["W2"], F32), g.dev(inp["b2"], F32)
    out = X.guarded(B, Kc, F32, "cuda", guard=8)
    g.call("vg_head_fwd", g.ptr(t), g.ptr(W2), g.ptr(b2), g.ptr(out), B, E, Kc, g.stream())
    g.sync()
    _whole(out, B, f"B {B} logits")
    return out[:B].cpu()


def _head_bwd_run(inp, B, E, Kc, path, want_wgrad=1):
    """path 'one': part given (Kc <= 16: the one-launch kernel, then the fold of its partial rows with vg_colsum_f32);
    path 'split': part = NULL (the separate kernels; db1 is vg_colsum_bf16 of dz).  The accumulated outputs start from inp's *_0."""
    g, lib = _u(), _lib()
    what = f"B {B} {path}{'' if want_wgrad else ' dz only'}"
    t, W2, dlog = g.dev(inp["t"], BF), g.dev(inp["W2"], F32), g.dev(inp["dlog"], F32)
    dz = X.guarded(B, E, BF, "cuda", guard=8)
    dW2, db2, db1 = _filled(inp["dW2_0"], F32), _filled(inp["db2_0"][None], F32, 1), _filled(inp["db1_0"][None], F32, 1)
    parts, width = lib.vg_head_bwd_parts(B), lib.vg_head_bwd_part_width(E, Kc)
    assert (parts, width) == (R.head_parts(B), R.head_part_width(E, Kc))
    part = X.guarded(parts, width, F32, "cuda", guard=2) if path == "one" else None
    rc = lib.vg_head_bwd(g.ptr(dlog), g.ptr(W2), g.ptr(t), g.ptr(dz), g.ptr(dW2), g.ptr(db2), g.ptr(part), B, E, Kc, want_wgrad, g.stream())
    one = path == "one" and want_wgrad
    assert rc == (1 if one else 0), f"{what}: vg_head_bwd returned {rc}"
    g.sync()
    _whole(dz, B, f"{what} dz")   # rows >= B stay untouched
    out = {"dz": dz[:B].cpu()}
    if not want_wgrad or one:     # nothing may have touched dW2 / db2 (and, dz only, the partial rows)
        X.assert_bitwise(dW2[:Kc].cpu(), X.rne(inp["dW2_0"], F32), f"{what}: dW2 must stay as it was")
        X.assert_bitwise(db2[0].cpu(), X.rne(inp["db2_0"], F32), f"{what}: db2 must stay as it was")
        if part is not None and not want_wgrad:
            X.assert_guard(part, 0, f"{what}: partial rows written by a dz-only call")
    if not want_wgrad:
        return out
    if one:
        _whole(part, parts, f"{what} part")   # every partial row in full, none beyond vg_head_bwd_parts(B)
        out["part"] = part[:parts].cpu()
        g.call("vg_colsum_f32", g.ptr(part), parts, width, g.ptr(dW2), Kc * E, g.ptr(db1), E, g.ptr(db2), Kc, None, 0, 1, g.stream())
    else:
        ws = torch.empty(lib.vg_colsum_bf16_parts(B) * E, dtype=F32, device="cuda")
        g.call("vg_colsum_bf16", g.ptr(dz), E, B, E, g.ptr(ws), g.ptr(db1), 1, g.stream())
    g.sync()
    for buf, rows, n in ((dW2, Kc, "dW2"), (db2, 1, "db2"), (db1, 1, "db1")):
        _whole(buf, rows, f"{what} {n}")
    out.update(dW2=dW2[:Kc].cpu(), db2=db2[0].cpu(), db1=db1[0].cpu())
    return out


def _head_paths(Kc):
    return ("one", "split") if Kc <= R.HEAD_KMAX else ("split",)


def _head_check(got, inp, B, E, Kc, path, stats, exact):
    what = f"B {B} {path}"
    dz64, floor = R.head_dz(inp)
    wg = R.head_wgrad(inp)
    if exact:
        X.assert_bitwise(got["dz"], X.rne(dz64, BF), f"{what} dz")
        assert bool((got["dz"][0] == 0).all()), f"{what}: the saturated row's gradient is not exactly zero"
        X.assert_bitwise(got["dW2"], X.rne(wg["dW2"][0], F32), f"{what} dW2")
        X.assert_bitwise(got["db2"], X.rne(wg["db2"][0], F32), f"{what} db2")
        X.assert_bitwise(got["db1"], X.rne(R.head_db1(dz64, inp["db1_0"])[0], F32), f"{what} db1")
    else:
        X.assert_ulps(got["dz"], dz64, f"{what} dz", ulps=1.0, floor=floor)
        stats[f"{path} dz"] = max(stats.get(f"{path} dz", 0.0), float(((got["dz"].double() - dz64).abs() / (X.bf16_ulp(dz64) + floor)).max()))
        R.within(got["dW2"], *wg["dW2"], f"{what} dW2", stats, f"{path} dW2")
        R.within(got["db2"], *wg["db2"], f"{what} db2", stats, f"{path} db2")
        R.within(got["db1"], *R.head_db1(got["dz"], inp["db1_0"]), f"{what} db1 (sum of the kernel's own rounded dz)", stats, f"{path} db1")
    if path != "one":
        return
    # every partial row against the float64 sum of its own 32 batch rows
    for y in range(R.head_parts(B)):
        rows = slice(y * R.HEAD_ROWS, min(B, (y + 1) * R.HEAD_ROWS))
        pw = R.head_wgrad(inp, rows=rows, start=False)
        row = got["part"][y]
        segs = (("dW2", row[:Kc * E].reshape(Kc, E), pw["dW2"]), ("db1", row[Kc * E:(Kc + 1) * E], R.head_db1(dz64 if exact else got["dz"], rows=rows)),
                ("db2", row[(Kc + 1) * E:], pw["db2"]))
        for n, seg, (ref, lim) in segs:
            if exact:
                X.assert_bitwise(seg.contiguous(), X.rne(ref, F32), f"{what} part row {y} {n}")
            else:
                R.within(seg, ref, lim, f"{what} part row {y} {n}", stats, f"one part {n}")


def _head_case(B, E, Kc, stats, exact):
    inp = R.head_exact_inputs(B, E, Kc) if exact else R.head_inputs(B, E, Kc)
    ref, lim = R.head_fwd(inp)
    logits = _head_fwd_run(inp, B, E, Kc)
    if exact:
        X.assert_bitwise(logits, X.rne(ref, F32), f"B {B} logits")
    else:
        R.within(logits, ref, lim, f"B {B} logits", stats, "logits")
    full = {}
    for path in _head_paths(Kc):
        full[path] = _head_bwd_run(inp, B, E, Kc, path)
        _head_check(full[path], inp, B, E, Kc, path, stats, exact)
    # dz only: the same kernel as the full call of the shape's own path, the same bits
    own = "one" if Kc <= R.HEAD_KMAX else "split"
    only = _head_bwd_run(inp, B, E, Kc, own, want_wgrad=0)
    X.assert_bitwise(only["dz"], full[own]["dz"], f"B {B}: dz of the dz-only call against the full call")
    if exact and len(full) == 2:
        X.assert_bitwise(full["split"]["dz"], full["one"]["dz"], f"B {B}: dz of the two paths on the exact probe")


@pytest.mark.parametrize("Kc", HEAD_KC)
@pytest.mark.parametrize("E", HEAD_E)
def test_head_random_probe(E, Kc):
    """logits, dW2, db2 within gamma(n) sum|terms| of float64, dz within one bf16 ulp (the gamma bound as the floor), db1 the sum of
    the kernel's own rounded dz; on the one-launch path every partial row against its own 32 rows, then their fold"""
    stats = {}
    X.collect(HEAD_B, lambda B: _head_case(B, E, Kc, stats, False), f"E {E} Kc {Kc} ")
    _show(f"head E {E} Kc {Kc}:", stats)


@pytest.mark.parametrize("Kc", HEAD_KC)
@pytest.mark.parametrize("E", HEAD_E)
def test_head_exact_probe(E, Kc):
    """t in {0, +-0.5, +-1}, dlog in {-1, 0, 1}, integer W2: every value is exact, every output bit for bit on both paths"""
    X.collect(HEAD_B, lambda B: _head_case(B, E, Kc, None, True), f"E {E} Kc {Kc} ")


@pytest.mark.parametrize("E", HEAD_E)
def test_head_17_classes_with_an_empty_class_is_its_16_class_twin(E):
    """a Kc = 17 problem whose 17th class has zero weight, bias, dlog and start values runs the separate kernels and must agree with
    the same problem at Kc = 16 on either path: dz to one bf16 ulp, the gradients and logits within the bound"""
    stats = {}

    def one(B):
        a = R.head_inputs(B, E, 16)
        pad = lambda x, dim: torch.cat([x, torch.zeros_like(x.narrow(dim, 0, 1))], dim)  # noqa: E731
        b = {"t": a["t"], "db1_0": a["db1_0"], "W2": pad(a["W2"], 0), "b2": pad(a["b2"], 0), "dlog": pad(a["dlog"], 1), "dW2_0": pad(a["dW2_0"], 0),
             "db2_0": pad(a["db2_0"], 0)}
        ref, lim = R.head_fwd(a)
        lb = _head_fwd_run(b, B, E, 17)
        R.within(lb[:, :16], ref, lim, f"B {B} logits of the first 16 classes", stats, "logits")
        assert bool((lb[:, 16] == 0).all()), f"B {B}: the empty class's logit is not zero"
        wide = _head_bwd_run(b, B, E, 17, "split")
        dz64, floor = R.head_dz(a)
        wg = R.head_wgrad(a)
        for path in ("one", "split"):
            twin = _head_bwd_run(a, B, E, 16, path)
            X.assert_ulps(wide["dz"], twin["dz"].double(), f"B {B} dz against the {path} twin", ulps=1.0, floor=floor)
            X.assert_ulps(twin["dz"], dz64, f"B {B} {path} twin dz", ulps=1.0, floor=floor)
            R.within(twin["dW2"], *wg["dW2"], f"B {B} {path} twin dW2", stats, "dW2")
            R.within(twin["db2"], *wg["db2"], f"B {B} {path} twin db2", stats, "db2")
        X.assert_ulps(wide["dz"], dz64, f"B {B} dz", ulps=1.0, floor=floor)
        R.within(wide["dW2"][:16], *wg["dW2"], f"B {B} dW2", stats, "dW2")
        R.within(wide["db2"][:16], *wg["db2"], f"B {B} db2", stats, "db2")
        assert bool((wide["dW2"][16] == 0).all()) and float(wide["db2"][16]) == 0.0, f"B {B}: the empty class received a gradient"
    X.collect([1, 9, 33, 130], one, f"E {E} B ")
    _show(f"head Kc 17 twin E {E}:", stats)


# ------------------------------------------------------------------------------------------------------------------ batch sum
BS_B, BS_S, BS_E = [1, 31, 32, 33, 96, 97, 128, 129, 225], [1, 5, 17], [64, 128, 384]


@pytest.mark.parametrize("E", BS_E)
def test_batch_sum(E):
    """B across the 32 batch lanes, the four-deep main loop's b + 96 < B and its remainder loop; integers bit for bit, the random
    probe within gamma(B) sum_b |g|"""
    g, stats = _u(), {}

    def one(case):
        B, S, exact = case
        x64 = R.batch_sum_inputs(B, S, E, exact)
        ref, lim = R.batch_sum(x64)
        if not exact:
            R.detects(lim, 0.25, "batch_sum")
        x = g.dev(x64.reshape(B * S, E), BF)
        out = X.guarded(S, E, F32, "cuda", guard=4)
        g.call("vg_batch_sum", g.ptr(x), g.ptr(out), B, S, E, g.stream())
        g.sync()
        _whole(out, S, "out")
        if exact:
            X.assert_bitwise(out[:S].cpu(), X.rne(ref, F32), "out")
        else:
            R.within(out[:S], ref, lim, "out", stats, "out")
    X.collect([(B, S, ex) for B in BS_B for S in BS_S for ex in (True, False)], one, f"E {E} (B, S, exact) ")
    _show(f"vg_batch_sum E {E}:", stats)


# ------------------------------------------------------------------------------------------------- embedding's small gradients
@pytest.mark.parametrize("E", [128, 384])
def test_embed_small_grads(E):
    """the three outputs accumulate onto non-zero contents; nothing is written past d_pos[(S - 1) E)"""
    g, stats = _u(), {}

    def one(case):
        S, exact = case
        inp = R.embed_inputs(S, E, exact)
        want = R.embed_small_grads(inp)
        tok = g.dev(inp["tok"], F32)
        bufs = {"d_cls": _filled(inp["cls_0"][None], F32, 1), "d_pos": _filled(inp["pos_0"], F32, 4), "d_bias": _filled(inp["bias_0"][None], F32, 1)}
        g.call("vg_embed_small_grads", g.ptr(tok), g.ptr(bufs["d_cls"]), g.ptr(bufs["d_pos"]), g.ptr(bufs["d_bias"]), S, E, g.stream())
        g.sync()
        if not exact:
            R.detects(want["d_bias"][1], 0.25, "d_bias")
        for n, buf in bufs.items():
            rows = S - 1 if n == "d_pos" else 1
            _whole(buf, rows, n)
            ref, lim = want[n]
            if exact:
                X.assert_bitwise(buf[:rows].cpu(), X.rne(ref.reshape(rows, E), F32), n)
            else:
                R.within(buf[:rows], ref.reshape(rows, E), lim.reshape(rows, E), n, stats, n)
    X.collect([(S, ex) for S in (2, 5, 65) for ex in (True, False)], one, f"E {E} (S, exact) ")
    _show(f"vg_embed_small_grads E {E}:", stats)


# -------------------------------------------------------------------------------------------------- row movers and vg_fill_cls
MOVER_SHAPES = [(B, S, E) for B in (1, 3, 35) for S in (2, 17, 65) for E in (128, 384)]


def _rand_bf16(shape, seed):
    return torch.randn(shape, generator=X.gen(seed), dtype=F32).to(BF)


def _step_counter():
    return torch.tensor([7], dtype=torch.int32, device="cuda")


def test_take_rows():
    """bit-exact against indexing: the patch rows (first 1, n S - 1), the CLS row (first 0, n 1) and one interior window"""
    g = _u()

    def one(shape):
        B, S, E = shape
        x = _rand_bf16((B * S, E), B * S + E)
        xd = x.cuda()
        for first, n in {(1, S - 1), (0, 1), (S // 3, max(1, S // 2))}:
            out = X.guarded(B * n, E, BF, "cuda", guard=8)
            g.call("vg_take_rows", g.ptr(xd), g.ptr(out), B, S, first, n, E, g.stream())
            g.sync()
            _whole(out, B * n, f"first {first} n {n}")
            X.assert_bitwise(out[:B * n].cpu(), R.take_rows(x, B, S, first, n).contiguous(), f"first {first} n {n}")
    X.collect(MOVER_SHAPES, one, "(B, S, E) ")


def _dropout_of(buf, p, site, step):
    """vg_dropout_apply over the whole of buf"""
    g = _u()
    y = torch.empty_like(buf)
    g.call("vg_dropout_apply", g.ptr(buf), g.ptr(y), buf.numel(), p, SEED, site, g.ptr(step), g.stream())
    g.sync()
    return y


def test_scatter_cls_and_its_masked_copy():
    """zero fill plus row copy, bit for bit; gm is vg_dropout_apply run over the whole scattered buffer with the same (p, seed, site,
    step), with step NULL and a device counter; p = 0 writes no gm; the pair form is two plain scatters"""
    g = _u()

    def one(shape):
        B, S, E = shape
        src, src2 = _rand_bf16((B, E), B + S + E), _rand_bf16((B, E), B + S + E + 1)
        want = R.scatter_cls(src, S)
        sd, sd2 = src.cuda(), src2.cuda()
        for step in (None, _step_counter()):
            out, gm = X.guarded(B * S, E, BF, "cuda", guard=8), X.guarded(B * S, E, BF, "cuda", guard=8)
            g.call("vg_scatter_cls", g.ptr(sd), g.ptr(out), g.ptr(gm), B, S, E, P_DROP, SEED, 4, g.ptr(step), g.stream())
            g.sync()
            what = f"step {'NULL' if step is None else 'device'}"
            _whole(out, B * S, what + " g")
            _whole(gm, B * S, what + " gm")
            X.assert_bitwise(out[:B * S].cpu(), want, what + " g")
            X.assert_bitwise(gm[:B * S], _dropout_of(out[:B * S], P_DROP, 4, step), what + " gm against vg_dropout_apply")
            assert int((gm[:B * S][::S] == 0).sum()) > 0 or B * E < 64, what + ": the mask dropped nothing"
        out, gm = X.guarded(B * S, E, BF, "cuda", guard=8), X.guarded(B * S, E, BF, "cuda", guard=8)
        g.call("vg_scatter_cls", g.ptr(sd), g.ptr(out), g.ptr(gm), B, S, E, 0.0, SEED, 4, None, g.stream())
        out2 = X.guarded(B * S, E, BF, "cuda", guard=8)
        g.call("vg_scatter_cls", g.ptr(sd), g.ptr(out2), None, B, S, E, P_DROP, SEED, 4, None, g.stream())
        pa, pb = X.guarded(B * S, E, BF, "cuda", guard=8), X.guarded(B * S, E, BF, "cuda", guard=8)
        g.call("vg_scatter_cls_pair", g.ptr(sd), g.ptr(pa), g.ptr(sd2), g.ptr(pb), B, S, E, g.stream())
        g.sync()
        X.assert_guard(gm, 0, "p = 0: gm written")
        for buf, w, n in ((out, want, "p = 0 g"), (out2, want, "gm NULL g"), (pa, want, "pair a"), (pb, R.scatter_cls(src2, S), "pair b")):
            _whole(buf, B * S, n)
            X.assert_bitwise(buf[:B * S].cpu(), w, n)
    X.collect(MOVER_SHAPES, one, "(B, S, E) ")


def test_fill_cls():
    """p = 0: bf16(cls) bit for bit on rows b S, no other row written.  p > 0: the zero pattern is vg_dropout_apply's on ones at the
    same indices, kept elements within one bf16 ulp of cls / keep."""
    g = _u()
    thr = round(P_DROP * 256)
    keep = (256 - thr) / 256.0

    def one(shape):
        B, S, E = shape
        cls64 = R.mags((E,), X.gen(E + S))
        cls = g.dev(cls64, F32)
        for p, step in ((0.0, None), (P_DROP, None), (P_DROP, _step_counter())):
            what = f"p {p} step {'NULL' if step is None else 'device'}"
            x = X.guarded(B * S, E, BF, "cuda", guard=8)
            g.call("vg_fill_cls", g.ptr(x), g.ptr(cls), B, S, E, p, SEED, 0, g.ptr(step), g.stream())
            g.sync()
            X.assert_guard(x, B * S, what)
            rows = x[:B * S].reshape(B, S, E)
            X.assert_written(rows[:, 0], B, what + " CLS rows")
            if S > 1:
                X.assert_guard(rows[:, 1:].reshape(-1, E), 0, what + ": a row that is not a CLS row was written")
            got = rows[:, 0].cpu()
            if p == 0.0:
                X.assert_bitwise(got.contiguous(), cls64.float().to(BF).expand(B, E).contiguous(), what)
                continue
            mask = g.dropout_mask((B, S, E), p, SEED, 0, step)[:, 0]
            assert torch.equal(got == 0, mask == 0), what + ": zero pattern differs from vg_dropout_apply's"
            assert 0 < int((mask == 0).sum()) < mask.numel() or B * E < 64
            kept = mask != 0
            X.assert_ulps(got[kept], (cls64 / keep).expand(B, E)[kept], what + " kept elements", ulps=1.0)
    X.collect(MOVER_SHAPES, one, "(B, S, E) ")


# ------------------------------------------------------------------------------------------------------------------- patchify
@pytest.mark.parametrize("C_,IH,P", [(3, 32, 4), (1, 32, 4), (3, 64, 8), (3, 48, 16), (2, 16, 16)])
def test_patchify_and_unpatchify(C_, IH, P):
    """bit-exact against the torch restatement (the fp32 path rounds as tensor.to(bfloat16)); unpatchify(patchify(x)) == x"""
    g = _u()
    NP, K = (IH // P) ** 2, C_ * P * P
    for B in (1, 3):
        img32 = torch.randn(B, C_, IH, IH, generator=X.gen(B + IH + P), dtype=F32)
        want = R.patchify(img32.to(BF), P).contiguous()
        for is_bf16 in (0, 1):
            src = (img32.to(BF) if is_bf16 else img32).cuda()
            A = X.guarded(B * NP, K, BF, "cuda", guard=8)
            g.call("vg_patchify", g.ptr(src), is_bf16, g.ptr(A), B, C_, IH, P, g.stream())
            back = X.guarded(B * C_ * IH, IH, BF, "cuda", guard=8)
            g.call("vg_unpatchify", g.ptr(A), g.ptr(back), B, C_, IH, P, g.stream())
            g.sync()
            what = f"B {B} {'bf16' if is_bf16 else 'fp32'} image"
            _whole(A, B * NP, what + " A")
            _whole(back, B * C_ * IH, what + " round trip")
            X.assert_bitwise(A[:B * NP].cpu(), want, what + " A")
            X.assert_bitwise(back[:B * C_ * IH].cpu(), img32.to(BF).reshape(B * C_ * IH, IH), what + ": unpatchify(patchify(x))")
        dA = _rand_bf16((B * NP, K), B + K)
        dAd, d_img = dA.cuda(), X.guarded(B * C_ * IH, IH, BF, "cuda", guard=8)
        g.call("vg_unpatchify", g.ptr(dAd), g.ptr(d_img), B, C_, IH, P, g.stream())
        g.sync()
        _whole(d_img, B * C_ * IH, f"B {B} d_img")
        X.assert_bitwise(d_img[:B * C_ * IH].cpu(), R.unpatchify(dA, B, C_, IH, P).reshape(B * C_ * IH, IH).contiguous(), f"B {B} d_img")


# ----------------------------------------------------------------------------------------------------------------- slab folds
@pytest.mark.parametrize("accumulate", [0, 1])
def test_slab_reduce(accumulate):
    """whole slices are added in slice order: a numpy float32 loop in that order matches bit for bit on random floats, and on integers;
    stride > n with sentinels between the slices; the pair form equals two single calls"""
    g = _u()

    def one(case):
        nslab, n, exact = case
        stride = n + 12
        slabs = [R.slab_inputs(nslab, n, stride, exact, seed) for seed in (0, 1)]
        dev = [(s.cuda(), st) for s, st in slabs]

        def dst_of(st):
            return _filled(st[None].double(), F32, 1) if accumulate else _vec(n)
        singles = []
        for (sd, st), (s, _) in zip(dev, slabs):
            dst = dst_of(st)
            g.call("vg_slab_reduce", g.ptr(sd), stride, nslab, g.ptr(dst), n, accumulate, g.stream())
            g.sync()
            _whole(dst, 1, "dst")
            X.assert_bitwise(dst[0].cpu(), R.slab_reduce(s, n, st, accumulate), "dst")
            if exact:
                X.assert_bitwise(dst[0].cpu(), X.rne(s[:, :n].double().sum(0) + (st.double() if accumulate else 0.0), F32), "dst against the exact sum")
            singles.append(dst[0].cpu())
        d0, d1 = dst_of(slabs[0][1]), dst_of(slabs[1][1])
        g.call("vg_slab_reduce_pair", g.ptr(dev[0][0]), g.ptr(dev[1][0]), stride, nslab, g.ptr(d0), g.ptr(d1), n, accumulate, g.stream())
        g.sync()
        for d, s, n_ in ((d0, singles[0], "pair dst0"), (d1, singles[1], "pair dst1")):
            _whole(d, 1, n_)
            X.assert_bitwise(d[0].cpu(), s, n_ + " against the single call")
    X.collect([(ns, n, ex) for ns in (1, 2, 7, 8, 9, 32) for n in (4, 1020, 4100) for ex in (True, False)], one, "(nslab, n, exact) ")


# ------------------------------------------------------------------------------------------------------------- position table
def test_add_table():
    """one float32 add and one rounding per element, in place: (x.float() + table[r % T]).to(bfloat16) bit for bit"""
    g = _u()

    def one(case):
        B, T, E = case
        rows = B * T
        x, table = _rand_bf16((rows, E), rows + E), torch.randn(T, E, generator=X.gen(T + E), dtype=F32)
        buf = X.guarded(rows, E, BF, "cuda", guard=8)
        buf[:rows] = x.cuda()
        td = table.cuda()
        g.call("vg_add_table", g.ptr(buf), g.ptr(td), rows, E, T, g.stream())
        g.sync()
        X.assert_guard(buf, rows, "x")
        X.assert_bitwise(buf[:rows].cpu(), R.add_table(x, table, T), "x")
    X.collect([(B, T, E) for B in (1, 3) for T in (5, 64) for E in (128, 384)], one, "(B, T, E) ")


# ------------------------------------------------------------------------------------------------------------- SIREN gradient
def test_sin_grad():
    """dz = bf16(dy w0 cos(w0 z)) at w0 = 30, |w0 z| <= 120, the zero crossings of the cosine included: within one bf16 ulp of the
    float64 value plus |dy| w0 (2^-24 |w0 z| + eps_cos), eps_cos = 2 EPS_COS_MEASURED <= 2^-10"""
    g, stats = _u(), {}
    for n in (4, 1020, 4100):
        dy64, z = R.sin_inputs(n)
        ref, lim = R.sin_grad(dy64, z, 2.0 * EPS_COS_MEASURED)
        dy, zd, dz = g.dev(dy64, BF), z.cuda(), _vec(n, BF)
        g.call("vg_sin_grad", g.ptr(dy), g.ptr(zd), g.ptr(dz), n, R.W0, g.stream())
        g.sync()
        _whole(dz, 1, f"n {n} dz")
        R.within(dz[0], ref, lim, f"n {n} dz", stats, f"n {n}")
    _show("vg_sin_grad:", stats)
