"""tests/ends_ref.py checked on the CPU, both halves of its contract: a float32 evaluation of every sum, in three different orders,
stays inside the bound the GPU test uses, and the same sum with any one term deleted does not; the restatements agree with torch in
float64 (F.linear + tanh autograd, unfold / permute, plain indexing); every exact probe really is exact."""
import math

import pytest
import torch
import torch.nn.functional as F

import ends_ref as R
import exact_util as X
from exact_util import BF

F32, F64 = torch.float32, torch.float64
HEAD_CASES = [(1, 128, 1), (9, 128, 10), (33, 128, 17), (130, 384, 40), (65, 384, 16)]


def _sum_cases():
    """(name, fp32 terms [n, cols], extra roundings per term, smallest |term|) for every sum the GPU test bounds, a few columns each"""
    out = []
    for B, E, Kc in HEAD_CASES:
        inp = R.head_inputs(B, E, Kc)
        t, W2, b2, dlog = (inp[k].float() for k in ("t", "W2", "b2", "dlog"))
        ks, es = list(range(min(Kc, 3))), [0, E // 2, E - 1]
        nb = min(B, 3)
        out.append((f"logits {B, E, Kc}", torch.cat([t[:nb].T[:, :, None] * W2[ks].T[:, None, :], b2[ks].expand(1, nb, len(ks))]).reshape(E + 1, -1), 1, 1 / 16))
        out.append((f"dz inner {B, E, Kc}", (dlog.T[:, :, None] * W2[:, None, es]).reshape(Kc, -1), 1, 1 / 16))
        out.append((f"dW2 {B, E, Kc}", torch.cat([dlog[:, ks, None] * t[:, None, es], inp["dW2_0"].float()[ks][:, es][None]]).reshape(B + 1, -1), 1, 1 / 16))
        out.append((f"db2 {B, E, Kc}", torch.cat([dlog, inp["db2_0"].float()[None]]), 0, 0.25))
    for B in (1, 33, 97, 225):
        out.append((f"batch_sum B {B}", R.batch_sum_inputs(B, 2, 64, False).float().reshape(B, -1), 0, 0.25))
    for S in (2, 5, 65):
        inp = R.embed_inputs(S, 128, False)
        out.append((f"d_bias S {S}", torch.cat([inp["tok"][1:], inp["bias_0"][None]]).float(), 0, 0.25))
    return out


def test_every_order_of_an_fp32_sum_is_inside_the_bound_and_a_deleted_term_is_not():
    for name, terms, extra, min_term in _sum_cases():
        n = terms.shape[0]
        t64 = terms.double()
        ref, bound = t64.sum(0), R.gamma(n + extra) * t64.abs().sum(0)
        assert float(t64.abs().min()) >= min_term * (1 - 2 * R.U), name   # (a product of two fp32 values, rounded)
        R.detects(bound, min_term * (1 - 2 * R.U), name)
        for order in R.ORDERS:
            got = R.sum_f32(terms, order)
            assert bool(((got.double() - ref).abs() <= bound).all()), f"{name}: order {order} outside the bound"
        # delete term i, for every i at once: [n deleted, n, cols] with a zero diagonal, summed in float32 over axis 1
        keep = (1.0 - torch.eye(n, dtype=F32))[:, :, None]
        for order in R.ORDERS:
            holed = R.sum_f32((keep * terms[None]).transpose(0, 1).contiguous(), order)   # [n deleted, cols]
            assert bool(((holed.double() - ref[None]).abs() > bound[None]).all()), f"{name}: a deleted term passes in order {order}"
            doubled = R.sum_f32(((2.0 - keep) * terms[None]).transpose(0, 1).contiguous(), order)
            assert bool(((doubled.double() - ref[None]).abs() > bound[None]).all()), f"{name}: a doubled term passes in order {order}"


def test_gamma_and_within():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and R.gamma(1000) > 1000 * R.U
    stats = {}
    assert R.within(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.5], dtype=F64), torch.tensor([0.0, 1.0], dtype=F64), "x", stats) == 0.5
    with pytest.raises(AssertionError):
        R.within(torch.tensor([1.0, 2.0]), torch.tensor([1.5, 2.0], dtype=F64), 0.25, "x")
    with pytest.raises(AssertionError):
        R.within(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0 + 1e-9], dtype=F64), 0.0, "x")
    with pytest.raises(AssertionError):
        R.detects(torch.tensor([0.2]), 0.25, "x")


@pytest.mark.parametrize("B,E,Kc", HEAD_CASES)
def test_head_restatement_against_autograd(B, E, Kc):
    """logits = F.linear(t, W2, b2) with t = tanh(z): the restated dz is autograd's gradient at z, dW2 / db2 those of fc2"""
    inp = R.head_inputs(B, E, Kc)
    z = torch.atanh(inp["t"]).requires_grad_(True)
    W2, b2 = inp["W2"].clone().requires_grad_(True), inp["b2"].clone().requires_grad_(True)
    logits = F.linear(torch.tanh(z), W2, b2)
    logits.backward(inp["dlog"])
    ref, lim = R.head_fwd(inp)
    assert torch.allclose(ref, logits.detach(), rtol=1e-12, atol=1e-12) and float(lim.min()) > 0
    dz, floor = R.head_dz(inp)
    assert torch.allclose(dz, z.grad, rtol=1e-9, atol=1e-12) and float(floor.min()) > 0
    wg = R.head_wgrad(inp, start=False)
    assert torch.allclose(wg["dW2"][0], W2.grad, rtol=1e-12, atol=1e-12) and torch.allclose(wg["db2"][0], b2.grad, rtol=1e-12, atol=1e-12)
    # partial rows add up to the whole, and the start value enters once
    parts = [R.head_wgrad(inp, rows=slice(HEAD * 32, HEAD * 32 + 32), start=False) for HEAD in range(R.head_parts(B))]
    assert torch.allclose(sum(p["dW2"][0] for p in parts) + inp["dW2_0"], R.head_wgrad(inp)["dW2"][0], rtol=1e-12, atol=1e-12)
    db1, _ = R.head_db1(dz.to(BF), inp["db1_0"])
    assert torch.allclose(db1, dz.to(BF).double().sum(0) + inp["db1_0"])
    # the random probe's condition holds at this shape for every output whose terms are inputs
    mins = R.head_min_terms()
    R.detects(lim, mins["logits"], "logits")
    R.detects(R.gamma(Kc + 1) * (inp["dlog"].abs() @ inp["W2"].abs()), mins["dz"], "dz inner sum")
    R.detects(R.head_wgrad(inp)["dW2"][1], mins["dW2"], "dW2")
    R.detects(R.head_wgrad(inp)["db2"][1], mins["db2"], "db2")
    assert R.head_parts(B) == -(-B // 32) and R.head_part_width(E, Kc) == (Kc + 1) * E + Kc


@pytest.mark.parametrize("B,E,Kc", [(1, 128, 1), (33, 128, 17), (130, 384, 40), (65, 384, 16)])
def test_head_exact_probe_is_exact(B, E, Kc):
    inp = R.head_exact_inputs(B, E, Kc)
    assert R.exact_in(inp["t"], BF) and all(R.exact_in(inp[k], F32) for k in ("W2", "b2", "dlog", "dW2_0", "db2_0", "db1_0"))
    assert bool((inp["t"][0].abs() == 1).all()), "row 0 is the saturated row"
    t, W2, dlog = inp["t"], inp["W2"], inp["dlog"]
    # every intermediate: the products, every partial sum (bounded by the sum of magnitudes: exact below 2^24 on this grid), 1 - t^2
    assert float((dlog.abs() @ W2.abs()).max()) <= 85.0
    for grid, m in ((0.5, t.abs() @ W2.abs().T + inp["b2"].abs()), (1.0, dlog.abs() @ W2.abs()),
                    (0.5, dlog.abs().T @ t.abs() + inp["dW2_0"].abs()), (1.0, dlog.abs().sum(0) + inp["db2_0"].abs())):
        assert float(m.max()) / grid < X.EXACT_LIMIT
    assert R.exact_in(t * t, F32) and R.exact_in(1 - t * t, F32)
    dz, _ = R.head_dz(inp)
    assert R.exact_in(dz, BF) and bool((dz[0] == 0).all()), "dz is a bf16, and exactly zero on the saturated row"
    assert R.exact_in(R.head_fwd(inp)[0], F32)
    wg = R.head_wgrad(inp)
    assert R.exact_in(wg["dW2"][0], F32) and R.exact_in(wg["db2"][0], F32)
    db1, _ = R.head_db1(dz, inp["db1_0"])
    assert R.exact_in(db1, F32) and float(dz.abs().sum(0).max() + 8) * 4 < X.EXACT_LIMIT


def test_batch_sum_and_embed_restatements():
    for exact in (False, True):
        g = R.batch_sum_inputs(33, 5, 64, exact)
        ref, lim = R.batch_sum(g)
        assert torch.equal(ref, torch.einsum("bse->se", g))
        if exact:
            assert R.exact_in(g, BF) and R.exact_in(ref, F32) and float(g.abs().sum(0).max()) < X.EXACT_LIMIT
        else:
            R.detects(R.batch_sum(R.batch_sum_inputs(225, 1, 64, False))[1], 0.25, "batch_sum B 225")
        inp = R.embed_inputs(65, 128, exact)
        out = R.embed_small_grads(inp)
        full = torch.cat([inp["cls_0"][None], inp["pos_0"]]) + inp["tok"]     # pos + cls gradient of x = cat(cls, patches) + pos, per token
        assert torch.equal(out["d_cls"][0], full[0]) and torch.equal(out["d_pos"][0], full[1:])
        assert torch.allclose(out["d_bias"][0], inp["bias_0"] + inp["tok"][1:].sum(0))
        if exact:
            assert all(R.exact_in(v[0], F32) for v in out.values()) and all(R.exact_in(v, F32) for v in inp.values())
        else:
            R.detects(out["d_bias"][1], 0.25, "d_bias S 65")


@pytest.mark.parametrize("C_,IH,P", [(3, 32, 4), (1, 32, 4), (3, 64, 8), (3, 48, 16), (2, 16, 16)])
def test_patchify_restatement_against_unfold(C_, IH, P):
    img = torch.randn(3, C_, IH, IH, generator=X.gen(IH + P), dtype=F64)
    A = R.patchify(img, P)
    want = F.unfold(img, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, C_ * P * P)   # [B, C P P, NP] -> rows of (c, py, px)
    assert torch.equal(A, want)
    assert torch.equal(R.unpatchify(A, 3, C_, IH, P), img)
    assert torch.equal(R.unpatchify(A, 3, C_, IH, P), F.fold(want.reshape(3, -1, C_ * P * P).transpose(1, 2), IH, kernel_size=P, stride=P))


def test_row_mover_restatements_against_indexing():
    B, S, E = 3, 17, 128
    x = torch.randn(B * S, E, generator=X.gen(1), dtype=F64)
    for first, n in ((1, S - 1), (0, 1), (5, 7)):
        got = R.take_rows(x, B, S, first, n)
        for b in range(B):
            for j in range(n):
                assert torch.equal(got[b * n + j], x[b * S + first + j])
    src = torch.randn(B, E, generator=X.gen(2), dtype=F64)
    g = R.scatter_cls(src, S)
    assert torch.equal(g[::S], src) and float(g.abs().sum()) == float(src.abs().sum())
    xb, table = torch.randn(B * 5, E, generator=X.gen(3)).to(BF), torch.randn(5, E, generator=X.gen(4))
    y = R.add_table(xb, table, 5)
    assert y.dtype == BF and torch.equal(y[7], (xb[7].float() + table[2]).to(BF))


def test_slab_restatement_and_exact_probe():
    for nslab, n in ((1, 4), (9, 1020)):
        slab, start = R.slab_inputs(nslab, n, n + 12, True)
        assert bool((slab[:, n:] == 1e30).all())
        for acc in (0, 1):
            got = R.slab_reduce(slab, n, start, acc)
            want = slab[:, :n].double().sum(0) + (start.double() if acc else 0.0)
            assert torch.equal(got.double(), want) and R.exact_in(want, F32)       # integers: exact in any order
        slab, start = R.slab_inputs(nslab, n, n + 12, False)
        got = R.slab_reduce(slab, n, start, 1)
        assert got.dtype == F32 and torch.allclose(got.double(), slab[:, :n].double().sum(0) + start.double(), atol=1e-4)


def test_sin_inputs_and_limit():
    dy, z = R.sin_inputs(1020)
    a = R.sin_arg(z)
    assert float(a.abs().max()) <= R.SIN_ARG_MAX + 1e-3
    k = torch.round(a / (math.pi / 2))
    on_grid = (a - k * math.pi / 2).abs() < 1e-4
    assert int(on_grid.sum()) >= 153 and int((on_grid & (k % 2 == 1)).sum()) >= 76, "the zero crossings of the cosine are among the arguments"
    assert R.exact_in(dy, BF) and float(dy.abs().min()) >= 0.25
    ref, lim = R.sin_grad(dy, z, 2.0 ** -12)
    assert torch.allclose(ref, dy * R.W0 * torch.cos(z.double() * R.W0)) and bool((lim > 0).all())
    # the rounded argument is inside what the limit grants for it
    assert bool(((a - z.double() * R.W0).abs() <= R.U * (z.double() * R.W0).abs() * (1 + 1e-6)).all())
    with pytest.raises(AssertionError):
        R.sin_grad(dy, z, 2.0 ** -9)
