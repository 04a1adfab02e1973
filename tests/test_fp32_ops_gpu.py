"""fp32 mode, per operator: each fp32 kernel through the C ABI against an fp64 CPU computation on the same fp32 inputs.

GEMMs: |got - ref| <= 4e-7 * sum_k |a_k b_k| per output (the f32-input MFMA is a k-ordered fmaf chain: ~1e-7 of that sum at
K <= 1024, with margin), plus a few fp32 ulps of |ref| for the epilogue's own arithmetic.  LayerNorm and attention: 1e-5 of
max|ref| per tensor.
"""
import ctypes as C
import math

import pytest
import torch

import gpu_util as u

pytestmark = pytest.mark.gpu

GEMM_REL = 4e-7
OP_TOL = 1e-5


def _gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _check_gemm(got, ref, absum, what, extra=0.0, extra_abs=0.0):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bound = GEMM_REL * absum + extra * ref.abs() + extra_abs + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, f"{what}: error {worst:.3f} x the bound (max err {float(err.max()):.3e})"
    return worst


# the engine's Linears at C2 (16 640 = 256 x 65 rows; 33 280 = the fused real + fake pass), the C4 / C5 widths, ragged rows
FWD_SHAPES = [(16640, 1152, 384), (33280, 384, 768), (16640, 768, 384), (4160, 512, 512), (2080, 768, 768), (1037, 384, 384), (77, 96, 768),
              (5, 1, 384)]


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_f32_fwd(M, N, K, act):
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + act)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    R = torch.randn(M, N, generator=g)
    X64, W64 = X.double(), W.double()
    pre = X64 @ W64.t() + b.double()
    absum = X64.abs() @ W64.abs().t() + b.double().abs()
    dX, dW, db, dR = (t.cuda() for t in (X, W, b, R))
    Y = torch.empty(M, N, device="cuda")
    Z = torch.empty(M, N, device="cuda") if act == 1 else None
    u.call("vg_linear_f32_fwd", u.ptr(dX), u.ptr(dW), u.ptr(db), u.ptr(dR), u.ptr(Y), u.ptr(Z), M, N, K, act, 0.0, 0, 0, None, u.stream())
    u.sync()
    if act == 1:
        _check_gemm(Z, pre, absum, "pre-activation")
        ref = _gelu64(pre)
        # GELU' <= 1.13: the GEMM's error passes through it; erff / expf add a few ulps
        _check_gemm(Y - dR, ref, 1.13 * absum, "gelu", extra=1e-6)
    elif act == 2:
        _check_gemm(Y - dR, torch.tanh(pre), absum, "tanh", extra=1e-6)
    else:
        _check_gemm(Y - dR, pre, absum, "linear", extra=2e-7)


def test_linear_f32_fwd_dropout_mask_is_the_engines():
    """The dropout epilogue multiplies by exactly the mask vg_dropout_apply produces for (p, seed, site) over the [M, N] output."""
    M, N, K, p, seed, site = 1040, 384, 384, 0.1, 1234, 3
    g = torch.Generator().manual_seed(5)
    X, W = torch.randn(M, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / 20).cuda()
    Y0, Y1 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    u.call("vg_linear_f32_fwd", u.ptr(X), u.ptr(W), None, None, u.ptr(Y0), None, M, N, K, 0, 0.0, 0, 0, None, u.stream())
    u.call("vg_linear_f32_fwd", u.ptr(X), u.ptr(W), None, None, u.ptr(Y1), None, M, N, K, 0, p, seed, site, None, u.stream())
    m = u.dropout_mask((M, N), p, seed, site).cuda()
    keep = torch.tensor(256.0 / (256.0 - round(p * 256)), dtype=torch.float32)
    mask = (m > 0).float() * keep.cuda()
    assert 0.85 < float((m > 0).float().mean()) < 0.95
    assert torch.equal(Y1, Y0 * mask)


@pytest.mark.parametrize("M,N,K", [(16640, 384, 768), (16640, 1152, 384), (33280, 384, 384), (2080, 512, 1024), (1037, 768, 1536), (5, 1, 384)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_f32_dgrad(M, N, K, act):
    g = torch.Generator().manual_seed(M + N + K + 11 * act)
    dY = torch.randn(M, N, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(N)
    aux = torch.randn(M, K, generator=g) * 2 if act == 1 else torch.tanh(torch.randn(M, K, generator=g))
    prod = dY.double() @ W.double()
    absum = dY.double().abs() @ W.double().abs()
    mul = {0: torch.ones_like(prod), 1: _gelu_grad64(aux.double()), 2: 1.0 - aux.double() ** 2}[act]
    ddY, dW, daux = dY.cuda(), W.cuda(), aux.cuda()
    dX = torch.empty(M, K, device="cuda")
    u.call("vg_linear_f32_dgrad", u.ptr(ddY), u.ptr(dW), u.ptr(daux) if act else None, u.ptr(dX), M, N, K, act, u.stream())
    u.sync()
    # the multiplier's own fp32 evaluation: GELU' = Phi(x) + x phi(x) cancels near x = -0.75, so its error is a few ulps of its
    # terms (<= 1.5), not of the product - an epilogue term on top of the GEMM's bound
    _check_gemm(dX, prod * mul, absum * mul.abs(), f"dgrad act {act}", extra=1e-6 if act else 0.0,
                extra_abs=1e-6 * prod.abs() if act == 1 else 0.0)


@pytest.mark.parametrize("M,N,K", [(16640, 1152, 384), (16640, 384, 768), (33280, 384, 384), (33280, 768, 384), (4160, 512, 512), (16384, 768, 48),
                                   (1037, 384, 384), (5, 1, 384)])
def test_linear_f32_wgrad_accumulates_and_is_repeatable(M, N, K):
    lib = u._lib.lib()
    g = torch.Generator().manual_seed(M * 3 + N + K)
    dY, X = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    ref = dY.double().t() @ X.double()
    absum = dY.double().abs().t() @ X.double().abs()
    bref = dY.double().sum(0)
    ns = lib.vg_linear_f32_wgrad_slab_floats(M, N, K)
    assert ns > 0
    slab = torch.empty(ns, device="cuda")
    ddY, dX = dY.cuda(), X.cuda()
    outs = []
    for _ in range(2):
        dW, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        u.call("vg_linear_f32_wgrad", u.ptr(ddY), u.ptr(dX), u.ptr(dW), u.ptr(db), u.ptr(slab), ns, M, N, K, u.stream())
        u.sync()
        outs.append((dW.clone(), db.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "weight gradient not bitwise repeatable"
    # (the slices are summed in fp32 after the MFMA chains: a few more roundings than one chain, inside the same bound)
    _check_gemm(outs[0][0], ref, absum, "wgrad")
    assert float((outs[0][1].double().cpu() - bref).abs().max()) <= 1e-6 * float(dY.abs().sum(0).max()), "bias gradient"
    # G += : a second call doubles it
    u.call("vg_linear_f32_wgrad", u.ptr(ddY), u.ptr(dX), u.ptr(dW), u.ptr(db), u.ptr(slab), ns, M, N, K, u.stream())
    u.sync()
    assert torch.equal(dW, 2 * outs[0][0]) and torch.equal(db, 2 * outs[0][1])


@pytest.mark.parametrize("M,K", [(64, 64), (130, 130), (16, 200)])
def test_linear_f32_identity_with_asymmetric_weights(M, K):
    """A = I: every output element is one weight element (a row/column swap in the C/D map would show); B asymmetric."""
    N = 96
    X = torch.eye(M, K)
    W = torch.arange(N * K, dtype=torch.float32).reshape(N, K) * 0.001 + torch.arange(N, dtype=torch.float32)[:, None] * 7.0
    dX, dW = X.cuda(), W.cuda()
    Y = torch.empty(M, N, device="cuda")
    u.call("vg_linear_f32_fwd", u.ptr(dX), u.ptr(dW), None, None, u.ptr(Y), None, M, N, K, 0, 0.0, 0, 0, None, u.stream())
    u.sync()
    assert torch.equal(Y.cpu(), X @ W.t())
    # and the input-gradient form: dX = dY W with dY = I
    dY = torch.eye(M, N).cuda()
    W2 = W[:, :K].contiguous().cuda()
    D = torch.empty(M, K, device="cuda")
    u.call("vg_linear_f32_dgrad", u.ptr(dY), u.ptr(W2), None, u.ptr(D), M, N, K, 0, u.stream())
    u.sync()
    assert torch.equal(D.cpu(), torch.eye(M, N) @ W2.cpu())


def _attn64(qkv, B, H, S, HE, scale):
    E = H * HE
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * S, E), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,H,S,HE", [(2, 4, 65, 96), (2, 8, 65, 64), (3, 4, 17, 32), (1, 12, 65, 64), (2, 4, 80, 32), (4, 6, 5, 64)])
def test_attention_f32(B, H, S, HE):
    E = H * HE
    g = torch.Generator().manual_seed(B * 100 + H * 10 + S + HE)
    qkv = torch.randn(B * S, 3 * E, generator=g) * 1.5
    dO = torch.randn(B * S, E, generator=g)
    scale = 1.0 / math.sqrt(HE)
    q64 = qkv.double().requires_grad_(True)
    o64, lse64 = _attn64(q64, B, H, S, HE, scale)
    (o64 * dO.double()).sum().backward()
    dq, ddo = qkv.cuda(), dO.cuda()
    out, lse = torch.empty(B * S, E, device="cuda"), torch.empty(B, H, S, device="cuda")
    u.call("vg_attention_f32_fwd", u.ptr(dq), u.ptr(out), u.ptr(lse), B, H, S, HE, scale, u.stream())
    dqkv = torch.empty(B * S, 3 * E, device="cuda")
    u.call("vg_attention_f32_bwd", u.ptr(dq), u.ptr(out), u.ptr(ddo), u.ptr(lse), u.ptr(dqkv), B, H, S, HE, scale, u.stream())
    u.sync()
    u.assert_close(out, o64.detach(), OP_TOL, "out", floor=0)
    u.assert_close(lse, lse64.detach(), OP_TOL, "lse", floor=0)
    for i, nm in enumerate("qkv"):
        u.assert_close(dqkv[:, i * E:(i + 1) * E], q64.grad[:, i * E:(i + 1) * E], OP_TOL, f"d{nm}", floor=0)


@pytest.mark.parametrize("E", [128, 256, 384, 512, 640, 768, 896, 1024])
@pytest.mark.parametrize("R", [1, 77, 2083])
def test_layernorm_f32(E, R):
    lib = u._lib.lib()
    g = torch.Generator().manual_seed(E + R)
    x = torch.randn(R, E, generator=g) * 3 + 0.5
    gam, bet = 1 + 0.3 * torch.randn(E, generator=g), 0.2 * torch.randn(E, generator=g)
    dy, gres = torch.randn(R, E, generator=g), torch.randn(R, E, generator=g)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    y64 = torch.nn.functional.layer_norm(x64, (E,), g64, b64, 1e-5)
    (y64 * dy.double()).sum().backward()
    dx_, dg_, db_, dd_, dres = (t.cuda() for t in (x, gam, bet, dy, gres))
    y, mean, rstd = torch.empty(R, E, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    u.call("vg_layernorm_f32_fwd", u.ptr(dx_), u.ptr(dg_), u.ptr(db_), u.ptr(y), u.ptr(mean), u.ptr(rstd), R, E, 1e-5, u.stream())
    part = torch.empty(lib.vg_layernorm_f32_bwd_part_floats(R, E), device="cuda")
    dx = torch.empty(R, E, device="cuda")
    dgam, dbet = torch.full((E,), 0.5, device="cuda"), torch.full((E,), -0.25, device="cuda")  # accumulated into
    u.call("vg_layernorm_f32_bwd", u.ptr(dd_), u.ptr(dx_), u.ptr(mean), u.ptr(rstd), u.ptr(dg_), u.ptr(dres), u.ptr(dx), u.ptr(dgam),
           u.ptr(dbet), u.ptr(part), R, E, u.stream())
    u.sync()
    u.assert_close(y, y64.detach(), OP_TOL, "y", floor=0)
    u.assert_close(mean, x64.detach().mean(-1), OP_TOL, "mean", floor=0)
    u.assert_close(dx, x64.grad + gres.double(), OP_TOL, "dx", floor=0)
    u.assert_close(dgam - 0.5, g64.grad, OP_TOL, "dgamma", floor=1e-6)
    u.assert_close(dbet + 0.25, b64.grad, OP_TOL, "dbeta", floor=1e-6)
