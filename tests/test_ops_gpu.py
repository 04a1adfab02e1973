"""Parity of every HIP operator (called through the C ABI) against an fp32 PyTorch reference.

Inputs are rounded to bf16 first, so the fp32 reference sees exactly what the kernel sees; the
remaining difference is accumulation order (fp32) plus ONE bf16 rounding of the stored output:
tolerance 2^-7 * max|ref| for bf16 outputs, 2e-5 * max|ref| for fp32 outputs (pre-activations,
weight gradients, LSE, statistics).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_util as u

pytestmark = pytest.mark.gpu

BF_TOL = 2.0 ** -7
F32_TOL = 3e-5


@pytest.mark.parametrize("M,N,K", [(130, 384, 384), (260, 1152, 384), (77, 96, 768), (256, 384, 48), (64, 768, 96),
                                   (1040, 768, 384)])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_linear_fwd(M, N, K, act):
    g = torch.Generator().manual_seed(M * 7 + N + K + act)
    A = u.rbf(torch.randn(M, K, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    R = u.rbf(torch.randn(M, N, generator=g))
    scale = 30.0 if act == 2 else 0.0
    if act == 2:
        W = u.rbf(W / 30.0)
    pre = A @ W.t() + b
    ref = {0: pre, 1: F.gelu(pre), 2: torch.sin(30.0 * pre), 3: torch.tanh(pre)}[act] + R
    dA, dW, db, dR = u.dev(A, u.BF), u.dev(W, u.BF), u.dev(b), u.dev(R, u.BF)
    out = torch.empty(M, N, dtype=u.BF, device="cuda")
    pre_b = torch.empty(M, N, dtype=u.BF, device="cuda")
    pre_f = torch.empty(M, N, dtype=torch.float32, device="cuda")
    u.call("vg_linear_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), u.ptr(dR), u.ptr(out), u.ptr(pre_b), u.ptr(pre_f),
           M, N, K, act, scale, u.stream())
    u.sync()
    u.assert_close(pre_f, pre, F32_TOL, "pre_f32")
    u.assert_close(pre_b, pre, BF_TOL, "pre_bf16")
    u.assert_close(out, ref, BF_TOL, "out")


# The K = 384 Linears with M % 32 == 0 and N % 128 == 0 run on the weights-in-registers kernel (csrc/gemm_wr.hip): rows are
# dealt to the workgroups in units of 32, so the sizes below exercise runs of one short tile only (256 rows over 56-168
# runs), full tiles followed by a 32/64/96-row tile, and the full-size launches of the C2 step.
WR_SHAPES = [(256, 384), (1312, 1152), (4160, 768), (16640, 1152), (33280, 384), (33280, 768)]


@pytest.mark.parametrize("M,N", [(1312, 768), (16640, 768)])
def test_linear_gelu_fwd_weights_in_registers(M, N):
    """fc1: GELU epilogue with the bf16 pre-activation as second output."""
    K = 384
    g = torch.Generator().manual_seed(M + N)
    A = u.rbf(torch.randn(M, K, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    pre = A @ W.t() + b
    dA, dW, db = u.dev(A, u.BF), u.dev(W, u.BF), u.dev(b)
    out = torch.empty(M, N, dtype=u.BF, device="cuda")
    pre_b = torch.empty(M, N, dtype=u.BF, device="cuda")
    u.call("vg_linear_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), None, u.ptr(out), u.ptr(pre_b), None, M, N, K, 1, 0.0, u.stream())
    u.sync()
    u.assert_close(pre_b, pre, BF_TOL, "pre_bf16")
    u.assert_close(out, F.gelu(pre), BF_TOL, "gelu")


def _gelu_grad(pre):
    return 0.5 * (1.0 + torch.erf(pre * 0.7071067811865476)) + pre * 0.3989422804014327 * torch.exp(-0.5 * pre * pre)


# (1312, 768) and (16640, 1536) run on gemm_wr.hip (K = 384), the others on the tiled kernel (gemm.hip): producer and consumer of
# the one-byte derivative code have to agree across the two kernels
@pytest.mark.parametrize("M,N,K", [(1312, 768, 384), (16640, 1536, 384), (130, 768, 192), (260, 2048, 512), (77, 96, 768)])
def test_linear_gelu_fwd_byte_derivative(M, N, K):
    """fc1 as the engine runs it: bf16 gelu(pre) + gelu'(pre) as ONE BYTE per element, code = round(200 g) + 27 (exact at 0 and 1);
    decoded it is within half a grid step (0.0025) of the fp32 derivative, plus what the accumulation order moves near a rounding
    boundary (one more step)."""
    g = torch.Generator().manual_seed(M + N + K)
    A = u.rbf(torch.randn(M, K, generator=g) * 1.5)
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    pre = A @ W.t() + b
    dA, dW, db = u.dev(A, u.BF), u.dev(W, u.BF), u.dev(b)
    out = torch.full((M + 8, N), 7.0, dtype=u.BF, device="cuda")
    code = torch.full((M + 8, N), 255, dtype=torch.uint8, device="cuda")
    u.call("vg_linear_gelu_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), u.ptr(out), u.ptr(code), M, N, K, u.stream())
    u.sync()
    u.assert_close(out[:M], F.gelu(pre), BF_TOL, "gelu")
    assert bool((out[M:] == 7.0).all()) and bool((code[M:] == 255).all()), "rows beyond M were written"
    dec = (code[:M].cpu().float() - 27.0) * 0.005
    ref = _gelu_grad(pre)
    err = (dec - ref).abs()
    assert float(err.max()) <= 0.0025 + 0.005, float(err.max())
    assert float((err > 0.00251).float().mean()) < 2e-3  # off-by-one codes only where the fp32 sum sits on a rounding boundary
    assert float(err.mean()) < 0.0014                    # uniform rounding on a grid of 0.005: mean |error| = 0.00125
    sat = pre.abs() > 6.0
    if bool(sat.any()):  # saturated units: the derivative is exactly 0 or 1
        assert torch.equal(dec[sat], (pre[sat] > 0).float())
    assert int(code[:M].min()) >= 1 and int(code[:M].max()) <= 253


@pytest.mark.parametrize("M,K,N", [(1312, 768, 384), (33280, 1536, 384), (130, 768, 192), (260, 2048, 512), (100, 96, 768)])
def test_linear_dgrad_byte_derivative(M, K, N):
    """fc2 input gradient times the decoded one-byte derivative (mul_mode 8), on both kernels."""
    g = torch.Generator().manual_seed(M + 5 * K + N)
    dY = u.rbf(torch.randn(M, N, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(N))
    code = torch.randint(1, 254, (M, K), generator=g, dtype=torch.int32).to(torch.uint8)
    ref = (dY @ W) * ((code.float() - 27.0) * 0.005)
    out = torch.full((M + 64, K), 7.0, dtype=u.BF, device="cuda")
    ddY, dW_, dcode = u.dev(dY, u.BF), u.dev(W, u.BF), code.cuda()
    u.call("vg_linear_dgrad", u.ptr(ddY), u.ptr(dW_), u.ptr(out), M, N, K, 8, u.ptr(dcode), None, 0.0, u.stream())
    u.sync()
    u.assert_close(out[:M], ref, BF_TOL, "dX")
    assert bool((out[M:] == 7.0).all()), "rows beyond M were written"


@pytest.mark.parametrize("M,N", WR_SHAPES)
@pytest.mark.parametrize("res", [False, True])
def test_linear_fwd_weights_in_registers(M, N, res):
    K = 384
    g = torch.Generator().manual_seed(M + 3 * N + int(res))
    A = u.rbf(torch.randn(M, K, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    R = u.rbf(torch.randn(M, N, generator=g)) if res else None
    ref = A @ W.t() + b + (R if res else 0.0)
    dA, dW, db = u.dev(A, u.BF), u.dev(W, u.BF), u.dev(b)
    dR = u.dev(R, u.BF) if res else None
    out = torch.full((M + 64, N), 7.0, dtype=u.BF, device="cuda")  # guard rows: nothing may be written past M
    u.call("vg_linear_fwd", u.ptr(dA), u.ptr(dW), u.ptr(db), u.ptr(dR) if res else None, u.ptr(out), None, None,
           M, N, K, 0, 0.0, u.stream())
    u.sync()
    u.assert_close(out[:M], ref, BF_TOL, "out")
    assert bool((out[M:] == 7.0).all()), "rows beyond M were written"


@pytest.mark.parametrize("M,K", WR_SHAPES)
@pytest.mark.parametrize("mul", [0, 7])
def test_linear_dgrad_weights_in_registers(M, K, mul):
    """dX[M, K] = dY[M, 384] @ W[384, K] (the out-proj / fc2 input gradients), optionally times a stored derivative."""
    N = 384
    g = torch.Generator().manual_seed(M + 5 * K + mul)
    dY = u.rbf(torch.randn(M, N, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(N))
    Z = u.rbf(torch.rand(M, K, generator=g) * 1.2 - 0.1)
    ref = dY @ W
    if mul == 7:
        ref = ref * Z
    out = torch.full((M + 64, K), 7.0, dtype=u.BF, device="cuda")
    dZ, ddY, dW_ = u.dev(Z, u.BF), u.dev(dY, u.BF), u.dev(W, u.BF)
    u.call("vg_linear_dgrad", u.ptr(ddY), u.ptr(dW_), u.ptr(out), M, N, K, mul, u.ptr(dZ) if mul else None, None,
           0.0, u.stream())
    u.sync()
    u.assert_close(out[:M], ref, BF_TOL, "dX")
    assert bool((out[M:] == 7.0).all()), "rows beyond M were written"


@pytest.mark.parametrize("M,N,K", [(130, 384, 384), (260, 1152, 384), (192, 768, 96), (256, 48, 384), (100, 96, 768)])
@pytest.mark.parametrize("mul", [0, 4, 5])
def test_linear_dgrad(M, N, K, mul):
    g = torch.Generator().manual_seed(M + N * 3 + K + mul)
    dY = u.rbf(torch.randn(M, N, generator=g))
    W = u.rbf(torch.randn(N, K, generator=g) / math.sqrt(N))
    Z = u.rbf(torch.randn(M, K, generator=g))
    Zf = torch.randn(M, K, generator=g) * 0.1
    ref = dY @ W
    if mul == 4:
        zz = Z.clone().requires_grad_(True)
        F.gelu(zz).sum().backward()
        ref = ref * zz.grad
    elif mul == 5:
        ref = ref * 30.0 * torch.cos(30.0 * Zf)
    out = torch.empty(M, K, dtype=u.BF, device="cuda")
    dZ, dZf, ddY, dW_ = u.dev(Z, u.BF), u.dev(Zf), u.dev(dY, u.BF), u.dev(W, u.BF)  # keep alive across the call
    u.call("vg_linear_dgrad", u.ptr(ddY), u.ptr(dW_), u.ptr(out), M, N, K, mul, u.ptr(dZ), u.ptr(dZf),
           30.0, u.stream())
    u.sync()
    u.assert_close(out, ref, BF_TOL, "dX")


# rows % 32 == 0, N % 128 == 0, K % 384 == 0: the 128 x 384-tile kernel (csrc/gemm_tn.hip) - one, two and many stages per
# K slice, ragged last slice (65 stages over 3 slices), K = 768 (two n-tiles); the other shapes stay on the tiled kernel
@pytest.mark.parametrize("M,N,K,splits", [(1040, 384, 384, 4), (650, 1152, 384, 3), (512, 96, 768, 2), (2048, 384, 48, 8),
                                          (256, 384, 384, 1), (130, 768, 384, 5),
                                          (64, 384, 384, 2), (2080, 1152, 384, 3), (4160, 768, 384, 10), (2080, 384, 768, 5),
                                          (33280, 1152, 384, 10),
                                          (2080, 1536, 512, 4), (1040, 512, 1024, 8), (64, 128, 512, 1)])  # 128 x 512 tiles (E = 512)
def test_linear_wgrad(M, N, K, splits):
    g = torch.Generator().manual_seed(M + N + K)
    dY = u.rbf(torch.randn(M, N, generator=g))
    X = u.rbf(torch.randn(M, K, generator=g))
    prev = torch.randn(N, K, generator=g)
    ref = dY.t() @ X
    dW = u.dev(prev.clone())
    slab = torch.empty(splits * N * K, dtype=torch.float32, device="cuda")
    a, b = u.dev(dY, u.BF), u.dev(X, u.BF)
    u.call("vg_linear_wgrad", u.ptr(a), u.ptr(b), u.ptr(dW), u.ptr(slab), slab.numel(), M, N, K, splits, 1, u.stream())
    u.sync()
    u.assert_close(dW, ref + prev, F32_TOL, "dW accumulate")
    u.call("vg_linear_wgrad", u.ptr(a), u.ptr(b), u.ptr(dW), u.ptr(slab), slab.numel(), M, N, K, splits, 0, u.stream())
    u.sync()
    first = dW.clone()
    u.assert_close(dW, ref, F32_TOL, "dW overwrite")
    u.call("vg_linear_wgrad", u.ptr(a), u.ptr(b), u.ptr(dW), u.ptr(slab), slab.numel(), M, N, K, splits, 0, u.stream())
    u.sync()
    assert torch.equal(first, dW), "wgrad must be bitwise reproducible (no float atomics)"


@pytest.mark.parametrize("R,E", [(130, 384), (65, 128), (33, 512), (7, 768)])
def test_layernorm(R, E):
    g = torch.Generator().manual_seed(R + E)
    x = u.rbf(torch.randn(R, E, generator=g) * 2 + 0.5).requires_grad_(True)
    gam = (1 + 0.1 * torch.randn(E, generator=g)).requires_grad_(True)
    bet = (0.1 * torch.randn(E, generator=g)).requires_grad_(True)
    dy = u.rbf(torch.randn(R, E, generator=g))
    gres = u.rbf(torch.randn(R, E, generator=g))
    y = F.layer_norm(x, (E,), gam, bet, 1e-5)
    y.backward(dy)
    dx_ref = x.grad + gres
    X, Y = u.dev(x.detach(), u.BF), torch.empty(R, E, dtype=u.BF, device="cuda")
    mean, rstd = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    G_, B_ = u.dev(gam.detach()), u.dev(bet.detach())
    u.call("vg_layernorm_fwd", u.ptr(X), E, u.ptr(G_), u.ptr(B_), u.ptr(Y), E, u.ptr(mean), u.ptr(rstd), R, E, 1e-5, u.stream())
    u.sync()
    u.assert_close(Y, y, BF_TOL, "ln y")
    u.assert_close(mean, x.detach().mean(-1), F32_TOL, "mean")
    parts = u._lib.lib().vg_layernorm_bwd_parts(R)
    part = torch.zeros(parts, 3 * E, device="cuda")
    dX = torch.empty(R, E, dtype=u.BF, device="cuda")
    DY, GRES = u.dev(dy, u.BF), u.dev(gres, u.BF)
    u.call("vg_layernorm_bwd", u.ptr(DY), u.ptr(X), u.ptr(mean), u.ptr(rstd), u.ptr(G_), u.ptr(GRES),
           u.ptr(dX), u.ptr(part), R, E, u.stream())
    dg, db, cs = torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")
    u.call("vg_colsum_f32", u.ptr(part), parts, 3 * E, u.ptr(dg), E, u.ptr(db), E, u.ptr(cs), E, None, 0, 1, u.stream())
    u.sync()
    u.assert_close(dX, dx_ref, BF_TOL, "ln dx")
    u.assert_close(dg, gam.grad, 2e-4, "dgamma")
    u.assert_close(db, bet.grad, 2e-4, "dbeta")
    u.assert_close(cs, dX.float().sum(0), 2e-4, "colsum(dx)")


@pytest.mark.parametrize("B,T,E,bcast", [(3, 32, 384, True), (3, 32, 384, False), (2, 17, 128, False)])
def test_sln(B, T, E, bcast):
    g = torch.Generator().manual_seed(B + T + E + int(bcast))
    R = B * T
    h = u.rbf(torch.randn(T if bcast else R, E, generator=g)).requires_grad_(True)
    w = u.rbf(torch.randn(R, E, generator=g)).requires_grad_(True)
    lw = (1 + 0.1 * torch.randn(E, generator=g)).requires_grad_(True)
    lb = (0.1 * torch.randn(E, generator=g)).requires_grad_(True)
    sc = torch.tensor([0.7, -0.4]).requires_grad_(True)  # gamma, beta
    dy = u.rbf(torch.randn(R, E, generator=g))
    gres = u.rbf(torch.randn(R, E, generator=g))
    hh = h.repeat(B, 1) if bcast else h
    y = sc[0] * w * F.layer_norm(hh, (E,), lw, lb, 1e-5) + sc[1] * w
    y.backward(dy)
    H, W = u.dev(h.detach(), u.BF), u.dev(w.detach(), u.BF)
    LW, LB, SC = u.dev(lw.detach()), u.dev(lb.detach()), u.dev(sc.detach())
    Y = torch.empty(R, E, dtype=u.BF, device="cuda")
    mean, rstd = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    import ctypes as C
    gs, bs = u.ptr(SC), C.c_void_p(SC.data_ptr() + 4)
    hb = T if bcast else 0
    u.call("vg_sln_fwd", u.ptr(H), hb, u.ptr(W), u.ptr(LW), u.ptr(LB), gs, bs, u.ptr(Y), u.ptr(mean), u.ptr(rstd), R, E, 1e-5, u.stream())
    u.sync()
    u.assert_close(Y, y, BF_TOL, "sln y")
    parts = u._lib.lib().vg_layernorm_bwd_parts(R)
    PW = 3 * E + 64
    part = torch.zeros(parts, PW, device="cuda")
    dH = torch.empty(R, E, dtype=u.BF, device="cuda")
    dwacc = torch.ones(R, E, device="cuda")
    DY, GRES = u.dev(dy, u.BF), u.dev(gres, u.BF)
    u.call("vg_sln_bwd", u.ptr(DY), u.ptr(H), hb, u.ptr(W), u.ptr(mean), u.ptr(rstd), u.ptr(LW), u.ptr(LB), gs, bs,
           u.ptr(GRES), u.ptr(dH), u.ptr(dwacc), 1, u.ptr(part), R, E, u.stream())
    dlw, dlb, cs = (torch.zeros(E, device="cuda") for _ in range(3))
    dsc = torch.zeros(2, device="cuda")
    u.call("vg_colsum_f32", u.ptr(part), parts, PW, u.ptr(dlw), E, u.ptr(dlb), E, u.ptr(cs), E, u.ptr(dsc), 2, 1, u.stream())
    u.sync()
    dh_full = (h.grad if not bcast else None)
    if bcast:  # per-row dh before the batch sum: recompute with an expanded leaf
        h2 = h.detach().repeat(B, 1).requires_grad_(True)
        (sc[0].detach() * w.detach() * F.layer_norm(h2, (E,), lw.detach(), lb.detach(), 1e-5)).backward(dy)
        dh_full = h2.grad
    u.assert_close(dH, dh_full + gres, BF_TOL, "sln dh")
    u.assert_close(dwacc, w.grad + 1.0, 1e-4, "sln dw (accumulate)")
    u.assert_close(dlw, lw.grad, 3e-4, "dlw")
    u.assert_close(dlb, lb.grad, 3e-4, "dlb")
    u.assert_close(dsc, sc.grad, 3e-4, "dgamma/dbeta")


@pytest.mark.parametrize("B,H,S,HE,scale", [(3, 4, 65, 96, None), (2, 4, 32, 96, 1 / math.sqrt(384)), (2, 8, 65, 64, None),
                                            (2, 4, 65, 32, None), (2, 2, 17, 64, None), (1, 4, 80, 96, None), (2, 4, 1, 32, None)])
def test_attention(B, H, S, HE, scale):
    E = H * HE
    scale = scale or 1 / math.sqrt(HE)
    g = torch.Generator().manual_seed(B + H + S + HE)
    qkv = u.rbf(torch.randn(B * S, 3 * E, generator=g) * 1.5).requires_grad_(True)
    dO = u.rbf(torch.randn(B * S, E, generator=g))
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    sc = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(sc, -1)
    o = (p @ v).transpose(1, 2).reshape(B * S, E)
    lse_ref = torch.logsumexp(sc, -1)
    QKV = u.dev(qkv.detach(), u.BF)
    O = torch.empty(B * S, E, dtype=u.BF, device="cuda")
    LSE = torch.empty(B, H, S, device="cuda")
    u.call("vg_attention_fwd", u.ptr(QKV), u.ptr(O), u.ptr(LSE), B, H, S, HE, scale, u.stream())
    u.sync()
    u.assert_close(LSE, lse_ref, 1e-4, "lse")
    u.assert_close(O, o, 2.0 ** -6, "attn out")  # P is rounded to bf16 before P.V: one extra bf16 rounding
    o.backward(dO)
    dQKV = torch.empty(B * S, 3 * E, dtype=u.BF, device="cuda")
    DO = u.dev(dO, u.BF)
    u.call("vg_attention_bwd", u.ptr(QKV), u.ptr(O), u.ptr(DO), u.ptr(LSE), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    for i, nm in enumerate("qkv"):
        u.assert_close(dQKV[:, i * E:(i + 1) * E], qkv.grad[:, i * E:(i + 1) * E], 2.0 ** -5, f"d{nm}")


@pytest.mark.parametrize("B,H,S,HE", [(3, 4, 65, 96), (16, 4, 65, 96), (2, 8, 65, 64), (2, 12, 65, 64), (5, 2, 17, 32), (2, 4, 80, 96)])
def test_attention_cls_query(B, H, S, HE):
    """The top block's attention as the classifier sees it (one query per image, row 0): against fp32 attention, and against the
    full kernels at that row - the forward's row 0, and the backward fed a d_out that is zero on every other row."""
    E, scale = H * HE, 1 / math.sqrt(HE)
    g = torch.Generator().manual_seed(B + H + S + HE)
    qkv = u.rbf(torch.randn(B * S, 3 * E, generator=g) * 1.5).requires_grad_(True)
    dO0 = u.rbf(torch.randn(B, E, generator=g))
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    sc = (q[:, :, :1] @ k.transpose(-1, -2)) * scale                       # [B, H, 1, S]
    o0 = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, E)
    lse_ref = torch.logsumexp(sc, -1).reshape(B, H)
    QKV = u.dev(qkv.detach(), u.BF)
    Oc = torch.empty(B, E, dtype=u.BF, device="cuda")
    Lc = torch.empty(B, H, device="cuda")
    u.call("vg_attention_cls_fwd", u.ptr(QKV), u.ptr(Oc), u.ptr(Lc), B, H, S, HE, scale, u.stream())
    u.sync()
    u.assert_close(Lc, lse_ref, 1e-4, "lse of the CLS query")
    u.assert_close(Oc, o0, 2.0 ** -6, "attention output of the CLS query")
    o0.backward(dO0)
    DOc = u.dev(dO0, u.BF)
    dQKV = torch.full((B * S, 3 * E), 7.0, dtype=u.BF, device="cuda")
    u.call("vg_attention_cls_bwd", u.ptr(QKV), u.ptr(Oc), u.ptr(DOc), u.ptr(Lc), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    for i, nm in enumerate("qkv"):
        u.assert_close(dQKV[:, i * E:(i + 1) * E], qkv.grad[:, i * E:(i + 1) * E], 2.0 ** -5, f"d{nm} (CLS query)")
    dq = dQKV[:, :E].reshape(B, S, E)
    assert bool((dq[:, 1:] == 0).all()), "dQ must be exactly zero off the CLS rows"
    if S <= 80:  # the full kernels' range: same operator, same roundings - row 0 of the forward, d_out zero elsewhere in the backward
        O = torch.empty(B * S, E, dtype=u.BF, device="cuda")
        LSE = torch.empty(B, H, S, device="cuda")
        u.call("vg_attention_fwd", u.ptr(QKV), u.ptr(O), u.ptr(LSE), B, H, S, HE, scale, u.stream())
        DO = torch.zeros(B, S, E, dtype=u.BF, device="cuda")
        DO[:, 0] = DOc
        dFull = torch.empty(B * S, 3 * E, dtype=u.BF, device="cuda")
        u.call("vg_attention_bwd", u.ptr(QKV), u.ptr(O), u.ptr(DO), u.ptr(LSE), u.ptr(dFull), B, H, S, HE, scale, u.stream())
        u.sync()
        u.assert_close(Oc, O.reshape(B, S, E)[:, 0].float().cpu(), 2.0 ** -8, "forward vs the full kernel's row 0")
        u.assert_close(Lc, LSE[:, :, 0].cpu(), 1e-5, "lse vs the full kernel's")
        u.assert_close(dQKV, dFull.float().cpu(), 2.0 ** -7, "backward vs the full kernel with d_out zero off the CLS rows")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("role", [0, 1, 2])
def test_gan_loss(kind, role):
    from oracle import step_oracle as so
    x = (torch.randn(300, generator=torch.Generator().manual_seed(role + 3 * kind)) * 2).requires_grad_(True)
    name = "ns" if kind == 0 else "hinge"
    loss = [so.d_loss_real, so.d_loss_fake, so.g_loss][role](x, name)
    loss.backward()
    X = u.dev(x.detach())
    d = torch.empty(300, device="cuda")
    lo = torch.zeros(1, device="cuda")
    u.call("vg_gan_loss", u.ptr(X), u.ptr(d), u.ptr(lo), 300, kind, role, 1.0, u.stream())
    u.sync()
    u.assert_close(lo, loss.detach().reshape(1), 1e-5, "loss")
    u.assert_close(d, x.grad, 1e-5, "dlogits")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gan_loss_pair_is_two_single_calls(kind):
    """The fused real + fake pass evaluates both halves' losses in one launch: bit-equal to the two single launches."""
    g = torch.Generator().manual_seed(kind)
    n0, n1 = 256, 256
    x = u.dev(torch.randn(n0 + n1, generator=g) * 2)
    d1, d2 = torch.zeros_like(x), torch.zeros_like(x)
    l1, l2 = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    u.call("vg_gan_loss", u.ptr(x), u.ptr(d1), u.ptr(l1), n0, kind, 0, 1.0, u.stream())
    u.call("vg_gan_loss", C.c_void_p(x.data_ptr() + 4 * n0), C.c_void_p(d1.data_ptr() + 4 * n0), C.c_void_p(l1.data_ptr() + 4), n1, kind, 1, 1.0, u.stream())
    u.call("vg_gan_loss_pair", u.ptr(x), u.ptr(d2), u.ptr(l2), n0, 0, n1, 1, kind, 1.0, u.stream())
    u.sync()
    assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_step_begin_kernels():
    """vg_zero_tick: zero_grad + device step counter in one launch; vg_step_inputs: bf16 cast of the real batch (torch's rounding) and the
    latent batch ~ N(0, 1), counter-based on (seed, step): reproducible, fresh per step and per seed, moments of a normal sample."""
    g = torch.full((4096 + 4,), 3.0, device="cuda")
    step = torch.tensor([7], dtype=torch.int32, device="cuda")
    u.call("vg_zero_tick", u.ptr(g), 4096, u.ptr(step), u.stream())
    u.sync()
    assert bool((g[:4096] == 0).all()) and bool((g[4096:] == 3.0).all()) and int(step) == 8
    real = torch.randn(8, 3, 32, 32, device="cuda")
    imgs = torch.zeros(8, 3, 32, 32, dtype=u.BF, device="cuda")
    n = 256 * 1024
    z = [torch.zeros(n + 2, device="cuda") for _ in range(4)]
    for i, (seed, st) in enumerate(((5, 8), (5, 8), (5, 9), (6, 8))):
        step.fill_(st)
        u.call("vg_step_inputs", u.ptr(real), u.ptr(imgs), real.numel(), u.ptr(z[i]), n, seed, u.ptr(step), u.stream())
    u.sync()
    assert torch.equal(imgs, real.to(u.BF))
    assert torch.equal(z[0], z[1]) and not torch.equal(z[0], z[2]) and not torch.equal(z[0], z[3])
    for t in z:
        assert bool((t[n:] == 0).all())           # nothing written past n_z
    x = z[0][:n].double().cpu()
    m, v = float(x.mean()), float(x.var())
    sk, ku = float(((x - m) ** 3).mean() / v ** 1.5), float(((x - m) ** 4).mean() / v ** 2)
    assert abs(m) < 4 / n ** 0.5 and abs(v - 1) < 0.01 and abs(sk) < 0.02 and abs(ku - 3) < 0.04, (m, v, sk, ku)
    assert float(x.abs().max()) <= 5.78
    # neighbours (the cos / sin of one pair, consecutive pairs) and the two steps are uncorrelated
    for a, b in ((x[:-1], x[1:]), (x[:-2], x[2:]), (x, z[2][:n].double().cpu()), (x, z[3][:n].double().cpu())):
        assert abs(float((a * b).mean())) < 5 / n ** 0.5
    # tail mass like a normal's: P(|z| > 3) = 2.70e-3
    assert abs(float((x.abs() > 3).double().mean()) - 2.70e-3) < 4e-4
    # noise only / cast only
    z2 = torch.zeros(n, device="cuda")
    step.fill_(8)
    u.call("vg_step_inputs", None, None, 0, u.ptr(z2), n, 5, u.ptr(step), u.stream())
    u.sync()
    assert torch.equal(z2, z[0][:n])


def test_adamw_matches_torch():
    n = 4096 + 64
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=g)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=5e-4, weight_decay=1e-3)
    P, M_, V_ = u.dev(p0.clone()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    SH = torch.empty(n, dtype=u.BF, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(n, generator=g)
        p.grad = gr.clone()
        opt.step()
        GR = u.dev(gr * 2.0)
        u.call("vg_adamw_step", u.ptr(P), u.ptr(GR), u.ptr(M_), u.ptr(V_), u.ptr(SH), n, 5e-4, 0.9, 0.999, 1e-8, 1e-3,
               step, None, 0.5, u.stream())
        u.sync()
        u.assert_close(P, p.detach(), 1e-6, f"adamw step {step}")
        u.assert_close(SH, p.detach(), 2.0 ** -8, "bf16 shadow")


def test_grad_clip_matches_torch():
    g = torch.Generator().manual_seed(3)
    for n, max_norm, gscale in ((4096, 0.5, 1.0), (1 << 20, 5.0, 0.25), (1000 * 4, 100.0, 1.0)):
        x = torch.randn(n, generator=g) * 0.01
        p = torch.nn.Parameter(torch.zeros(n))
        p.grad = (x * gscale).clone()
        total = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        xd = u.dev(x)
        scratch = torch.zeros(1 + 1024, device="cuda")
        u.call("vg_grad_clip", u.ptr(xd), C.c_longlong(n), C.c_float(gscale), C.c_float(max_norm), u.ptr(scratch), u.stream())
        u.sync()
        assert abs(float(scratch[0]) - total) <= 5e-5 * max(total, 1.0)  # fp32 sums of up to 1M squares in a different order
        u.assert_close(xd * gscale, p.grad, 1e-4, "clipped gradient")


def test_wasserstein_loss_kind():
    x = torch.randn(37, generator=torch.Generator().manual_seed(1))
    for role, want, dw in ((0, -x.mean(), -1.0), (1, x.mean(), 1.0), (2, -x.mean(), -1.0)):
        xd, dl, lo = u.dev(x), torch.empty(37, device="cuda"), torch.empty(1, device="cuda")
        u.call("vg_gan_loss", u.ptr(xd), u.ptr(dl), u.ptr(lo), 37, 2, role, C.c_float(1.0), u.stream())
        u.sync()
        assert abs(float(lo) - float(want)) < 1e-6
        assert torch.allclose(dl.cpu(), torch.full((37,), dw / 37))


@pytest.mark.parametrize("B,D", [(8, 48), (64, 3072), (256, 100)])
def test_diversity_loss_matches_torch(B, D):
    """vg_diversity_loss vs torch.cdist(p=1) (src/v2/utils.py:147-152): loss within 1e-4 relative; gradient (added onto an
    existing bf16 gradient) within 2^-7 of max|ref|."""
    g = torch.Generator().manual_seed(B + D)
    x = torch.randn(B, D, generator=g).to(torch.bfloat16)
    d0 = (torch.randn(B, D, generator=g) * 1e-3).to(torch.bfloat16)
    xr = x.float().requires_grad_(True)
    ref = torch.cdist(xr, xr, p=1).sum() / (B * (B - 1))
    ref.backward()
    w = 0.1
    xd, dd = u.dev(x), u.dev(d0)
    lo = torch.empty(1, device="cuda")
    scratch = torch.zeros((D + 15) // 16, device="cuda")
    u.call("vg_diversity_loss", u.ptr(xd), u.ptr(dd), u.ptr(lo), u.ptr(scratch), B, D, C.c_float(w), u.stream())
    u.sync()
    assert abs(float(lo) - float(ref)) <= 1e-4 * float(ref)
    u.assert_close(dd, d0.float() + w * xr.grad, 2.0 ** -7, "d images")


def test_linear_wgrad_rejects_undersized_slab_without_launching():
    """Round-1 fault (gpurun_out/splits.log: 'Write access to a read-only page'): K slices written past a slab carved for
    fewer slices.  The public entry point now takes the slab size and refuses; nothing is launched (dW untouched)."""
    M, N, K = 512, 128, 128
    a = torch.zeros(M, N, dtype=u.BF, device="cuda"); b = torch.zeros(M, K, dtype=u.BF, device="cuda")
    dW = torch.full((N, K), 7.0, device="cuda")
    slab = torch.empty(2 * N * K, dtype=torch.float32, device="cuda")
    L = _lib_mod().lib()
    assert L.vg_linear_wgrad_slab_floats(N, K, 4) == 4 * N * K
    assert L.vg_linear_wgrad_slab_floats(N, K, 65) == -2 and L.vg_linear_wgrad_slab_floats(N, K, 0) == -2
    for splits, floats in ((4, slab.numel()), (65, 1 << 40), (0, slab.numel()), (2, 2 * N * K - 1)):
        rc = L.vg_linear_wgrad(u.ptr(a), u.ptr(b), u.ptr(dW), u.ptr(slab), floats, M, N, K, splits, 0, u.stream())
        assert rc == -2, (splits, floats, rc)
    u.sync()
    assert bool((dW == 7.0).all())


def _lib_mod():
    from vit_gan_amd import _lib
    return _lib


@pytest.mark.parametrize("B,H,S,HE", [(2, 12, 65, 64), (3, 4, 65, 96), (2, 4, 32, 96), (2, 4, 17, 32)])
def test_attention_fp8(B, H, S, HE):
    """fp8 (OCP e4m3) MFMA operands for Q.K^T and P.V (BASELINE.json configs[4]).  Two references: (a) the same math with
    the operands quantised where the kernel quantises them (e4m3 Q, K for the scores in forward AND backward recompute;
    e4m3 of 256 p and of V for P.V; every gradient-carrying product in bf16) - tight, it pins layout and scaling;
    (b) plain fp32 attention - loose: what e4m3's 3 mantissa bits cost."""
    E, scale = H * HE, 1 / math.sqrt(HE)
    f8 = torch.float8_e4m3fn
    g = torch.Generator().manual_seed(B + H + S + HE)
    qkv = u.rbf(torch.randn(B * S, 3 * E, generator=g) * 1.5)
    dO = u.rbf(torch.randn(B * S, E, generator=g))
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    q8, k8, v8 = (t.to(f8).float() for t in (q, k, v))
    s = (q8 @ k8.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = (((p * 256.0).to(f8).float() @ v8) / 256.0 / l)
    lse_ref = (m + torch.log(l)).squeeze(-1)
    o_rows = o.transpose(1, 2).reshape(B * S, E)
    QKV = u.dev(qkv, u.BF)
    O = torch.empty(B * S, E, dtype=u.BF, device="cuda")
    LSE = torch.empty(B, H, S, device="cuda")
    u.call("vg_attention_fp8_fwd", u.ptr(QKV), u.ptr(O), u.ptr(LSE), B, H, S, HE, scale, u.stream())
    u.sync()
    u.assert_close(LSE, lse_ref, 1e-4, "lse (fp8 scores)")
    # e4m3 steps are 6-12 % apart: where 256 p sits at a rounding boundary (within the ~1e-3 by which the hardware's fp8 dot
    # product and fp32 arithmetic on the quantised operands differ) one numerator moves a whole step, i.e. by up to
    # 1/8 of a large probability - a few such elements per tensor reach 2 % of max|out|; the typical row is within 0.2 %
    u.assert_close(O, o_rows, 2.0 ** -5, "attn out vs the e4m3-operand model")
    assert float((O.float().cpu() - o_rows).abs().median()) < 2e-3 * float(o_rows.abs().max())
    plain = (torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v).transpose(1, 2).reshape(B * S, E)
    err = u.assert_close(O, plain, 2.0 ** -3, "attn out vs fp32 attention")
    # backward: P from the fp8 scores and the forward's lse; gradient products in bf16 on the bf16 Q, K, V
    Ost = O.float().cpu().reshape(B, S, H, HE).transpose(1, 2)
    do = dO.reshape(B, S, H, HE).transpose(1, 2)
    pn = torch.exp(s - lse_ref.unsqueeze(-1))
    dp = do @ v.transpose(-1, -2)
    delta = (do * Ost).sum(-1, keepdim=True)
    ds = u.rbf(pn * (dp - delta) * scale)
    ref = [ds @ k, ds.transpose(-1, -2) @ q, u.rbf(pn).transpose(-1, -2) @ do]
    dQKV = torch.empty(B * S, 3 * E, dtype=u.BF, device="cuda")
    DO = u.dev(dO, u.BF)
    u.call("vg_attention_fp8_bwd", u.ptr(QKV), u.ptr(O), u.ptr(DO), u.ptr(LSE), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    for i, nm in enumerate("qkv"):
        u.assert_close(dQKV[:, i * E:(i + 1) * E], ref[i].transpose(1, 2).reshape(B * S, E), 2.0 ** -6, f"d{nm} vs the e4m3-operand model")
    print(f"fp8 attention B={B} H={H} S={S} HE={HE}: forward within {err:.3f} of max|fp32 attention|")
