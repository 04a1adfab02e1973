"""The attention operators at 81 to 256 tokens (csrc/attention_long.hip through vg_attention_fwd / _bwd, and the CLS-query kernels
raised to 256 keys) against fp32 PyTorch on bf16-rounded inputs, with the tolerances of test_ops_gpu.py::test_attention."""
import math

import pytest
import torch

import gpu_util as u

pytestmark = pytest.mark.gpu


def _case(B, H, S, HE, seed):
    E = H * HE
    g = torch.Generator().manual_seed(seed)
    qkv = u.rbf(torch.randn(B * S, 3 * E, generator=g) * 1.5).requires_grad_(True)
    dO = u.rbf(torch.randn(B * S, E, generator=g))
    return qkv, dO


def _ref(qkv, B, H, S, HE, scale):
    E = H * HE
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    sc = (q @ k.transpose(-1, -2)) * scale
    o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, E)
    return o, torch.logsumexp(sc, -1)


def _run(QKV, DO, B, H, S, HE, scale):
    E = H * HE
    O = torch.empty(B * S, E, dtype=u.BF, device="cuda")
    LSE = torch.empty(B, H, S, device="cuda")
    u.call("vg_attention_fwd", u.ptr(QKV), u.ptr(O), u.ptr(LSE), B, H, S, HE, scale, u.stream())
    dQKV = torch.full((B * S, 3 * E), 7.0, dtype=u.BF, device="cuda")  # every element must be written
    u.call("vg_attention_bwd", u.ptr(QKV), u.ptr(O), u.ptr(DO), u.ptr(LSE), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    return O, LSE, dQKV


@pytest.mark.parametrize("S", [81, 96, 145, 197, 226, 256])
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_long_attention_vs_fp32(S, HE):
    _check(2, 3, S, HE, 1 / math.sqrt(HE))


def test_long_attention_generator_scale():
    """The v1 generator's scale 1/sqrt(H * HE) (a flatter softmax) at 256 rows."""
    _check(2, 4, 256, 32, 1 / math.sqrt(4 * 32))


def _check(B, H, S, HE, scale):
    E = H * HE
    qkv, dO = _case(B, H, S, HE, B + H + S + HE)
    o, lse_ref = _ref(qkv, B, H, S, HE, scale)
    QKV, DO = u.dev(qkv.detach(), u.BF), u.dev(dO, u.BF)
    O, LSE, dQKV = _run(QKV, DO, B, H, S, HE, scale)
    u.assert_close(LSE, lse_ref, 1e-4, "lse")
    u.assert_close(O, o, 2.0 ** -6, "attn out")
    o.backward(dO)
    for i, nm in enumerate("qkv"):
        u.assert_close(dQKV[:, i * E:(i + 1) * E], qkv.grad[:, i * E:(i + 1) * E], 2.0 ** -5, f"d{nm}")
    # bitwise determinism: a second backward (and forward) reproduces every bit
    O2, LSE2, dQKV2 = _run(QKV, DO, B, H, S, HE, scale)
    assert torch.equal(O2, O) and torch.equal(LSE2, LSE) and torch.equal(dQKV2, dQKV)


def test_long_attention_full_size():
    """The fused real + fake batch of the ViT-B/16 geometry: B = 512, H = 12, S = 197, HE = 64.  Finite everywhere; sampled heads
    of sampled images against fp32."""
    B, H, S, HE = 512, 12, 197, 64
    E, scale = H * HE, 1 / math.sqrt(HE)
    g = torch.Generator().manual_seed(5)
    QKV = (torch.randn(B * S, 3 * E, generator=g) * 1.5).to(u.BF).cuda()
    DO = torch.randn(B * S, E, generator=g).to(u.BF).cuda()
    O, LSE, dQKV = _run(QKV, DO, B, H, S, HE, scale)
    assert bool(torch.isfinite(O.float()).all()) and bool(torch.isfinite(LSE).all()) and bool(torch.isfinite(dQKV.float()).all())
    imgs = [0, 7, 255, 511]
    rows = torch.cat([torch.arange(b * S, (b + 1) * S) for b in imgs])
    qkv = QKV[rows.cuda()].float().cpu().requires_grad_(True)
    Bs = len(imgs)
    o, lse_ref = _ref(qkv, Bs, H, S, HE, scale)
    u.assert_close(LSE[imgs], lse_ref, 1e-4, "lse (sampled images)")
    u.assert_close(O[rows.cuda()], o, 2.0 ** -6, "attn out (sampled images)")
    o.backward(DO[rows.cuda()].float().cpu())
    d = dQKV[rows.cuda()]
    for i, nm in enumerate("qkv"):
        for h in (0, 5, 11):
            cols = slice(i * E + h * HE, i * E + (h + 1) * HE)
            u.assert_close(d[:, cols], qkv.grad[:, cols], 2.0 ** -5, f"d{nm} head {h}")


@pytest.mark.parametrize("S,HE", [(197, 64), (256, 96), (145, 32)])
def test_cls_query_long(S, HE):
    """The CLS-query kernels with 256 keys: against fp32 attention, and against row 0 of the full (long) kernels."""
    B, H = 3, 4
    E, scale = H * HE, 1 / math.sqrt(HE)
    g = torch.Generator().manual_seed(S + HE)
    qkv = u.rbf(torch.randn(B * S, 3 * E, generator=g) * 1.5).requires_grad_(True)
    dO0 = u.rbf(torch.randn(B, E, generator=g))
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, S, H, HE).transpose(1, 2) for i in range(3))
    sc = (q[:, :, :1] @ k.transpose(-1, -2)) * scale
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
    assert bool((dQKV[:, :E].reshape(B, S, E)[:, 1:] == 0).all()), "dQ must be exactly zero off the CLS rows"
    # row 0 of the full kernels, d_out zero on every other row (online softmax: p is rounded against a running max, so the
    # agreement is the output tier, not bitwise)
    DO = torch.zeros(B, S, E, dtype=u.BF, device="cuda")
    DO[:, 0] = DOc
    O, LSE, dFull = _run(QKV, DO.reshape(B * S, E), B, H, S, HE, scale)
    u.assert_close(Oc, O.reshape(B, S, E)[:, 0].float().cpu(), 2.0 ** -6, "forward vs the full kernel's row 0")
    u.assert_close(Lc, LSE[:, :, 0].cpu(), 1e-5, "lse vs the full kernel's")
    for i, nm in enumerate("qkv"):
        u.assert_close(dQKV[:, i * E:(i + 1) * E], dFull[:, i * E:(i + 1) * E].float().cpu(), 2.0 ** -5, f"d{nm} vs the full kernel")
