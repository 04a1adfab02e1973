"""fp32 mode, whole network (the acceptance test of the mode): vg_vit_forward_f32 / vg_vit_backward_f32 and the module surface
against the fp32 oracle and the reference's recorded numbers, at SURVEY 8d's fp32 bounds:

  logits |d| <= 1e-5 + 1e-4 |ref| elementwise;  d_img and every weight gradient |d| <= 1e-3 |ref| + 1e-5 max|ref| elementwise;
  keys.bias (true gradient 0): max|ours| <= 1e-5 max|queries.bias grad|.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("c1", None), ("c1", 5), ("c1k10", None), ("e128", None), ("c4", None), ("c5", None)]


def _case(name, batch=None):
    from cases import VIT_CASES
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    c = dict(VIT_CASES[name])
    if batch:
        c["batch"] = batch
    d = vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"],
                   layers=c["layers"], mlp_ratio=c["mlp_ratio"], classes=c["classes"])
    st_np = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    x = torch.from_numpy(make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"], "uniform"))
    return c, d, st_np, x


class F32Net:
    """The network's flat buffers and one workspace, driven through the C ABI."""

    def __init__(self, d, st_np, B, drop_p=0.0, seed=0):
        from vit_gan_amd import _lib, flat
        self.dd = flat.vit_dims_struct(d.channels, d.image, d.patch, d.embed, d.heads, d.layers, d.mlp_ratio, d.classes)
        self.slots = flat.vit_slots(self.dd)
        self.P = flat.pack(self.slots, flat.vit_layout(self.dd).total, st_np, device="cuda")
        self.Pb = self.P.to(torch.bfloat16)
        self.G = torch.zeros_like(self.P)
        self.net = _lib.VgVitNet(self.dd, self.P.data_ptr(), self.Pb.data_ptr(), self.G.data_ptr(), drop_p, seed, None, None, 0, 0)
        self.B, self.d = B, d
        self.ws = torch.empty(_lib.lib().vg_vit_ws_bytes_f32(C.byref(self.dd), B), dtype=torch.uint8, device="cuda")
        self.logits = torch.empty(B, d.classes, device="cuda")
        self.dimg = torch.empty(B, d.channels, d.image, d.image, device="cuda")

    def run(self, X, R, u):
        u.call("vg_vit_forward_f32", C.byref(self.net), self.B, u.ptr(X), u.ptr(self.ws), u.ptr(self.logits), u.stream())
        u.call("vg_vit_backward_f32", C.byref(self.net), self.B, u.ptr(self.ws), u.ptr(R), u.ptr(self.dimg), 1, u.stream())

    def grads(self):
        from vit_gan_amd import flat
        return {k: v.clone().cpu() for k, v in flat.unpack(self.slots, self.G).items()}


def _oracle(st_np, x, d, R, masks=None):
    from oracle import vit_oracle as vo
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xr = x.clone().requires_grad_(True)
    out = vo.vit_forward(st, xr, d, masks=masks)
    (out * R).sum().backward()
    return out.detach(), xr.grad, {k: p.grad for k, p in st.items()}


def _close(got, ref, what, rel=1e-3, of_max=1e-5):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    bound = rel * ref.abs() + of_max * float(ref.abs().max())
    ratio = float(((got - ref).abs() / (bound + 1e-30)).max())
    assert ratio <= 1.0, f"{what}: {ratio:.2f} x the bound (max err {float((got - ref).abs().max()):.3e}, max|ref| {float(ref.abs().max()):.3e})"
    return ratio


def _close_abs(got, ref, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    bound = 1e-5 + 1e-4 * ref.abs()
    ratio = float(((got - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{what}: {ratio:.2f} x the bound (max err {float((got - ref).abs().max()):.3e})"
    return ratio


def _check_grads(grads, dimg, ref_dx, ref_g, B=None):
    worst = {"d_img": _close(dimg, ref_dx, "d_img")}
    for k, ref in ref_g.items():
        if float(ref.abs().max()) < 1e-6:  # keys.bias: softmax is shift invariant, the true gradient is 0
            sib = float(ref_g[k.replace("keys", "queries")].abs().max())
            assert float(grads[k].abs().max()) <= 1e-5 * sib, k
            continue
        worst[k] = _close(grads[k], ref, f"grad {k}")
    return worst


def _masks(u, B, S, E, L, p, seed):
    keep = torch.tensor(256.0 / (256.0 - round(p * 256)), dtype=torch.float32)

    def mask(site):
        return (u.dropout_mask((B, S, E), p, seed, site) > 0).float() * keep

    m = {"embed": mask(0)}
    for l in range(L):
        m[("attn", l)], m[("mlp", l)] = mask(1 + 2 * l), mask(2 + 2 * l)
    return m


@pytest.mark.parametrize("name,batch", CASES)
def test_fp32_network_vs_oracle(name, batch):
    import gpu_util as u
    from weights import make_input
    c, d, st_np, x = _case(name, batch)
    B = c["batch"]
    R = torch.from_numpy(make_input((B, d.classes), c["seed"] + 1))
    out, dx, g = _oracle(st_np, x, d, R)
    n = F32Net(d, st_np, B)
    n.run(x.cuda(), R.cuda(), u)
    u.sync()
    _close_abs(n.logits, out, "logits")
    worst = _check_grads(n.grads(), n.dimg, dx, g)
    print(f"{name} B={B}: worst gradient {max(worst.values()):.3f} of the bound ({max(worst, key=worst.get)})")


def _summary_close(npz, key, arr, rtol=3e-4):  # the logic of tests/test_oracle_golden.py
    from weights import summarize
    s = summarize(arr)
    ref_norm = float(npz[f"{key}/norm"])
    assert list(s["shape"]) == list(npz[f"{key}/shape"]), key
    if ref_norm < 1e-5:
        assert float(s["norm"]) < 1e-5, key
        return
    scale = max(ref_norm / max(1.0, np.sqrt(arr.size)), 1e-12)
    np.testing.assert_allclose(float(s["norm"]), ref_norm, rtol=rtol, atol=1e-7, err_msg=key)
    np.testing.assert_allclose(s["sample"], npz[f"{key}/sample"], rtol=rtol, atol=20 * rtol * scale, err_msg=key)


@pytest.mark.parametrize("name", ["c1", "c1k10", "e128", "c4", "c5"])
def test_fp32_network_vs_reference_fixture(name):
    """Against the reference's own recorded numbers, at the bounds the oracle itself meets there."""
    import gpu_util as u
    from weights import make_input
    c, d, st_np, x = _case(name)
    npz = np.load(os.path.join(GOLD, f"vit_{name}.npz"))
    B = c["batch"]
    R = torch.from_numpy(make_input((B, d.classes), c["seed"] + 1))
    n = F32Net(d, st_np, B)
    n.run(x.cuda(), R.cuda(), u)
    u.sync()
    np.testing.assert_allclose(n.logits.cpu().numpy(), npz["out"], rtol=2e-4, atol=2e-5)
    _summary_close(npz, "dx", n.dimg.cpu().numpy())
    for k, v in n.grads().items():
        _summary_close(npz, f"grad/{k}", v.numpy())


@pytest.mark.parametrize("name", ["c1", "c4"])
def test_fp32_network_dropout_vs_oracle(name):
    """Train-mode dropout (p = 0.1): the fp32 network against the oracle fed the masks vg_dropout_apply extracts."""
    import gpu_util as u
    from weights import make_input
    c, d, st_np, x = _case(name)
    B, p, seed = c["batch"], 0.1, 987654321
    masks = _masks(u, B, d.seq, d.embed, d.layers, p, seed)
    R = torch.from_numpy(make_input((B, d.classes), c["seed"] + 1))
    out, dx, g = _oracle(st_np, x, d, R, masks)
    out0, _, _ = _oracle(st_np, x, d, R)
    assert float((out - out0).abs().max()) > 1e-3, "the masks must matter"
    n = F32Net(d, st_np, B, p, seed)
    n.run(x.cuda(), R.cuda(), u)
    u.sync()
    _close_abs(n.logits, out, "logits (dropout)")
    _check_grads(n.grads(), n.dimg, dx, g)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_fp32_network_full_size_c2(dropout):
    """C2 geometry at full size (B = 256, 6 blocks): finite, bitwise repeatable, 8 images against the oracle, and within the loose
    tier of the bf16 engine on the same weights and masks (both modes compute the same function)."""
    import gpu_util as u
    from weights import make_input
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib
    c, d, st_np, _ = _case("c1")
    B, seed = 256, 4242
    x = torch.from_numpy(make_input((B, 3, 32, 32), 77, "uniform"))
    R = torch.from_numpy(make_input((B, 1), 78))
    n = F32Net(d, st_np, B, dropout, seed)
    X, Rd = x.cuda(), R.cuda()
    n.run(X, Rd, u)
    u.sync()
    l1, dimg1, g1 = n.logits.clone(), n.dimg.clone(), n.G.clone()
    assert torch.isfinite(l1).all() and torch.isfinite(dimg1).all() and torch.isfinite(g1).all()
    n.G.zero_()
    n.run(X, Rd, u)
    u.sync()
    assert torch.equal(l1, n.logits) and torch.equal(dimg1, n.dimg) and torch.equal(g1, n.G), "two runs differ"
    # 8 images of the batch (each image is independent of the others; the masks are the batch's own)
    k = 8
    masks = None
    if dropout:
        masks = {key: v[:k] for key, v in _masks(u, B, d.seq, d.embed, d.layers, dropout, seed).items()}
    st = {kk: torch.from_numpy(v) for kk, v in st_np.items()}
    xr = x[:k].clone().requires_grad_(True)
    out = vo.vit_forward(st, xr, d, masks=masks)
    (out * R[:k]).sum().backward()
    _close_abs(l1[:k], out.detach(), "logits of 8 images")
    _close(dimg1[:k], xr.grad, "d_img of 8 images")
    # the bf16 engine on the same weights and masks: the loose tier (2^-5 of max|logit|)
    ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(n.dd), B), dtype=torch.uint8, device="cuda")
    lb = torch.empty(B, 1, device="cuda")
    u.call("vg_vit_forward", C.byref(n.net), B, u.ptr(X), 0, u.ptr(ws), u.ptr(lb), u.stream())
    u.sync()
    u.assert_close(lb, l1, 2.0 ** -5, "bf16 engine vs fp32 mode")


def test_fp32_network_graph_replay_equals_eager():
    import gpu_util as u
    from weights import make_input
    c, d, st_np, x = _case("c1", 5)
    B = 5
    R = torch.from_numpy(make_input((B, 1), 3)).cuda()
    X = x.cuda()
    n = F32Net(d, st_np, B, 0.1, 99)
    n.run(X, R, u)
    u.sync()
    ref = (n.logits.clone(), n.dimg.clone(), n.G.clone())
    n.G.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        n.run(X, R, u)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        n.G.zero_()
        n.logits.zero_()
        n.dimg.zero_()
        graph.replay()
        u.sync()
        assert torch.equal(n.logits, ref[0]) and torch.equal(n.dimg, ref[1]) and torch.equal(n.G, ref[2])


def test_fp32_module_surface():
    """ViTDiscriminator with vit.precision = "fp32": logits and every parameter's .grad against the oracle; back to "bf16" gives
    exactly what a module that never left bf16 gives."""
    import gpu_util as u
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    c, d, st_np, x = _case("c1")
    cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=6, classes_count=1, dropout_rate=0.0,
                 image_size=32, patch_size=4)
    D = ViTDiscriminator(cfg)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    D = D.cuda()
    D.vit.precision = "fp32"
    X = x.cuda().requires_grad_(True)
    y = D(X)
    y.sum().backward()
    out, dx, g = _oracle(st_np, x, d, torch.ones(x.shape[0], 1))
    _close_abs(y, out, "module logits")
    _check_grads({k: p.grad.cpu() for k, p in D.named_parameters()}, X.grad, dx, g)
    assert X.grad.dtype == torch.float32
    # a bf16 input is cast up, its gradient comes back in bf16
    Xb = x.cuda().to(torch.bfloat16).requires_grad_(True)
    D(Xb).sum().backward()
    assert Xb.grad.dtype == torch.bfloat16
    # back to bf16: bitwise what a module that never left bf16 computes
    D.vit.precision = "bf16"
    D.zero_grad()
    ref = ViTDiscriminator(cfg)
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    ref = ref.cuda()
    X1, X2 = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    y1, y2 = D(X1), ref(X2)
    y1.sum().backward()
    y2.sum().backward()
    u.sync()
    assert torch.equal(y1, y2) and torch.equal(X1.grad, X2.grad)
    for (k, p1), (_, p2) in zip(D.named_parameters(), ref.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), k
    # fp32 + fp8 attention is refused
    D.vit.precision = "fp32"
    D.vit.attention_fp8 = True
    with pytest.raises(ValueError):
        D(x.cuda())
