"""Whole networks at 81 to 256 tokens: the ViT through vg_vit_forward / _backward against the fp32 oracle and the rounding-faithful
bf16 model (the LOOSE whole-network tier of test_net_gpu.py: 2^-5 logits, 2^-4 gradients), the pruned top block against the dense
one, the module against composed_forward, the patch-grid generator and a GanEngine step against their oracles, graph replay
against eager."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# (image, patch, embed, heads): S = 197, 145, 226
GEOMETRIES = [(224, 16, 768, 12), (48, 4, 384, 4), (60, 4, 128, 4)]


@pytest.mark.parametrize("image,patch,embed,heads", GEOMETRIES)
def test_long_vit_forward_backward_vs_oracle(image, patch, embed, heads):
    import gpu_util as u
    from weights import make_input, make_state
    from oracle import bf16_model as bm
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat

    B, seed = 2, 11
    d = vo.VitDims(channels=3, image=image, patch=patch, embed=embed, heads=heads, layers=2, mlp_ratio=2, classes=1)
    st_np = make_state(vo.vit_param_shapes(d), seed, "vit")
    x = torch.from_numpy(make_input((B, 3, image, image), seed, "uniform"))
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xr = x.clone().requires_grad_(True)
    out = vo.vit_forward(st, xr, d)
    R = torch.from_numpy(make_input(tuple(out.shape), seed + 1))
    (out * R).sum().backward()
    st_t = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xt = x.clone().requires_grad_(True)
    out_t = bm.vit_forward(st_t, xt, d)
    (out_t * R).sum().backward()

    dd = flat.vit_dims_struct(3, image, patch, embed, heads, 2, 2, 1)
    lay = flat.vit_layout(dd)
    slots = flat.vit_slots(dd)
    P = flat.pack(slots, lay.total, st_np, device="cuda")
    Pb = P.to(torch.bfloat16)
    G = torch.zeros_like(P)
    net = _lib.VgVitNet(dd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), 0.0, 0, None, None)
    ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(dd), B), dtype=torch.uint8, device="cuda")
    logits = torch.empty(B, 1, device="cuda")
    u.call("vg_vit_forward", C.byref(net), B, u.ptr(x.cuda()), 0, u.ptr(ws), u.ptr(logits), u.stream())
    u.sync()
    u.assert_close(logits, out_t, 2.0 ** -5, "logits vs the rounding-faithful model")
    u.assert_close(logits, out, 2.0 ** -5, "logits")
    dimg = torch.empty(B, 3, image, image, dtype=torch.bfloat16, device="cuda")
    u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(R.cuda()), u.ptr(dimg), 1, u.stream())
    u.sync()
    u.assert_close(dimg, xt.grad, 2.0 ** -4, "d_img vs the rounding-faithful model")
    u.assert_close(dimg, xr.grad, 2.0 ** -4, "d_img")
    grads = flat.unpack(slots, G)
    for k, p in st.items():
        ref = p.grad
        if float(ref.abs().max()) < 1e-6:  # keys.bias: the true gradient is 0 (softmax is shift-invariant); see test_net_gpu.py
            sib = float(st[k.replace("keys", "queries")].grad.abs().max())
            assert float(grads[k].abs().max()) < 2.0 ** -4 * sib + 1e-4, k
            continue
        u.assert_close(grads[k], st_t[k].grad, 2.0 ** -4, f"grad {k} vs the rounding-faithful model")
        u.assert_close(grads[k], ref, 2.0 ** -4, f"grad {k}")


def _long_d(dropout=0.0, layers=2):
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(3)
    return ViTDiscriminator(Config(image_size=224, patch_size=16, embeddings_dimension=768, attention_heads_count=12,
                                   transformer_blocks_count=layers, dropout_rate=dropout, classes_count=1)).cuda()


def test_pruned_top_block_equals_dense_with_dropout_at_197_tokens():
    """The top block's CLS-query attention (256-key CLS kernels) against the dense top block (the long full kernels), dropout on:
    same logits and gradients (the dense one computes rows the classifier never reads)."""
    import gpu_util as u
    from weights import make_state
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat
    B = 4
    d = vo.VitDims(channels=3, image=224, patch=16, embed=768, heads=12, layers=2, mlp_ratio=2, classes=1)
    dd = flat.vit_dims_struct(3, 224, 16, 768, 12, 2, 2, 1)
    slots = flat.vit_slots(dd)
    P = flat.pack(slots, flat.vit_layout(dd).total, make_state(vo.vit_param_shapes(d), 21, "vit"), device="cuda")
    Pb = P.to(torch.bfloat16)
    x = (torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    dl = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).cuda()
    res = {}
    for dense in (0, 1):
        G = torch.zeros_like(P)
        net = _lib.VgVitNet(dd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), 0.1, 1234, None, None, 0, dense)
        ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(dd), B), dtype=torch.uint8, device="cuda")
        logits = torch.empty(B, 1, device="cuda")
        u.call("vg_vit_forward", C.byref(net), B, u.ptr(x), 0, u.ptr(ws), u.ptr(logits), u.stream())
        u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(dl), None, 1, u.stream())
        u.sync()
        res[dense] = (logits.clone(), G)
    u.assert_close(res[0][0], res[1][0], 2.0 ** -6, "logits: pruned vs dense top block")
    u.assert_close(res[0][1], res[1][1], 2.0 ** -5, "gradients: pruned vs dense top block")


def test_module_forward_backward_equals_composed_forward_at_197_tokens():
    D = _long_d()
    D.eval()
    x = (torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda()
    import gpu_util as u
    D.zero_grad()
    out = D(x)
    out.sum().backward()
    g_fused = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
    D.zero_grad()
    out_c = D.vit.composed_forward(x)
    out_c.sum().backward()
    u.assert_close(out, out_c, 2.0 ** -5, "fused vs composed logits")
    params = dict(D.named_parameters())
    for k, p in params.items():
        if "keys.bias" in k:  # the true gradient is 0 (softmax is shift-invariant): both paths give rounding noise
            sib = float(params[k.replace("keys", "queries")].grad.abs().max())
            assert float((g_fused[k] - p.grad).abs().max()) < 2.0 ** -4 * sib + 1e-4, k
            continue
        u.assert_close(g_fused[k], p.grad, 2.0 ** -4, f"fused vs composed grad {k}")


def test_patch_grid_generator_and_engine_step_at_48_over_4():
    """GanEngine at 48/4 (145-token discriminator, 144-token patch-grid generator), E = 384: one step against the fp32 step
    oracle; then graph replay against eager, bitwise, with dropout on."""
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo

    B = 4
    torch.manual_seed(5)
    cfg = Config(embeddings_dimension=384, attention_heads_count=4, transformer_blocks_count=2, image_size=48, patch_size=4,
                 classes_count=1, dropout_rate=0.0, batch_size=B)
    D = ViTDiscriminator(cfg)
    G = SirenGenerator(latent=256, image_size=48, channels=3, embed=384, heads=4, layers=2, siren_hidden=256, dropout=0.0, patch_size=4)
    ddims = vo.VitDims(image=48, patch=4, embed=384, heads=4, layers=2, classes=1)
    gdims = go.GenDims(latent=256, tokens=144, embed=384, heads=4, layers=2, siren_hidden=256, image=48, patch=4)
    oracle = so.GanStepOracle({k: v.detach().clone() for k, v in D.state_dict().items()},
                              {k: v.detach().clone() for k, v in G.state_dict().items()}, ddims, gdims)
    sd_d = {k: v.detach().clone() for k, v in D.state_dict().items()}
    sd_g = {k: v.detach().clone() for k, v in G.state_dict().items()}
    eng = GanEngine(D.cuda(), G.cuda(), batch=B)
    real = torch.rand(B, 3, 48, 48, generator=torch.Generator().manual_seed(0)) * 2 - 1
    losses = eng.step(real.cuda())
    torch.cuda.synchronize()
    ref = oracle.step(real, eng.z.detach().cpu().clone())
    got = losses.cpu().tolist()
    assert abs(got[0] - ref["d_real"]) < 2e-2 and abs(got[1] - ref["d_fake"]) < 2e-2 and abs(got[2] - ref["g"]) < 2e-2, (got, ref)

    # graph replay == eager, bitwise, dropout on in both networks
    runs = {}
    for use_graph in (False, True):
        D2 = ViTDiscriminator(cfg)
        G2 = SirenGenerator(latent=256, image_size=48, channels=3, embed=384, heads=4, layers=2, siren_hidden=256, dropout=0.0,
                            patch_size=4)
        D2.load_state_dict(sd_d)
        G2.load_state_dict(sd_g)
        e = GanEngine(D2.cuda(), G2.cuda(), batch=B, d_dropout=0.1, g_dropout=0.2, seed=9, use_graph=use_graph)
        ls = [e.step(real.cuda()).clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs[use_graph] = (torch.stack(ls).cpu(), e.vit._flat.flat.detach().clone(), e.gen._flat.flat.detach().clone())
    assert torch.isfinite(runs[False][0]).all()
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b), "graph replay differs from eager"
