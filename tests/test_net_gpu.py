"""Whole-network parity through the C ABI: vg_vit_forward/backward and vg_gen_forward/backward
against the fp32 CPU oracle on the golden-fixture parameters.

Whole networks are held to the LOOSE tier, per tensor as a fraction of max|ref|: the distance
between bf16 storage and fp32 arithmetic itself - 2^-5 logits / 2^-4 gradients for the ViT, 0.08 / 0.12 / 0.35 behind
sin(30 x) - against TWO references: the fp32 oracle pinned to the reference's outputs, and oracle/bf16_model.py, the CPU
model that rounds to bf16 exactly where the kernels store bf16.  The second one proves the looseness is inherent, not the
kernels': bf16 storage is chaotic at the ulp level, so beyond one or two blocks even the rounding-faithful model sits as
far from the kernels as fp32 does (tests/parity_tiers.py prints the table; a depth-1 network matches it to 2e-7 / 1e-3).
The TIGHT tier (2 bf16 ulps of the largest element) is therefore applied stage by stage, with each stage of the model fed
the engine's own tensors: tests/test_blocks_gpu.py.  Here the model is asserted tight only where depth allows (1 block).
"""
TIGHT = 2.0 ** -6
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _vit_case(name, batch=None):
    import gpu_util as u
    from cases import VIT_CASES
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat

    c = dict(VIT_CASES[name])
    if batch:
        c["batch"] = batch
    d = vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"],
                   layers=c["layers"], mlp_ratio=c["mlp_ratio"], classes=c["classes"])
    st_np = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    x = torch.from_numpy(make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"], "uniform"))
    return u, c, d, st_np, x


@pytest.mark.parametrize("name,batch", [("c1", None), ("c1", 5), ("c1k10", None), ("e128", None), ("c4", None), ("c5", None)])
def test_vit_forward_backward_vs_oracle(name, batch):
    u, c, d, st_np, x = _vit_case(name, batch)
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat
    from weights import make_input

    from oracle import bf16_model as bm
    B = c["batch"]
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xr = x.clone().requires_grad_(True)
    out = vo.vit_forward(st, xr, d)                      # LOOSE tier: the fp32 oracle pinned to the reference
    R = torch.from_numpy(make_input(tuple(out.shape), c["seed"] + 1))
    (out * R).sum().backward()
    st_t = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xt = x.clone().requires_grad_(True)
    out_t = bm.vit_forward(st_t, xt, d)                  # TIGHT tier: bf16 roundings where the kernels round
    (out_t * R).sum().backward()

    dd = flat.vit_dims_struct(d.channels, d.image, d.patch, d.embed, d.heads, d.layers, d.mlp_ratio, d.classes)
    lay = flat.vit_layout(dd)
    slots = flat.vit_slots(dd)
    P = flat.pack(slots, lay.total, st_np, device="cuda")
    Pb = P.to(torch.bfloat16)
    G = torch.zeros_like(P)
    net = _lib.VgVitNet(dd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), 0.0, 0, None, None)
    ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(dd), B), dtype=torch.uint8, device="cuda")
    logits = torch.empty(B, d.classes, device="cuda")
    X = x.cuda()
    u.call("vg_vit_forward", C.byref(net), B, u.ptr(X), 0, u.ptr(ws), u.ptr(logits), u.stream())
    u.sync()
    u.assert_close(logits, out_t, 2.0 ** -5, "logits vs the rounding-faithful model")
    u.assert_close(logits, out, 2.0 ** -5, "logits")
    dimg = torch.empty(B, d.channels, d.image, d.image, dtype=torch.bfloat16, device="cuda")
    Rd = R.cuda()
    u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(Rd), u.ptr(dimg), 1, u.stream())
    u.sync()
    u.assert_close(dimg, xt.grad, 2.0 ** -4, "d_img vs the rounding-faithful model")
    u.assert_close(dimg, xr.grad, 2.0 ** -4, "d_img")
    grads = {k: v.clone() for k, v in flat.unpack(slots, G).items()}
    worst = 0.0
    for k, p in st.items():
        ref = p.grad
        if float(ref.abs().max()) < 1e-6:
            # keys.bias: softmax is invariant to a key shift, the true gradient is 0; ours is bf16 rounding noise summed
            # over B*S rows - and the rounding-faithful model reproduces that noise: compare with IT, relative to the
            # sibling queries.bias gradient
            sib = float(st[k.replace("keys", "queries")].grad.abs().max())
            assert float((grads[k].cpu() - st_t[k].grad).abs().max()) < 2.0 ** -4 * sib + 1e-6, k
            assert float(grads[k].abs().max()) < 2.0 ** -4 * sib + 1e-4, k
            continue
        worst = max(worst, u.assert_close(grads[k], st_t[k].grad, 2.0 ** -4, f"grad {k} vs the rounding-faithful model"))
        u.assert_close(grads[k], ref, 2.0 ** -4, f"grad {k}")
    print(f"{name}: worst gradient distance to the rounding-faithful model {worst:.2e} of max|ref|")
    # accumulate semantics: a second backward doubles G
    u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(Rd), None, 1, u.stream())
    u.sync()
    g2 = flat.unpack(slots, G)
    for k in ("vit.encoder.0.fc1.weight", "vit.embedding.conv1.weight", "vit.norm.bias", "vit.embedding.pos_embedding"):
        u.assert_close(g2[k], 2 * grads[k], 1e-3, f"accumulate {k}")


def _dropout_masks(u, B, S, E, L, p, seed):
    """the multipliers (mask / keep) of every dropout site of a ViT run with (p, seed), through vg_dropout_apply"""
    keep = 256.0 / (256.0 - round(p * 256))

    def mask(site):
        return (u.dropout_mask((B, S, E), p, seed, site) > 0).float() * keep
    masks = {"embed": mask(0)}
    for l in range(L):
        masks[("attn", l)], masks[("mlp", l)] = mask(1 + 2 * l), mask(2 + 2 * l)
    return masks


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("Kc", [17, 40])
def test_vit_head_wider_than_16_classes_vs_oracle(Kc, B, dropout):
    """Above 16 classes (a CIFAR-100 discriminator has 100) the head's backward leaves its one-launch kernel for vg_head_bwd_dz_kernel +
    vg_head_bwd_w2_kernel, which accumulate straight into G, and db1 comes from vg_colsum_bf16.  The smallest network the layout takes
    (16 x 16 images, 4 x 4 patches, E 128, 2 blocks), forward and staged backward with want_wgrad 1 and 0, against the fp32 oracle
    computed live (with the engine's own masks at dropout 0.1), at this file's tolerances."""
    import gpu_util as u
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat
    from weights import make_input, make_state

    d = vo.VitDims(channels=3, image=16, patch=4, embed=128, heads=4, layers=2, mlp_ratio=2, classes=Kc)
    L, S, E = d.layers, d.seq, d.embed
    st_np = make_state(vo.vit_param_shapes(d), 40 + Kc, "vit")
    x = torch.from_numpy(make_input((B, 3, 16, 16), 41 + Kc, "uniform"))
    seed = 777
    masks = _dropout_masks(u, B, S, E, L, dropout, seed) if dropout > 0 else None
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    xr = x.clone().requires_grad_(True)
    out = vo.vit_forward(st, xr, d, masks=masks)
    R = torch.from_numpy(make_input(tuple(out.shape), 42 + Kc))
    (out * R).sum().backward()

    dd = flat.vit_dims_struct(3, 16, 4, E, 4, L, 2, Kc)
    lay, slots = flat.vit_layout(dd), flat.vit_slots(dd)
    P = flat.pack(slots, lay.total, st_np, device="cuda")
    Pb, X, Rd = P.to(torch.bfloat16), x.cuda(), R.cuda()
    ws = torch.empty(_lib.lib().vg_vit_ws_bytes(C.byref(dd), B), dtype=torch.uint8, device="cuda")
    for want_wgrad in (1, 0):
        G = torch.zeros_like(P)
        net = _lib.VgVitNet(dd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), dropout, seed, None, _lib.context(), 0, 0)
        logits = torch.empty(B, Kc, device="cuda")
        dimg = torch.empty(B, 3, 16, 16, dtype=torch.bfloat16, device="cuda")
        u.call("vg_vit_forward", C.byref(net), B, u.ptr(X), 0, u.ptr(ws), u.ptr(logits), u.stream())
        for stage in range(L + 2):
            u.call("vg_vit_backward_stages", C.byref(net), B, u.ptr(ws), u.ptr(Rd), u.ptr(dimg), want_wgrad, stage, stage + 1, u.stream())
        u.sync()
        what = f"want_wgrad {want_wgrad}: "
        u.assert_close(logits, out, 2.0 ** -5, what + "logits")
        u.assert_close(dimg, xr.grad, 2.0 ** -4, what + "d_img")
        if not want_wgrad:
            assert int(torch.count_nonzero(G)) == 0, "want_wgrad = 0 wrote a weight gradient"
            continue
        grads = flat.unpack(slots, G)
        for k, p in st.items():
            if k.endswith("keys.bias"):  # the exact gradient is zero (softmax is invariant to a key shift): rounding noise against its sibling
                sib = float(st[k.replace("keys", "queries")].grad.abs().max())
                assert float(grads[k].abs().max()) < 2.0 ** -4 * sib + 1e-4, k
                continue
            u.assert_close(grads[k], p.grad, 2.0 ** -4, what + f"grad {k}")


@pytest.mark.parametrize("name", ["g1", "g1b3"])
def test_gen_forward_backward_vs_oracle(name):
    import gpu_util as u
    from cases import GEN_CASES
    from weights import make_input, make_state
    from oracle import gen_oracle as go
    from vit_gan_amd import _lib, flat

    c = GEN_CASES[name]
    d = go.GenDims()
    B = c["batch"]
    st_np = make_state(go.gen_param_shapes(d), c["seed"], "gen")
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    z = torch.from_numpy(make_input((B, d.latent), c["seed"]))
    out = go.gen_forward(st, z, d)
    R = torch.from_numpy(make_input(tuple(out.shape), c["seed"] + 1)).to(torch.bfloat16).float()  # d_img is handed over in bf16
    (out * R).sum().backward()

    gd = _lib.VgGenDims(d.latent, d.tokens, d.embed, d.heads, d.layers, d.siren_hidden, d.out_features, d.omega0, 0, d.channels, d.image)
    _run_gen_vs_oracle(u, gd, d, st, st_np, z, out, R, B)


def _run_gen_vs_oracle(u, gd, d, st, st_np, z, out, R, B, pos_table=None):
    from oracle import bf16_model as bm
    from vit_gan_amd import _lib, flat
    st_t = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    out_t = bm.gen_forward(st_t, z, d, pos_table=pos_table)   # TIGHT tier
    (out_t * R).sum().backward()
    lay = flat.gen_layout(gd)
    slots = flat.gen_slots(gd)
    P = flat.pack(slots, lay.total, st_np, device="cuda")
    Pb = P.to(torch.bfloat16)
    G = torch.zeros_like(P)
    tab = None if pos_table is None else pos_table.cuda().contiguous()
    net = _lib.VgGenNet(gd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), 0.0, 0, None, None if tab is None else tab.data_ptr())
    ws = torch.empty(_lib.lib().vg_gen_ws_bytes(C.byref(gd), B), dtype=torch.uint8, device="cuda")
    img = torch.empty(B, d.channels, d.image, d.image, dtype=torch.bfloat16, device="cuda")
    Zd = z.cuda()
    u.call("vg_gen_forward", C.byref(net), B, u.ptr(Zd), u.ptr(ws), u.ptr(img), u.stream())
    u.sync()
    u.assert_close(img, out_t, 0.08, "generated image vs the rounding-faithful model")
    # sin(30 * z): a bf16 rounding of the 768-wide hidden layer moves the phase; images live in [-1, 1]
    u.assert_close(img, out, 0.08, "generated image")
    Rd = R.to(torch.bfloat16).cuda()
    u.call("vg_gen_backward", C.byref(net), B, u.ptr(ws), u.ptr(Rd), u.stream())
    u.sync()
    grads = flat.unpack(slots, G)
    rel = {}
    for k, p in st.items():
        # sin(30 z) amplifies each bf16 rounding of its input ~30x; the SLN scalars (gamma, beta) are heavily cancelling
        # sums over B*T*E random-sign products: 0.35, everything else 0.12 of max|ref| - against both references.  (The
        # scalars are held tight where that is well-defined: per operator in test_ops_gpu.py::test_sln at 3e-4, and stage
        # by stage in test_blocks_gpu.py against the 2-norm of their terms.)
        tol = 0.35 if k.endswith(("gamma", "beta")) else 0.12
        rel[k] = u.assert_close(grads[k], st_t[k].grad, tol, f"grad {k} vs the rounding-faithful model", floor=1e-4)
        u.assert_close(grads[k], p.grad, tol, f"grad {k}", floor=1e-4)
    print("largest distances to the rounding-faithful model:", [(k, f"{v:.2e}") for k, v in sorted(rel.items(), key=lambda kv: -kv[1])[:5]])


@pytest.mark.parametrize("image,patch,embed,heads,batch", [(32, 4, 384, 4, 3), (64, 8, 512, 8, 2), (128, 16, 256, 4, 1)])
def test_patch_grid_generator_vs_oracle(image, patch, embed, heads, batch):
    """the SLN/SIREN generator on the discriminator's patch grid (64 tokens, one C x P x P patch per
    token, assembled by the un-patchify scatter).  Not in the reference - the oracle defines it ("parity unpinned")."""
    import gpu_util as u
    from weights import make_input
    from oracle import gen_oracle as go
    from vit_gan_amd import _lib

    d = go.GenDims(latent=256, tokens=(image // patch) ** 2, embed=embed, heads=heads, layers=2, siren_hidden=256,
                   channels=3, image=image, patch=patch)
    st0 = go.init_gen_state(d, seed=11)
    st_np = {k: v.numpy() for k, v in st0.items()}
    st = {k: v.clone().requires_grad_(True) for k, v in st0.items()}
    z = torch.from_numpy(make_input((batch, d.latent), 5))
    out = go.gen_forward(st, z, d)
    assert out.shape == (batch, 3, image, image)
    R = torch.from_numpy(make_input(tuple(out.shape), 6)).to(torch.bfloat16).float()
    (out * R).sum().backward()
    gd = _lib.VgGenDims(d.latent, d.tokens, d.embed, d.heads, d.layers, d.siren_hidden, d.out_features, d.omega0, patch, 3, image)
    _run_gen_vs_oracle(u, gd, d, st, st_np, z, out, R, batch)


def test_patch_grid_generator_module_and_geometry_checks():
    from vit_gan_amd import _lib, flat
    from vit_gan_amd.generator import SirenGenerator
    import ctypes as C_
    G = SirenGenerator(latent=128, image_size=64, channels=3, embed=256, heads=4, layers=1, siren_hidden=128, dropout=0.0, patch_size=8).cuda()
    assert G.embedding.shape == (64, 256) and G.output_network[1].linear.weight.shape == (3 * 64, 128)
    img = G(torch.randn(2, 128, device="cuda"))
    assert img.shape == (2, 3, 64, 64) and torch.isfinite(img).all() and float(img.abs().max()) <= 1.0
    img.sum().backward()
    assert G.embedding.grad is not None and torch.isfinite(G.embedding.grad).all()
    bad = _lib.VgGenDims(128, 60, 256, 4, 1, 128, 192, 30.0, 8, 3, 64)  # 60 tokens is not the 8x8 grid
    lay = _lib.VgGenLayout()
    assert _lib.lib().vg_gen_layout(C_.byref(bad), C_.byref(lay)) != 0


@pytest.mark.parametrize("patch", [0, 4])
def test_generator_with_fourier_position_input(patch):
    """Optional Fourier positional input of the SIREN (north_star; not in the reference, the oracle defines it): module
    forward / backward against the oracle, the state_dict unchanged, product and oracle tables identical."""
    import vit_gan_amd  # noqa: F401
    import gpu_util as u
    from weights import make_input
    from oracle import gen_oracle as go
    from vit_gan_amd.generator import SirenGenerator, fourier_position_table

    T = 64 if patch else 32
    d = go.GenDims(latent=128, tokens=T, embed=256, heads=4, layers=1, siren_hidden=128, channels=3, image=32, patch=patch)
    tab = go.fourier_position_table(d)
    assert tab.shape == (T, 256) and torch.equal(tab, fourier_position_table(T, 256, 32, patch))
    G = SirenGenerator(latent=128, image_size=32, channels=3, embed=256, heads=4, layers=1, siren_hidden=128, dropout=0.0,
                       patch_size=patch, fourier_features=True)
    plain = SirenGenerator(latent=128, image_size=32, channels=3, embed=256, heads=4, layers=1, siren_hidden=128, dropout=0.0, patch_size=patch)
    assert list(G.state_dict()) == list(plain.state_dict())
    st = {k: v.detach().clone().requires_grad_(True) for k, v in G.state_dict().items()}
    G = G.cuda()
    z = torch.from_numpy(make_input((3, 128), 8))
    from oracle import bf16_model as bm
    ref = go.gen_forward(st, z, d, pos_table=tab)
    R = torch.from_numpy(make_input(tuple(ref.shape), 9)).to(torch.bfloat16).float()
    (ref * R).sum().backward()
    st_t = {k: v.detach().clone().requires_grad_(True) for k, v in st.items()}
    ref_t = bm.gen_forward(st_t, z, d, pos_table=tab)
    (ref_t * R).sum().backward()
    out = G(z.cuda())
    u.assert_close(out, ref_t, 0.08, "image vs the rounding-faithful model")
    u.assert_close(out, ref, 0.08, "image")
    no_table = go.gen_forward({k: v.detach() for k, v in st.items()}, z, d)
    assert float((ref.detach() - no_table).abs().max()) > 0.1  # the table matters
    (out * R.cuda()).sum().backward()
    got = dict(G.named_parameters())
    for k in ("output_network.0.linear.weight", "transformer_layers.0.mlp.model.0.0.weight", "embedding", "mapping_mlp.model.0.0.bias"):
        u.assert_close(got[k].grad, st_t[k].grad, 0.12, f"grad {k} vs the rounding-faithful model", floor=1e-4)
        u.assert_close(got[k].grad, st[k].grad, 0.12, f"grad {k}", floor=1e-4)


def test_v2_vitgenerator_on_hip_matches_reference_fixture():
    """the product's ``ViTGenerator`` (src/v2/modules.py:344-372) run on the HIP path against the
    reference's own outputs (tests/golden/vitgen_v2.npz, generated by importing the reference): the trunk output, the
    Linear(K, batch_size) + flat view where it is legal (batch_size^2 % 3072 == 0), and the reference's exact exception
    text where it is not."""
    import os
    import gpu_util as u
    from cases import VIT_CASES
    from weights import make_input, make_state, summarize
    from oracle import bf16_model as bm, vit_oracle as vo
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTGenerator

    c = VIT_CASES["c1k10"]
    npz = np.load(os.path.join(os.path.dirname(__file__), "golden", "vitgen_v2.npz"))
    d = vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"],
                   layers=c["layers"], mlp_ratio=c["mlp_ratio"], classes=c["classes"])
    for bs, tag in ((c["batch"], "illegal"), (96, "legal")):
        cfg = Config(attention_heads_count=c["heads"], batch_size=bs, classes_count=c["classes"], dropout_rate=0.0,
                     embeddings_dimension=c["embed"], image_size=c["image"], input_channels=c["channels"],
                     mlp_ratio=c["mlp_ratio"], patch_size=c["patch"], transformer_blocks_count=c["layers"])
        G = ViTGenerator(cfg)
        assert list(G.state_dict().keys()) == [str(s) for s in npz[f"{tag}/state_keys"]]
        st = {k: torch.from_numpy(v) for k, v in make_state(vo.vit_param_shapes(d), c["seed"], "vit").items()}
        rng = np.random.Generator(np.random.PCG64(99))
        st["linear.weight"] = torch.from_numpy((rng.standard_normal(size=(bs, c["classes"])) * 0.3).astype(np.float32))
        st["linear.bias"] = torch.from_numpy((rng.standard_normal(size=(bs,)) * 0.1).astype(np.float32))
        G.load_state_dict(st, strict=True)
        G = G.cuda().eval()
        x = torch.from_numpy(make_input((bs, c["channels"], c["image"], c["image"]), c["seed"]))
        with torch.no_grad():
            trunk = G.vit(x.cuda())
            u.assert_close(trunk, bm.vit_forward(st, x, d), 2.0 ** -5, f"{tag}: vit(x) vs the rounding-faithful model")
            u.assert_close(trunk, torch.from_numpy(npz[f"{tag}/vit_out"]), 2.0 ** -5, f"{tag}: vit(x) vs the reference's output")
            err = str(npz[f"{tag}/error"])
            if err:
                with pytest.raises(RuntimeError) as ei:
                    G(x.cuda())
                assert f"RuntimeError: {ei.value}" == err
            else:
                y = G(x.cuda())
                assert list(y.shape) == list(npz[f"{tag}/out_shape"])   # batch_size^2 / 3072 images, not batch_size
                s = summarize(y.float().cpu().numpy())
                ref_norm = float(npz[f"{tag}/out/norm"])
                assert abs(float(s["norm"]) - ref_norm) < 2.0 ** -6 * ref_norm
                scale = float(np.abs(npz[f"{tag}/out/sample"]).max())
                assert float(np.abs(s["sample"] - npz[f"{tag}/out/sample"]).max()) < 2.0 ** -5 * scale


def test_vit_with_fp8_attention_at_c5_geometry():
    """BASELINE.json configs[4]: 128x128, patch 16, E=768, 12 heads with fp8 MFMA attention.  Whole network through the
    module surface (``vit.attention_fp8 = True``) against the fp32 oracle: fp8 scores cost more than bf16 storage does -
    2^-3 of max|ref| on logits and gradients (the operator itself is pinned tightly in test_ops_gpu.py::test_attention_fp8)."""
    import gpu_util as u
    from cases import VIT_CASES
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    from vit_gan_amd.config import Config
    from vit_gan_amd.modules import ViTDiscriminator

    c = VIT_CASES["c5"]
    d = vo.VitDims(channels=3, image=128, patch=16, embed=768, heads=12, layers=c["layers"], mlp_ratio=2, classes=1)
    st_np = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    st = {k: torch.from_numpy(v).requires_grad_(True) for k, v in st_np.items()}
    x = torch.from_numpy(make_input((2, 3, 128, 128), c["seed"], "uniform"))
    out = vo.vit_forward(st, x, d)
    R = torch.from_numpy(make_input(tuple(out.shape), 3))
    (out * R).sum().backward()
    D = ViTDiscriminator(Config(embeddings_dimension=768, attention_heads_count=12, transformer_blocks_count=c["layers"], image_size=128,
                                patch_size=16, classes_count=1, dropout_rate=0.0))
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st_np.items()}, strict=True)
    D = D.cuda().eval()
    y_bf16 = D(x.cuda()).detach()
    D.vit.attention_fp8 = True
    y = D(x.cuda())
    assert not torch.equal(y.detach(), y_bf16), "the flag must change the arithmetic"
    u.assert_close(y, out, 2.0 ** -3, "logits (fp8 attention)")
    D.zero_grad()
    (y * R.cuda()).sum().backward()
    got = dict(D.named_parameters())
    for k in ("vit.encoder.0.attention.queries.weight", "vit.encoder.0.attention.values.weight", "vit.encoder.0.fc1.weight", "vit.embedding.conv1.weight"):
        u.assert_close(got[k].grad, st[k].grad, 2.0 ** -3, f"grad {k} (fp8 attention)")
