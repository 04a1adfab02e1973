"""The discriminator's ends around its encoder blocks - the patch embedding with block 0's LayerNorm, and its backward - through
vg_vit_forward / vg_vit_backward_stages, against the float64 restatement of tests/embed_ref.py.

Geometry 32 x 32, patch 4, E = 384, 4 heads, ONE block: the geometry the fused launches of csrc/embed.hip take.  B = 1 (a single
image), 3 (an odd batch, off the full-row path), 16 (the smallest batch on it) and 35 (no multiple of any image group: the forward's
last tile of 32 rows is partial and starts inside an image); dropout 0 and 0.1; fp32 and bf16 images.  One and four channels (K = 16 and 64) run at B = 3.
C4's geometry (patch 8, E = 512) at B = 2 keeps the unfused launches and is held to the same checks.

Tiers: X[0], d image and the four parameter gradients at 2^-6 of max|ref| (TIGHT of tests/test_blocks_gpu.py: two bf16 ulps of the
largest element; the sums over the batch against the 2-norm of their terms where that exceeds the sum).  The LayerNorm outputs are
bit-equal to vg_layernorm_fwd on the X[0] the forward produced, Apatch to the bf16 cast of the gathered image, the CLS rows of X[0] to
cls times the mask of vg_dropout_apply at site 0.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TIGHT = 2.0 ** -6
BATCHES = [1, 3, 16, 35]
ENDS = dict(image=32, patch=4, embed=384, heads=4, layers=1, mlp_ratio=2, classes=1, channels=3, seed=41)
ENDS_C1 = dict(ENDS, channels=1, seed=43)   # K = 16: one k-step, one 16-byte piece of a patch row per two threads of the staging
ENDS_C4 = dict(ENDS, channels=4, seed=44)   # K = 64: the widest the fused launches take, both k-steps full
C4 = dict(image=64, patch=8, embed=512, heads=8, layers=1, mlp_ratio=2, classes=1, channels=3, seed=42)
SEED = 977
FOLD_ADDS = 32  # the most partial sums a call folds into one gradient element: EMB_SPLIT_CAP K slices (csrc/engine.hip)
EMB_KEYS = {"d_w": "vit.embedding.conv1.weight", "d_b": "vit.embedding.conv1.bias", "d_pos": "vit.embedding.pos_embedding",
            "d_cls": "vit.embedding.cls_token"}


def _view(ws, off, shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return ws[off:off + n].view(dtype).view(*shape)


@functools.lru_cache(maxsize=None)
def _run(geom, B, dropout, img_bf16):
    """one forward and one staged backward of the one-block network; everything the tests look at, on the CPU, computed once"""
    import gpu_util as u
    import embed_ref as er
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    from vit_gan_amd import _lib, flat

    c = {"ends": ENDS, "ends_c1": ENDS_C1, "ends_c4": ENDS_C4, "c4": C4}[geom]
    d = vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"], layers=c["layers"],
                   mlp_ratio=c["mlp_ratio"], classes=c["classes"])
    L, S, E, NP, P_, Cn, IH = d.layers, d.seq, d.embed, d.seq - 1, d.patch, d.channels, d.image
    K, M = Cn * P_ * P_, B * S
    st = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    x = torch.from_numpy(make_input((B, Cn, IH, IH), c["seed"] + B, "uniform"))
    if img_bf16:
        x = x.to(torch.bfloat16)
    dd = flat.vit_dims_struct(Cn, IH, P_, E, d.heads, L, d.mlp_ratio, d.classes)
    lay, slots = flat.vit_layout(dd), flat.vit_slots(dd)
    Pm = flat.pack(slots, lay.total, st, device="cuda")
    Pb, G = Pm.to(torch.bfloat16), torch.zeros_like(Pm)
    net = _lib.VgVitNet(dd, Pm.data_ptr(), Pb.data_ptr(), G.data_ptr(), dropout, SEED, None, None, 0, 0)
    wm = _lib.VgVitWsMap()
    u.call("vg_vit_ws_map", C.byref(dd), B, C.byref(wm))
    ws = torch.zeros(_lib.lib().vg_vit_ws_bytes(C.byref(dd), B), dtype=torch.uint8, device="cuda")
    logits = torch.empty(B, d.classes, device="cuda")
    X = x.cuda()
    u.call("vg_vit_forward", C.byref(net), B, u.ptr(X), 1 if img_bf16 else 0, u.ptr(ws), u.ptr(logits), u.stream())
    u.sync()
    out = {"d": d, "B": B}
    x0 = _view(ws, wm.X, (M, E), torch.bfloat16)
    out["x0"] = x0.cpu().clone()
    out["xn1"] = _view(ws, wm.xn1, (M, E), torch.bfloat16).cpu().clone()
    out["mean1"] = _view(ws, wm.mean1, (M,), torch.float32).cpu().clone()
    out["rstd1"] = _view(ws, wm.rstd1, (M,), torch.float32).cpu().clone()
    out["apatch"] = _view(ws, 0, (B, NP, K), torch.bfloat16).cpu().clone()  # the first tensor of the workspace carve
    # vg_layernorm_fwd on the X[0] the forward produced
    g1, b1 = (torch.from_numpy(st[f"vit.encoder.0.norm1.{n}"]).cuda() for n in ("weight", "bias"))
    y, mu, rs = torch.empty(M, E, dtype=torch.bfloat16, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    u.call("vg_layernorm_fwd", u.ptr(x0), E, u.ptr(g1), u.ptr(b1), u.ptr(y), E, u.ptr(mu), u.ptr(rs), M, E, 1e-5, u.stream())
    u.sync()
    out["ln"] = (y.cpu(), mu.cpu(), rs.cpu())
    mask = None
    if dropout > 0:
        mo = u.dropout_mask((B, S, E), dropout, SEED, 0)
        thr = round(dropout * 256)
        keep = torch.tensor(256.0, dtype=torch.float32) / torch.tensor(256.0 - thr, dtype=torch.float32)  # the kernels' fp32 scale
        mask = (mo > 0).float() * keep
    out["mask"] = mask
    # backward: the head and the block, then the embedding stage on its own - twice, then without weight gradients, then into a fresh buffer
    R = torch.from_numpy(make_input((B, d.classes), c["seed"] + 1)).cuda()
    dimg = torch.full((B, Cn, IH, IH), float("nan"), dtype=torch.bfloat16, device="cuda")

    def stage(net_, a, b, want, di):
        u.call("vg_vit_backward_stages", C.byref(net_), B, u.ptr(ws), u.ptr(R), u.ptr(di), want, a, b, u.stream())
        u.sync()
    for s in range(L + 1):
        stage(net, s, s + 1, 1, dimg)
    out["gin"] = _view(ws, wm.gin[1], (B, S, E), torch.bfloat16).cpu().clone()  # dL/dX[0]: block 0 wrote it into the other set
    g_before = G.clone()
    stage(net, L + 1, L + 2, 1, dimg)
    out["touched_only_embedding"] = bool(torch.equal(G[lay.layer0:], g_before[lay.layer0:]))
    out["g1"] = {k: v.cpu().clone() for k, v in flat.unpack(slots, G).items() if k.startswith("vit.embedding.")}
    out["dimg"] = dimg.cpu().clone()
    dimg2 = torch.full_like(dimg, float("nan"))
    stage(net, L + 1, L + 2, 1, dimg2)
    out["g2"] = {k: v.cpu().clone() for k, v in flat.unpack(slots, G).items() if k.startswith("vit.embedding.")}
    out["dimg2"] = dimg2.cpu().clone()
    g_keep = G.clone()
    dimg3 = torch.full_like(dimg, float("nan"))
    stage(net, L + 1, L + 2, 0, dimg3)
    out["no_wgrad_untouched"] = bool(torch.equal(G, g_keep))
    out["dimg3"] = dimg3.cpu().clone()
    Gf = torch.zeros_like(Pm)
    netf = _lib.VgVitNet(dd, Pm.data_ptr(), Pb.data_ptr(), Gf.data_ptr(), dropout, SEED, None, None, 0, 0)
    stage(netf, L + 1, L + 2, 1, None)
    out["gf"] = {k: v.cpu().clone() for k, v in flat.unpack(slots, Gf).items() if k.startswith("vit.embedding.")}
    # float64 reference
    t = {k: torch.from_numpy(v) for k, v in st.items()}
    fw = er.embed_fwd(x.float(), t["vit.embedding.conv1.weight"], t["vit.embedding.conv1.bias"], t["vit.embedding.pos_embedding"],
                      t["vit.embedding.cls_token"], P_, mask)
    out["ref_fwd"] = fw
    out["ref_bwd"] = er.embed_bwd(out["gin"], fw["apatch"], t["vit.embedding.conv1.weight"], Cn, IH, P_, mask)
    out["cls"] = t["vit.embedding.cls_token"].reshape(E)
    return out


CASES = [(B, p, bf) for B in BATCHES for p in (0.0, 0.1) for bf in (False, True)]


def _check_forward(r):
    import embed_ref as er
    from exact_util import BF, assert_bitwise, rne
    d, B = r["d"], r["B"]
    S, E = d.seq, d.embed
    # Apatch: the bf16 cast of the gathered image
    assert_bitwise(r["apatch"], rne(r["ref_fwd"]["apatch"], BF), "Apatch")
    # X[0]
    e = er.tier_err(r["x0"].reshape(B, S, E), r["ref_fwd"]["x"], TIGHT)
    print(f"X[0]: {e:.3e} of the 2^-6 tier")
    assert e <= 1.0, f"embedding: X[0] at {e:.3f} x the 2^-6 tier"
    # CLS rows: cls times the mask, in the kernels' fp32, one rounding
    cls = r["cls"].float().expand(B, E)
    want = cls if r["mask"] is None else cls * r["mask"][:, 0]
    assert_bitwise(r["x0"].reshape(B, S, E)[:, 0].contiguous(), want.to(torch.bfloat16).contiguous(), "CLS rows of X[0]")
    # LayerNorm: bit-equal to vg_layernorm_fwd on the X[0] the forward produced
    y, mu, rs = r["ln"]
    assert_bitwise(r["xn1"], y, "xn1[0] vs vg_layernorm_fwd(X[0])")
    assert_bitwise(r["mean1"], mu, "mean1[0] vs vg_layernorm_fwd(X[0])")
    assert_bitwise(r["rstd1"], rs, "rstd1[0] vs vg_layernorm_fwd(X[0])")


def _check_backward(r):
    import embed_ref as er
    ref = r["ref_bwd"]
    e = er.tier_err(r["dimg"], ref["d_img"], TIGHT)
    print(f"d image: {e:.3e} of the 2^-6 tier")
    assert e <= 1.0, f"embedding: d image at {e:.3f} x the 2^-6 tier"
    for name, key in EMB_KEYS.items():
        got = r["g1"][key]
        e = er.tier_err(got, ref[name].reshape(got.shape), TIGHT, ref["nrm_" + name[2:]].reshape(got.shape))
        print(f"{key}: {e:.3e} of the 2^-6 tier")
        assert e <= 1.0, f"embedding: grad {key} at {e:.3f} x the 2^-6 tier"
    assert r["touched_only_embedding"], "the embedding stage wrote gradients outside the embedding's parameters"


def _check_repeats(r):
    from exact_util import assert_bitwise
    for name, key in EMB_KEYS.items():
        a, b = r["g1"][key].double(), r["g2"][key].double()
        # A call adds n <= FOLD_ADDS partial sums s_i to the gradient one after the other (the K slices of d conv_w; one sum for the
        # others).  The first call leaves G1 = sum s_i + e1 with |e1| <= (n - 1) u Mag, u = 2^-24 and Mag = sum |s_i| <= mag, the sum of the
        # absolute values of the terms; the second G2 = G1 + sum s_i + e2 with |e2| <= n u (|G1| + Mag).  So |G2 - 2 G1| = |e2 - e1| <=
        # 2 n u (|G1| + mag): the roundings of the accumulating adds and nothing else.
        mag = r["ref_bwd"]["mag_" + name[2:]].reshape(a.shape)
        lim = 2 * FOLD_ADDS * 2.0 ** -24 * (a.abs() + mag)
        assert bool(((b - 2 * a).abs() <= lim).all()), f"{key}: two calls are not twice one call"
        assert_bitwise(r["gf"][key], r["g1"][key], f"{key}: a second network into a fresh gradient buffer")
    assert_bitwise(r["dimg2"], r["dimg"], "d image of two identical calls")
    assert r["no_wgrad_untouched"], "want_wgrad = 0 wrote to the gradient buffer"
    assert_bitwise(r["dimg3"], r["dimg"], "d image with and without weight gradients")


@pytest.mark.parametrize("B,dropout,img_bf16", CASES)
def test_forward_end(B, dropout, img_bf16):
    _check_forward(_run("ends", B, dropout, img_bf16))


@pytest.mark.parametrize("B,dropout,img_bf16", CASES)
def test_backward_end(B, dropout, img_bf16):
    _check_backward(_run("ends", B, dropout, img_bf16))


@pytest.mark.parametrize("B,dropout,img_bf16", CASES)
def test_backward_end_accumulates_and_repeats(B, dropout, img_bf16):
    _check_repeats(_run("ends", B, dropout, img_bf16))


@pytest.mark.parametrize("geom", ["ends_c1", "ends_c4"])
def test_other_channel_counts(geom):
    """the fused launches are instantiated for 1 to 4 channels (K = 16 C): the narrowest and the widest, every check of the three-channel
    cases, at an odd batch with dropout on"""
    r = _run(geom, 3, 0.1, False)
    _check_forward(r)
    _check_backward(r)
    _check_repeats(r)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_c4_geometry_keeps_its_values(dropout):
    """patch 8, E = 512: outside the fused launches' geometry.  The same checks - values against the float64 reference at the tier, the
    LayerNorm outputs against vg_layernorm_fwd bit for bit - on the launches it keeps.  They hold that geometry to what is asked of it; they
    cannot tell which launches ran, and they do not pin the earlier bytes."""
    r = _run("c4", 2, dropout, False)
    _check_forward(r)
    _check_backward(r)
    _check_repeats(r)
