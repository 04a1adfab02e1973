"""fp32 mode of the generator, whole network (the acceptance test of the mode): vg_gen_forward_f32 / vg_gen_backward_f32 and the module
surface against gen_oracle.gen_forward in float32 and the reference's recorded numbers, at the discriminator mode's bounds:

  image |d| <= 1e-5 + 1e-4 |ref| elementwise;  every gradient |d| <= 1e-3 |ref| + 1e-5 max|ref| elementwise;  nothing skipped.

tests/test_gen_fp32_cpu.py::test_bounds_are_admissible shows the float32 oracle itself within 0.21 / 0.13 of them against float64.
The cases and their oracle runs are tests/gen_f32_ref.py's, computed once."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gen_f32_ref as gr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _dims(d):
    from vit_gan_amd import _lib
    return _lib.VgGenDims(d.latent, d.tokens, d.embed, d.heads, d.layers, d.siren_hidden, d.out_features, d.omega0, d.patch, d.channels, d.image)


class F32Gen:
    """The generator's flat buffers and one workspace, driven through the C ABI."""

    def __init__(self, name):
        from vit_gan_amd import _lib, flat
        c = self.c = gr.case(name)
        d = c["d"]
        self.gd = _dims(d)
        self.slots = flat.gen_slots(self.gd)
        self.P = flat.pack(self.slots, flat.gen_layout(self.gd).total, c["st_np"], device="cuda")
        self.G = torch.zeros_like(self.P)
        self.tab = None if c["pos_table"] is None else c["pos_table"].cuda().contiguous()
        # Pb = NULL: the fp32 calls never read the bf16 shadow
        self.net = _lib.VgGenNet(self.gd, self.P.data_ptr(), None, self.G.data_ptr(), c["dropout"], c["drop_seed"], None,
                                 None if self.tab is None else self.tab.data_ptr())
        self.cond = None
        if c["K"]:
            self.labels, self.table = c["labels"].cuda(), c["table"].cuda().contiguous()
            self.table_grad = torch.zeros_like(self.table)
            self.cond = _lib.VgGenCondF32(self.labels.data_ptr(), self.table.data_ptr(), self.table_grad.data_ptr(), c["K"])
        self.B = c["B"]
        self.ws = torch.empty(_lib.lib().vg_gen_ws_bytes_f32(C.byref(self.gd), self.B), dtype=torch.uint8, device="cuda")
        self.img = torch.empty(self.B, d.channels, d.image, d.image, device="cuda")
        self.z, self.R = c["z"].cuda(), c["R"].cuda()

    def run(self, u):
        cond = None if self.cond is None else C.byref(self.cond)
        u.call("vg_gen_forward_f32", C.byref(self.net), self.B, u.ptr(self.z), u.ptr(self.ws), u.ptr(self.img), cond, u.stream())
        u.call("vg_gen_backward_f32", C.byref(self.net), self.B, u.ptr(self.ws), u.ptr(self.R), cond, u.stream())
        u.sync()

    def grads(self):
        from vit_gan_amd import flat
        g = {k: v.clone().cpu() for k, v in flat.unpack(self.slots, self.G).items()}
        if self.cond is not None:
            g[gr.CLASS_KEY] = self.table_grad.clone().cpu()
        return g


def _check(img, grads, ref_img, ref_g, what):
    ri = gr.image_ratio(img, ref_img)
    assert ri <= 1.0, f"{what}: image {ri:.2f} x the bound (max err {float((img.cpu() - ref_img).abs().max()):.3e})"
    assert set(grads) == set(ref_g), set(grads) ^ set(ref_g)
    worst = {k: gr.grad_ratio(grads[k], ref_g[k]) for k in ref_g}
    top = max(worst, key=worst.get)
    print(f"{what}: image {ri:.3f} of its bound, worst gradient {worst[top]:.3f} ({top})")
    for k, r in worst.items():
        assert r <= 1.0, f"{what}: grad {k} {r:.2f} x the bound"
    return ri, worst


@pytest.mark.parametrize("name", ["g1", "g1b3", "p32", "p64", "fourier", "cond"])
def test_fp32_generator_vs_oracle(name):
    import gpu_util as u
    n = F32Gen(name)
    n.run(u)
    img1, G1 = n.img.clone(), n.G.clone()
    ref_img, ref_g = gr.oracle_f32(name)
    _check(n.img, n.grads(), ref_img, ref_g, name)
    if name == "cond":  # the absent class keeps a zero row, every present class has a gradient
        tg = n.table_grad.cpu()
        assert float(tg[1].abs().max()) == 0.0 and float(tg[0].abs().max()) > 0.0 and float(tg[2].abs().max()) > 0.0
    # a second run from zeroed gradients is bit-equal
    n.G.zero_()
    if n.cond is not None:
        n.table_grad.zero_()
    n.img.zero_()
    n.run(u)
    assert torch.equal(n.img, img1) and torch.equal(n.G, G1), "two runs differ"


def test_fp32_generator_dropout_vs_oracle():
    """dropout 0.2 at the generator's sites: the masks vg_dropout_apply extracts (gpu_util.dropout_mask) are the definition's
    (drop_ref), and the fp32 generator matches the oracle fed them - one seed draws the same masks in both modes."""
    import gpu_util as u
    c = gr.case("drop")
    d, B = c["d"], c["B"]
    keep = torch.tensor(256.0 / (256.0 - round(c["dropout"] * 256)), dtype=torch.float32)
    host = gr.host_masks("drop")
    for key, site in gr.drop_sites(d):
        dev = (u.dropout_mask((B, d.tokens, d.embed), c["dropout"], c["drop_seed"], site) > 0).float() * keep
        assert torch.equal(dev, host[key]), (key, site)
    n = F32Gen("drop")
    n.run(u)
    ref_img, ref_g = gr.oracle_f32("drop")
    _check(n.img, n.grads(), ref_img, ref_g, "drop")
    img0, _ = gr.oracle_run("drop", torch.float32, None)
    assert float((img0 - ref_img).abs().max()) > 1e-2, "the masks must matter"


def _summary_close(npz, key, arr, rtol=3e-4):  # the comparison of tests/test_fp32_net_gpu.py::test_fp32_network_vs_reference_fixture
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


@pytest.mark.parametrize("name", ["g1", "g1b3"])
def test_fp32_generator_vs_reference_fixture(name):
    """Against the reference's own recorded numbers (tests/golden/gen_*.npz): the image elementwise at the oracle bound, every gradient
    by the fixture's summaries at rtol 3e-4."""
    import gpu_util as u
    npz = np.load(os.path.join(GOLD, f"gen_{name}.npz"))
    n = F32Gen(name)
    n.run(u)
    ri = gr.image_ratio(n.img, torch.from_numpy(npz["out"]))
    assert ri <= 1.0, f"image {ri:.2f} x the bound"
    grads = n.grads()
    assert sorted(grads) == sorted(str(s) for s in npz["param_names"])
    for k, v in grads.items():
        _summary_close(npz, f"grad/{k}", v.numpy())


def _module(name):
    from vit_gan_amd.generator import SirenGenerator
    c = gr.case(name)
    d = c["d"]
    G = SirenGenerator(latent=d.latent, image_size=d.image, channels=d.channels, embed=d.embed, heads=d.heads, layers=d.layers,
                       siren_hidden=d.siren_hidden, omega_0=d.omega0, dropout=0.0, patch_size=d.patch, fourier_features=c["pos_table"] is not None,
                       n_classes=c["K"])
    st = {k: torch.from_numpy(v) for k, v in c["st_np"].items()}
    if c["K"]:
        st[gr.CLASS_KEY] = c["table"]
    G.load_state_dict(st, strict=True)
    return G.cuda(), c


@pytest.mark.parametrize("name", ["p32", "fourier", "cond"])
def test_fp32_module_surface(name):
    """SirenGenerator with precision = "fp32": the image and every parameter's .grad against the oracle; the gradient accumulates on
    a second backward; back in "bf16" the module computes bit for bit what one that never left bf16 computes."""
    import gpu_util as u
    G, c = _module(name)
    G.precision = "fp32"
    z, R = c["z"].cuda(), c["R"].cuda()
    labels = None if not c["K"] else c["labels"].cuda()
    out = G(z, labels)
    assert out.dtype == torch.float32 and out.shape == R.shape
    (out * R).sum().backward()
    u.sync()
    ref_img, ref_g = gr.oracle_f32(name)
    g1 = {k: p.grad.clone() for k, p in G.named_parameters()}
    _check(out, {k: v.cpu() for k, v in g1.items()}, ref_img, ref_g, f"module {name}")
    # a second backward accumulates: the same addends onto themselves, exactly twice the first
    out2 = G(z, labels)
    assert torch.equal(out2, out)
    (out2 * R).sum().backward()
    u.sync()
    for k, p in G.named_parameters():
        assert torch.equal(p.grad, 2.0 * g1[k]), k
    # back to bf16: bitwise what a module that never left bf16 computes
    G.precision = "bf16"
    G.zero_grad()
    ref, _ = _module(name)
    y1, y2 = G(z, labels), ref(z, labels)
    (y1 * R).sum().backward()
    (y2 * R).sum().backward()
    u.sync()
    assert torch.equal(y1, y2) and not torch.equal(y1, out)
    for (k, p1), (_, p2) in zip(G.named_parameters(), ref.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), k


def test_fp32_calls_draw_the_bf16_masks():
    """With one seed the fp32 call applies the masks the bf16 engine applies: the two images stay as close as the two modes are without
    dropout, far closer than two different masks leave them."""
    import gpu_util as u
    from vit_gan_amd import _lib
    n = F32Gen("drop")
    n.run(u)
    c, gd = n.c, n.gd
    Pb = n.P.to(torch.bfloat16)
    img_b = torch.empty_like(n.img, dtype=torch.bfloat16)
    ws = torch.empty(_lib.lib().vg_gen_ws_bytes(C.byref(gd), n.B), dtype=torch.uint8, device="cuda")

    def bf16_image(seed):
        net = _lib.VgGenNet(gd, n.P.data_ptr(), Pb.data_ptr(), n.G.data_ptr(), c["dropout"], seed, None, None)
        u.call("vg_gen_forward", C.byref(net), n.B, u.ptr(n.z), u.ptr(ws), u.ptr(img_b), u.stream())
        u.sync()
        return img_b.float().clone()
    same, other = bf16_image(c["drop_seed"]), bf16_image(c["drop_seed"] + 1)
    u.assert_close(same, n.img, 0.08, "bf16 engine vs fp32 mode, one seed")  # test_net_gpu.py's image tolerance of the bf16 generator
    # two images inside that tier of one reference differ by at most twice it: beyond 2 x 0.08 max|image| the masks are other masks
    top = float(n.img.abs().max())
    d_other = float((other - n.img).abs().max())
    print(f"one seed: {float((same - n.img).abs().max()):.3f}, another seed: {d_other:.3f} (max|image| {top:.3f})")
    assert d_other > 2 * 0.08 * top, "another seed draws other masks"
