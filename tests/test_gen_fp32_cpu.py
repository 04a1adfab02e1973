"""The generator's fp32 mode without a GPU: the exports and their signatures, the refusals of the C calls (all on the host, with a NULL
stream), the ``precision`` property of SirenGenerator, GanEngine's refusal, and the admissibility of the bounds the GPU tests apply -
the float32 oracle against the float64 oracle stays within half of every one of them on every network case."""
import ctypes as C

import pytest
import torch

import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib

import gen_f32_ref as gr

NEW = ("vg_gen_ws_bytes_f32", "vg_gen_forward_f32", "vg_gen_backward_f32", "vg_sln_f32_fwd", "vg_sln_f32_bwd", "vg_sln_f32_bwd_part_floats",
       "vg_siren_f32_fwd", "vg_siren_f32_dgrad")
p = C.c_void_p(4096)  # a non-null dummy: never dereferenced on the paths below


def _dims(d):
    return _lib.VgGenDims(d.latent, d.tokens, d.embed, d.heads, d.layers, d.siren_hidden, d.out_features, d.omega0, d.patch, d.channels, d.image)


def _g1():
    return _lib.VgGenDims(1024, 32, 384, 4, 4, 768, 96, 30.0, 0, 3, 32)


def test_new_symbols_are_exported_with_signatures_and_the_abi_is_9():
    lib = _lib.lib()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib._SIGNATURES, n
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9


@pytest.mark.parametrize("name", list(gr.CASES))
def test_workspace_size_of_every_case(name):
    c = gr.case(name)
    small, large = (_lib.lib().vg_gen_ws_bytes_f32(C.byref(_dims(c["d"])), B) for B in (c["B"], 2 * c["B"]))
    assert 0 < small < large


def test_whole_network_calls_refuse_on_the_host():
    lib = _lib.lib()
    d = _g1()
    net = _lib.VgGenNet(d, 4096, None, 4096, 0.0, 0, None, None)  # Pb is ignored: NULL is fine
    cond = _lib.VgGenCondF32(4096, 4096, 4096, 3)
    fwd = lambda net_, B, z, ws, img, cond_: lib.vg_gen_forward_f32(net_, B, z, ws, img, cond_, None)  # noqa: E731
    bwd = lambda net_, B, ws, dimg, cond_: lib.vg_gen_backward_f32(net_, B, ws, dimg, cond_, None)  # noqa: E731
    # -1: a null pointer or B < 1
    assert fwd(None, 2, p, p, p, None) == -1 and bwd(None, 2, p, p, None) == -1
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert fwd(C.byref(net), 2, *a, None) == -1, hole
    assert bwd(C.byref(net), 2, None, p, None) == -1 and bwd(C.byref(net), 2, p, None, None) == -1
    assert fwd(C.byref(net), 0, p, p, p, None) == -1 and bwd(C.byref(net), 0, p, p, None) == -1
    assert fwd(C.byref(net), -3, p, p, p, None) == -1
    assert fwd(C.byref(_lib.VgGenNet(d, None, None, 4096, 0.0, 0, None, None)), 2, p, p, p, None) == -1   # no master
    assert bwd(C.byref(_lib.VgGenNet(d, 4096, None, None, 0.0, 0, None, None)), 2, p, p, None) == -1     # no gradient buffer
    for hole in ("labels", "table"):
        bad = _lib.VgGenCondF32(4096, 4096, 4096, 3)
        setattr(bad, hole, None)
        assert fwd(C.byref(net), 2, p, p, p, C.byref(bad)) == -1 and bwd(C.byref(net), 2, p, p, C.byref(bad)) == -1, hole
    nograd = _lib.VgGenCondF32(4096, 4096, None, 3)
    assert bwd(C.byref(net), 2, p, p, C.byref(nograd)) == -1
    # -2: K outside [1, 16]
    for K in (0, 17, -1):
        bad = _lib.VgGenCondF32(4096, 4096, 4096, K)
        assert fwd(C.byref(net), 2, p, p, p, C.byref(bad)) == -2 and bwd(C.byref(net), 2, p, p, C.byref(bad)) == -2, K
    # -3: a shape vg_gen_layout refuses, more than 80 tokens, a head width outside {32, 64, 96}
    shapes = {
        "E not a multiple of 128": _lib.VgGenDims(1024, 32, 200, 4, 4, 768, 96, 30.0, 0, 3, 32),
        "head width 128": _lib.VgGenDims(1024, 32, 512, 4, 4, 768, 96, 30.0, 0, 3, 32),
        "head width 16": _lib.VgGenDims(1024, 32, 128, 8, 4, 768, 96, 30.0, 0, 3, 32),
        "81 tokens": _lib.VgGenDims(1024, 81, 384, 4, 4, 768, 8 * 3, 30.0, 0, 3, 32),
        "256 tokens (the bf16 engine's limit)": _lib.VgGenDims(256, 256, 384, 4, 2, 256, 3 * 16, 30.0, 4, 3, 64),
        "60 tokens are not the 8 x 8 grid": _lib.VgGenDims(128, 60, 256, 4, 1, 128, 192, 30.0, 8, 3, 64),
        "no layers": _lib.VgGenDims(1024, 32, 384, 4, 0, 768, 96, 30.0, 0, 3, 32),
    }
    for what, bad in shapes.items():
        nb = _lib.VgGenNet(bad, 4096, None, 4096, 0.0, 0, None, None)
        assert fwd(C.byref(nb), 2, p, p, p, None) == -3, what
        assert fwd(C.byref(nb), 2, p, p, p, C.byref(cond)) == -3, what
        assert bwd(C.byref(nb), 2, p, p, None) == -3, what
        assert lib.vg_gen_ws_bytes_f32(C.byref(bad), 2) == -1, what
    assert lib.vg_gen_ws_bytes_f32(None, 2) == -1 and lib.vg_gen_ws_bytes_f32(C.byref(d), 0) == -1
    # the bf16 engine takes the 256-token network the fp32 mode refuses
    assert lib.vg_gen_ws_bytes(C.byref(shapes["256 tokens (the bf16 engine's limit)"]), 2) > 0
    # 80 tokens are taken
    assert lib.vg_gen_ws_bytes_f32(C.byref(_lib.VgGenDims(1024, 80, 384, 4, 4, 768, 24, 30.0, 0, 3, 32)), 2) > 0


def test_single_operators_refuse_on_the_host():
    lib = _lib.lib()
    sln_f = lambda a, R, E, hb=0: lib.vg_sln_f32_fwd(a[0], hb, a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], R, E, 1e-5, None)  # noqa: E731
    for hole in range(9):
        a = [p] * 9
        a[hole] = None
        assert sln_f(a, 4, 128) == -1, hole
    assert sln_f([p] * 9, 0, 128) == -2 and sln_f([p] * 9, 4, 128, hb=-1) == -2
    for E in (0, 64, 192, 1152, 2048):
        assert sln_f([p] * 9, 4, E) == -3, E

    def sln_b(a, R, E, acc=0, hb=0):  # a: dy h w mean rstd lw lb gs bs gres dh dw_acc dlw dlb dgs dbs part
        return lib.vg_sln_f32_bwd(a[0], a[1], hb, *a[2:12], acc, *a[12:17], R, E, None)
    for hole in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11):
        a = [p] * 17
        a[hole] = None
        assert sln_b(a, 4, 128) == -1, hole
    for hole in (12, 13, 14, 15, 16):  # the four parameter sums and their scratch: all or none
        a = [p] * 17
        a[hole] = None
        assert sln_b(a, 4, 128) == -1, hole
    assert sln_b([p] * 17, 0, 128) == -2 and sln_b([p] * 17, 4, 128, acc=2) == -2 and sln_b([p] * 17, 4, 128, hb=-2) == -2
    assert sln_b([p] * 17, 4, 100) == -3
    assert sln_b([p] * 16 + [C.c_void_p(4100)], 4, 128) == -3  # the scratch holds fp64 row sums: 8-byte aligned
    assert lib.vg_sln_f32_bwd_part_floats(0, 128) == -2 and lib.vg_sln_f32_bwd_part_floats(4, 100) == -2
    # ceil(R / 256) partial rows of 2E + 2 floats (padded to an even count), then two doubles per row
    assert lib.vg_sln_f32_bwd_part_floats(256, 128) == 258 + 4 * 256 and lib.vg_sln_f32_bwd_part_floats(257, 384) == 2 * 770 + 4 * 257

    for hole in (0, 1, 3, 4):  # X, W, Y, Z (the bias is optional)
        a = [p] * 5
        a[hole] = None
        assert lib.vg_siren_f32_fwd(*a, 4, 8, 8, 30.0, None) == -1, hole
    for M, N, K in ((0, 8, 8), (4, 0, 8), (4, 8, 0)):
        assert lib.vg_siren_f32_fwd(p, p, p, p, p, M, N, K, 30.0, None) == -2
    for hole in (0, 2, 3):  # dY, aux, dX (W == NULL is the elementwise form)
        a = [p] * 4
        a[hole] = None
        assert lib.vg_siren_f32_dgrad(*a, 4, 8, 8, 30.0, None) == -1, hole
    assert lib.vg_siren_f32_dgrad(p, p, p, p, 4, 8, 0, 30.0, None) == -2 and lib.vg_siren_f32_dgrad(p, None, p, p, 0, 8, 0, 30.0, None) == -2
    # the generic fp32 Linear keeps refusing the new epilogue codes
    for act in (3, 5, 6):
        assert lib.vg_linear_f32_fwd(p, p, p, None, p, p, 4, 8, 8, act, 0.0, 0, 0, None, None) == -4, act
        assert lib.vg_linear_f32_dgrad(p, p, p, p, 4, 8, 8, act, None) == -4, act


def _small(**kw):
    from vit_gan_amd.generator import SirenGenerator
    a = dict(latent=64, image_size=32, channels=3, embed=128, heads=4, layers=1, siren_hidden=64, dropout=0.0)
    a.update(kw)
    return SirenGenerator(**a)


def test_precision_property():
    import inspect
    from vit_gan_amd.config import Config
    from vit_gan_amd.generator import SirenGenerator
    assert "precision" not in inspect.signature(SirenGenerator.__init__).parameters and not hasattr(Config(), "precision")
    assert isinstance(SirenGenerator.precision, property)
    torch.manual_seed(5)
    G = _small()
    torch.manual_seed(5)
    twin = _small()
    assert G.precision == "bf16"
    before = {k: v.clone() for k, v in G.state_dict().items()}
    names = [k for k, _ in G.named_parameters()]
    G.precision = "fp32"
    assert G.precision == "fp32"
    after = G.state_dict()
    assert list(after) == list(before) == list(twin.state_dict()) and names == [k for k, _ in G.named_parameters()]
    for k, v in before.items():
        assert torch.equal(after[k], v) and torch.equal(twin.state_dict()[k], v), k  # the same init draws, untouched by the switch
    for bad in ("fp16", "FP32", "", None, 32):
        with pytest.raises(ValueError):
            G.precision = bad
        assert G.precision == "fp32"
    G.precision = "bf16"
    assert G.precision == "bf16" and all(torch.equal(G.state_dict()[k], v) for k, v in before.items())
    # the conditional generator keeps its table where it was
    Gc = _small(n_classes=3)
    keys = list(Gc.state_dict())
    Gc.precision = "fp32"
    assert list(Gc.state_dict()) == keys and keys[-1] == "class_embedding.weight"


def test_precision_fp32_refuses_what_the_kernels_do_not_take():
    G = _small(image_size=64, patch_size=4, embed=128, heads=4)  # 256 tokens: the bf16 engine's, above the fp32 attention's 80
    with pytest.raises(ValueError, match="80 tokens"):
        G.precision = "fp32"
    assert G.precision == "bf16"
    G = _small(image_size=64, patch_size=8)  # 64 tokens
    G.precision = "fp32"
    with pytest.raises(RuntimeError, match="cuda"):
        G(torch.zeros(2, 64))  # no CPU fallback in either mode


def test_gan_engine_refuses_an_fp32_generator():
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.modules import ViTDiscriminator
    D = ViTDiscriminator(Config(embeddings_dimension=128, transformer_blocks_count=1))
    G = _small()
    G.precision = "fp32"
    with pytest.raises(ValueError, match="fp32"):
        GanEngine(D, G, batch=4)


@pytest.mark.parametrize("name", list(gr.CASES))
def test_bounds_are_admissible(name):
    """float32 oracle against float64 oracle (both gen_oracle.gen_forward): within 0.5 of every bound the GPU test applies, so a kernel
    with another summation order has the same room again.  Measured: 0.21 on the image, 0.13 on gradients at the worst."""
    masks = gr.host_masks(name)
    img64, g64 = gr.oracle_run(name, torch.float64, masks)
    img32, g32 = gr.oracle_f32(name)
    ri = gr.image_ratio(img32, img64)
    worst = {k: gr.grad_ratio(g32[k], g64[k]) for k in g64}
    top = max(worst, key=worst.get)
    print(f"{name}: image {ri:.3f} of its bound (max |d| {float((img32.double() - img64).abs().max()):.2e}), worst gradient {worst[top]:.3f} ({top})")
    assert set(g32) == set(g64) and (gr.CLASS_KEY in g64) == bool(gr.case(name)["K"])
    assert ri <= 0.5
    for k, r in worst.items():
        assert r <= 0.5, (k, r)
    if masks is not None:  # the masks matter
        img0, _ = gr.oracle_run(name, torch.float32, None)
        assert float((img0 - img32).abs().max()) > 1e-2
