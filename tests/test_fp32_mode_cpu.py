"""fp32 mode, CPU side: the new C-ABI symbols are exported and validate their arguments without a device, the workspace query
covers every golden case, and the module attribute leaves the reference's contract (state_dict, Config) untouched."""
import ctypes as C

import pytest
import torch

import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib
from vit_gan_amd.config import Config

F32_SYMBOLS = ("vg_vit_ws_bytes_f32", "vg_vit_forward_f32", "vg_vit_backward_f32", "vg_linear_f32_fwd", "vg_linear_f32_dgrad",
               "vg_linear_f32_wgrad_slab_floats", "vg_linear_f32_wgrad", "vg_attention_f32_fwd", "vg_attention_f32_bwd",
               "vg_layernorm_f32_fwd", "vg_layernorm_f32_bwd_part_floats", "vg_layernorm_f32_bwd")


def test_fp32_symbols_exported_with_signatures():
    lib = _lib.lib()
    for n in F32_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGNATURES, n
    assert lib.vg_abi_version() == 9


def _net(dims, attn_fp8=0, G=16):
    return _lib.VgVitNet(dims, 16, 16, G, 0.0, 0, None, None, attn_fp8, 0)  # non-null dummies: never dereferenced on these paths


def test_fp32_argument_validation_without_gpu():
    lib = _lib.lib()
    p = C.c_void_p(16)
    d = _lib.VgVitDims(3, 32, 4, 384, 4, 6, 2, 1)
    net = _net(d)
    # null pointers
    assert lib.vg_vit_forward_f32(None, 2, p, p, p, None) == -1
    assert lib.vg_vit_forward_f32(C.byref(net), 2, None, p, p, None) == -1
    assert lib.vg_vit_forward_f32(C.byref(net), 2, p, None, p, None) == -1
    assert lib.vg_vit_backward_f32(C.byref(net), 2, None, p, p, 1, None) == -1
    assert lib.vg_vit_backward_f32(C.byref(_net(d, G=None)), 2, p, p, p, 1, None) == -1  # no gradient buffer to accumulate into
    assert lib.vg_linear_f32_fwd(None, p, None, None, p, None, 8, 8, 8, 0, 0.0, 0, 0, None, None) == -1
    assert lib.vg_linear_f32_dgrad(p, None, None, p, 8, 8, 8, 0, None) == -1
    assert lib.vg_linear_f32_dgrad(p, p, None, p, 8, 8, 8, 1, None) == -1  # GELU' needs the pre-activation
    assert lib.vg_linear_f32_wgrad(p, None, p, None, p, 1 << 30, 8, 8, 8, None) == -1
    assert lib.vg_attention_f32_fwd(None, None, None, 1, 1, 1, 32, 1.0, None) == -1
    assert lib.vg_attention_f32_bwd(p, p, None, p, p, 1, 1, 1, 32, 1.0, None) == -1
    assert lib.vg_layernorm_f32_fwd(p, p, p, None, p, p, 4, 384, 1e-5, None) == -1
    assert lib.vg_layernorm_f32_bwd(p, p, p, p, None, None, p, None, None, None, 4, 384, None) == -1
    # unsupported shapes: HE = 48 (E = 384, 8 heads), 257 tokens; bad modes
    he48 = _lib.VgVitDims(3, 32, 4, 384, 8, 6, 2, 1)
    assert lib.vg_vit_forward_f32(C.byref(_net(he48)), 2, p, p, p, None) == -3
    assert lib.vg_vit_backward_f32(C.byref(_net(he48)), 2, p, p, p, 1, None) == -3
    t257 = _lib.VgVitDims(3, 64, 4, 384, 4, 6, 2, 1)
    assert lib.vg_vit_forward_f32(C.byref(_net(t257)), 2, p, p, p, None) == -3
    assert lib.vg_vit_ws_bytes_f32(C.byref(t257), 2) == -1 and lib.vg_vit_ws_bytes_f32(None, 2) == -1
    assert lib.vg_attention_f32_fwd(p, p, p, 1, 8, 65, 48, 1.0, None) == -3
    assert lib.vg_attention_f32_fwd(p, p, p, 1, 4, 257, 96, 1.0, None) == -3
    assert lib.vg_layernorm_f32_fwd(p, p, p, p, p, p, 4, 320, 1e-5, None) == -3
    assert lib.vg_linear_f32_fwd(p, p, None, None, p, None, 8, 8, 8, 3, 0.0, 0, 0, None, None) == -4
    assert lib.vg_linear_f32_dgrad(p, p, p, p, 8, 8, 8, 3, None) == -4
    # the fp32 mode has no fp8 attention
    assert lib.vg_vit_forward_f32(C.byref(_net(d, attn_fp8=1)), 2, p, p, p, None) == -4
    assert lib.vg_vit_backward_f32(C.byref(_net(d, attn_fp8=1)), 2, p, p, p, 1, None) == -4
    # scratch sizes are checked before any launch
    need = lib.vg_linear_f32_wgrad_slab_floats(16640, 1152, 384)
    assert need >= 1152 * 384 and lib.vg_linear_f32_wgrad_slab_floats(0, 8, 8) == -2
    assert lib.vg_linear_f32_wgrad(p, p, p, None, p, need - 1, 16640, 1152, 384, None) == -2
    assert lib.vg_layernorm_f32_bwd_part_floats(16640, 384) == 2 * 384 * 65


def test_fp32_workspace_for_every_golden_case():
    from cases import VIT_CASES
    lib = _lib.lib()
    for name, c in VIT_CASES.items():
        d = _lib.VgVitDims(c["channels"], c["image"], c["patch"], c["embed"], c["heads"], c["layers"], c["mlp_ratio"], c["classes"])
        for B in (c["batch"], 5):
            assert lib.vg_vit_ws_bytes_f32(C.byref(d), B) > 0, (name, B)


def test_precision_attribute_leaves_the_contract_unchanged():
    from vit_gan_amd.modules import ViTDiscriminator, ViTGenerator
    torch.manual_seed(0)
    cfg = Config(embeddings_dimension=128, transformer_blocks_count=2)
    s_before = str(cfg)
    D = ViTDiscriminator(cfg)
    assert D.vit.precision == "bf16"
    sd0 = {k: v.clone() for k, v in D.state_dict().items()}
    D.vit.precision = "fp32"
    sd1 = D.state_dict()
    assert list(sd1) == list(sd0)
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    assert str(Config(embeddings_dimension=128, transformer_blocks_count=2)) == s_before and str(Config()) == str(Config())
    assert "precision" not in str(Config()) and "precision" not in Config.model_fields
    D.vit.precision = "bf16"
    assert D.vit.precision == "bf16"
    for bad in ("fp16", "FP32", "", None, 32):
        with pytest.raises(ValueError):
            D.vit.precision = bad
    assert D.vit.precision == "bf16"
    G = ViTGenerator(Config(classes_count=10, batch_size=3, embeddings_dimension=128, transformer_blocks_count=1))
    G.vit.precision = "fp32"
    assert G.vit.precision == "fp32"


def test_fp32_mode_refused_where_the_path_is_bf16():
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.penalty import gradient_penalty
    D = ViTDiscriminator(Config(embeddings_dimension=128, transformer_blocks_count=1, dropout_rate=0.0))
    G = SirenGenerator(layers=1, dropout=0.0)
    D.vit.precision = "fp32"
    with pytest.raises(ValueError, match="fp32"):
        GanEngine(D, G, batch=4)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match="fp32"):
        gradient_penalty(D, x, x)
    with pytest.raises(ValueError, match="bf16"):
        D.vit.twice_differentiable_forward(x)
