"""81 to 256 tokens, CPU side (no GPU): the layouts accept the patch grids 9x9 .. 15x15 (+ CLS) and the patch-grid / row generators
up to 256 tokens, 257 stays refused, and every path whose attention kernels stay S <= 80 (fp32 mode, fp8 attention, the gradient
penalty's second-order attention) is refused before anything is launched - in the C ABI and in the nn.Module surface."""
import ctypes as C

import pytest
import torch

import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib
from vit_gan_amd.config import Config

LONG_VITS = [(3, 224, 16, 768, 12, 6, 2, 1), (3, 48, 4, 384, 4, 6, 2, 1), (3, 60, 4, 128, 4, 6, 2, 1)]  # S = 197, 145, 226
S197 = (3, 224, 16, 768, 12, 2, 2, 1)


def _vit_layout(dims):
    return _lib.lib().vg_vit_layout(C.byref(_lib.VgVitDims(*dims)), C.byref(_lib.VgVitLayout()))


def _gen_layout(*args):
    return _lib.lib().vg_gen_layout(C.byref(_lib.VgGenDims(*args)), C.byref(_lib.VgGenLayout()))


@pytest.mark.parametrize("dims", LONG_VITS)
def test_vit_layout_accepts_up_to_256_tokens(dims):
    assert _vit_layout(dims) == 0
    d = _lib.VgVitDims(*dims)
    assert _lib.lib().vg_vit_ws_bytes(C.byref(d), 2) > 0


def test_vit_layout_every_square_grid_to_15x15():
    for n in range(9, 16):
        assert _vit_layout((3, 4 * n, 4, 128, 4, 2, 2, 1)) == 0, n
    assert _vit_layout((3, 64, 4, 384, 4, 6, 2, 1)) == -3  # 16 x 16 + CLS = 257 tokens


def test_gen_layout_tokens():
    # patch-grid generator at 48/4: T = 144, CW = 3 * 4 * 4
    assert _gen_layout(128, 144, 384, 4, 2, 128, 48, 30.0, 4, 3, 48) == 0
    assert _gen_layout(128, 225, 384, 4, 2, 128, 48, 30.0, 4, 3, 60) == 0
    # v1 row generator (patch = 0): T rows up to 256
    assert _gen_layout(128, 256, 128, 4, 2, 128, 96, 30.0, 0, 3, 32) == 0
    assert _gen_layout(128, 257, 128, 4, 2, 128, 96, 30.0, 0, 3, 32) == -3
    assert _gen_layout(128, 256, 384, 4, 2, 128, 48, 30.0, 4, 3, 64) == 0
    assert _gen_layout(128, 289, 384, 4, 2, 128, 48, 30.0, 4, 3, 68) == -3  # 17 x 17


def _net(dims, attn_fp8=0):
    return _lib.VgVitNet(_lib.VgVitDims(*dims), 16, 16, 16, 0.0, 0, None, None, attn_fp8, 0)  # dummies: never dereferenced


def test_short_only_paths_refused_before_any_launch():
    lib = _lib.lib()
    p = C.c_void_p(16)
    d = _lib.VgVitDims(*S197)
    # fp32 mode (its attention kernels are S <= 80)
    assert lib.vg_vit_forward_f32(C.byref(_net(S197)), 2, p, p, p, None) == -3
    assert lib.vg_vit_backward_f32(C.byref(_net(S197)), 2, p, p, p, 1, None) == -3
    assert lib.vg_vit_ws_bytes_f32(C.byref(d), 2) == -1
    # fp8 attention
    assert lib.vg_vit_forward(C.byref(_net(S197, attn_fp8=1)), 2, p, 0, p, p, None) == -3
    assert lib.vg_vit_backward(C.byref(_net(S197, attn_fp8=1)), 2, p, p, None, 1, None) == -3
    # gradient penalty (second-order attention kernels are S <= 80)
    assert lib.vg_vit_penalty(C.byref(_net(S197)), 16, p, p, p, 1.0, p, p, p, None) == -3
    # the same calls at 65 tokens still get past these checks: the fp32 workspace query answers
    assert lib.vg_vit_ws_bytes_f32(C.byref(_lib.VgVitDims(3, 32, 4, 384, 4, 2, 2, 1)), 2) > 0


def test_attention_entry_points_range():
    lib = _lib.lib()
    p = C.c_void_p(16)
    assert lib.vg_attention_fwd(p, p, p, 1, 4, 257, 64, 1.0, None) == -2
    assert lib.vg_attention_bwd(p, p, p, p, p, 1, 4, 257, 64, 1.0, None) == -2
    assert lib.vg_attention_cls_fwd(p, p, p, 1, 4, 257, 64, 1.0, None) == -2
    assert lib.vg_attention_cls_bwd(p, p, p, p, p, 1, 4, 257, 64, 1.0, None) == -2
    # L2-distance scores and fp8 operands stay S <= 80
    assert lib.vg_attention_l2_fwd(p, p, p, 1, 4, 81, 64, 1.0, None) == -2
    assert lib.vg_attention_l2_bwd(p, p, p, p, p, 1, 4, 81, 64, 1.0, None) == -2
    assert lib.vg_attention_fp8_fwd(p, p, p, 1, 4, 81, 64, 1.0, None) == -2
    assert lib.vg_attention_fp8_bwd(p, p, p, p, p, 1, 4, 81, 64, 1.0, None) == -2
    assert lib.vg_attention_bwd_bwd(p, p, p, p, p, p, 1, 4, 81, 64, 1.0, None) == -2
    # head dim still 32 / 64 / 96 on the long path
    assert lib.vg_attention_fwd(p, p, p, 1, 8, 197, 48, 1.0, None) == -3


def _long_discriminator():
    from vit_gan_amd.modules import ViTDiscriminator
    return ViTDiscriminator(Config(image_size=224, patch_size=16, embeddings_dimension=768, attention_heads_count=12,
                                   transformer_blocks_count=1, dropout_rate=0.0))


def test_module_builds_at_197_tokens():
    D = _long_discriminator()
    assert D.vit.tokens == 197
    assert D.vit.precision == "bf16" and D.vit.attention_fp8 is False


def test_module_refuses_short_only_modes():
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.penalty import gradient_penalty
    D = _long_discriminator()
    with pytest.raises(ValueError, match="80 tokens"):
        D.vit.precision = "fp32"
    assert D.vit.precision == "bf16"
    with pytest.raises(ValueError, match="80 tokens"):
        D.vit.attention_fp8 = True
    assert D.vit.attention_fp8 is False
    D.vit.attention_fp8 = False  # switching it off is always allowed
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(ValueError, match="80 tokens"):
        D.vit.twice_differentiable_forward(x)
    with pytest.raises(ValueError, match="80 tokens"):
        gradient_penalty(D, x, x)
    G = SirenGenerator(layers=1, dropout=0.0)
    with pytest.raises(ValueError, match="80 tokens"):
        GanEngine(D, G, batch=4, gp_weight=10.0)


def test_short_networks_keep_every_mode():
    from vit_gan_amd.modules import ViTDiscriminator
    D = ViTDiscriminator(Config(embeddings_dimension=128, transformer_blocks_count=1))
    assert D.vit.tokens == 65
    D.vit.attention_fp8 = True
    D.vit.attention_fp8 = False
    D.vit.precision = "fp32"
    D.vit.precision = "bf16"
