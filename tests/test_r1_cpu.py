"""R1 penalty, what holds without a GPU: the restatements of tests/r1_ref.py (pass 3 against float64 autograd; the oracle is the
gradient of its own value, and the same criterion rejects two planted mistakes), the option parsing and the lazy schedule, the
argument errors of GanEngine / train_model, and the C ABI of vg_vit_r1."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib, ops

import r1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass3_restatement_is_the_derivative_of_the_weighted_penalty():
    g_np = np.random.Generator(np.random.PCG64(3)).standard_normal((5, 48))
    weight = 3.5
    g = torch.from_numpy(g_np).requires_grad_(True)
    pen = g.pow(2).sum(dim=1).mean()
    (u_ref,) = torch.autograd.grad(weight * pen, g)
    pen_img, penalty, u = r1_ref.pass3(g_np, weight)
    assert abs(penalty - float(pen.detach())) <= 1e-12 * abs(float(pen.detach()))
    assert abs(pen_img.sum() - penalty) <= 1e-12 * penalty and pen_img.shape == (5,)
    assert np.abs(u - u_ref.numpy()).max() <= 1e-12 * np.abs(u_ref.numpy()).max()
    # a zero gradient needs no special case
    _, p0, u0 = r1_ref.pass3(np.zeros((2, 8)), 1.0)
    assert p0 == 0.0 and not u0.any()


def _case():
    from make_golden import GP_CASE as c
    from weights import make_input, make_state
    from oracle import vit_oracle as vo
    d = r1_ref.case_dims(c)
    st = make_state(vo.vit_param_shapes(d), c["seed"], "vit")
    x = make_input((c["batch"], c["channels"], c["image"], c["image"]), c["seed"], "uniform")
    return d, st, torch.from_numpy(x).to(torch.bfloat16).float().numpy()  # the images as a bf16 engine is fed them


def _directional(seed, scale=1e-3):
    """(penalty, relative deviation of the central-difference derivative of the VALUE along the gradient from |grad|^2, tensors with a gradient)"""
    d, st, x = _case()
    pen, grads = r1_ref.r1_oracle(st, d, x, torch.float64, seed=seed)
    gn2 = sum(float(g.pow(2).sum()) for g in grads.values() if g is not None)
    h = scale * pen / gn2
    vals = []
    for sgn in (+1.0, -1.0):
        moved = {k: torch.from_numpy(v).double() + (sgn * h * grads[k] if grads[k] is not None else 0.0) for k, v in st.items()}
        vals.append(r1_ref.r1_value(moved, d, x, torch.float64))
    fd = (vals[0] - vals[1]) / (2 * h)
    return pen, abs(fd - gn2) / gn2, grads


def test_oracle_is_the_gradient_of_its_own_value():
    pen, rel, grads = _directional(r1_ref.r1_seed)
    d, st, x = _case()
    pen32 = r1_ref.r1_oracle(st, d, x, torch.float32)[0]
    print(f"R1 on the GP_CASE network: fp64 {pen:.7f}  fp32 {pen32:.7f};  directional derivative off by {rel:.2e} relative")
    assert abs(pen - 0.3291226) < 2e-7 and abs(pen32 - 0.3291225) < 2e-6
    assert [k for k, g in grads.items() if g is None] == ["vit.classifier.fc2.bias"] and len(grads) == 42
    assert rel <= 1e-6


@pytest.mark.parametrize("seed", [r1_ref.gp_seed, r1_ref.mean_first_seed])
def test_the_criterion_rejects_a_planted_mistake(seed):
    _, rel, _ = _directional(seed)
    print(f"{seed.__name__}: directional derivative off by {rel:.2e} relative")
    assert rel > 1e-6


def test_option_parsing_and_the_lazy_schedule():
    assert ops.parse_r1_options(0.0, 1) == (0.0, 1) and ops.parse_r1_options(10, 16) == (10.0, 16)
    for gamma in (-1.0, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="r1_gamma"):
            ops.parse_r1_options(gamma, 1)
    for interval in (0, -2, 1.0, 2.5, True, "4", None):
        with pytest.raises(ValueError, match="r1_interval"):
            ops.parse_r1_options(10.0, interval)
    with pytest.raises(ValueError, match="r1_interval"):
        ops.parse_r1_options(0.0, 4)
    due = lambda k: [s for s in range(1, 12) if ops.r1_due(s, k)]  # noqa: E731
    assert due(1) == list(range(1, 12)) and due(2) == [1, 3, 5, 7, 9, 11] and due(5) == [1, 6, 11]


def _nets():
    from vit_gan_amd.config import Config
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    return ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1)), SirenGenerator(layers=1)


BAD = [(dict(r1_gamma=-1.0), "r1_gamma"), (dict(r1_gamma=float("nan")), "r1_gamma"), (dict(r1_gamma=float("inf")), "r1_gamma"),
       (dict(r1_gamma=10.0, r1_interval=0), "r1_interval"), (dict(r1_gamma=10.0, r1_interval=2.0), "r1_interval"),
       (dict(r1_interval=4), "r1_interval"), (dict(r1_gamma=10.0, gp_weight=10.0), "gp_weight")]


def test_engine_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.engine import GanEngine
    D, G = _nets()
    for kw, match in BAD + [(dict(r1_gamma=10.0, two_stream=True), "two_stream")]:
        with pytest.raises(ValueError, match=match):
            GanEngine(D, G, batch=4, **kw)
    D.vit.attention_fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        GanEngine(D, G, batch=4, r1_gamma=10.0)


def test_trainer_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.training import train_model
    for kw, match in BAD:
        with pytest.raises(ValueError, match=match):
            train_model(save_artifacts=False, **kw)


def test_c_abi_of_the_r1_call():
    """Fails on the parent commit: the symbol, its declaration, its binding and its host-side argument check are this feature's."""
    lib = _lib.lib()
    assert hasattr(lib, "vg_vit_r1")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitgan_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+vg_vit_r1\s*\(([^)]*)\)\s*;", header)
    assert m, "vg_vit_r1 is not declared in include/vitgan_hip.h"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const VgVitNet* net", "int B", "const void* x", "float weight", "void* ws", "void* ws_pen", "float* penalty_out", "void* stream"]
    P = C.c_void_p
    assert _lib._SIGNATURES["vg_vit_r1"] == (C.c_int, [C.POINTER(_lib.VgVitNet), C.c_int, P, C.c_float, P, P, P, P])
    p16 = C.c_void_p(16)  # (non-null dummies: never dereferenced on these paths)
    assert lib.vg_vit_r1(None, 16, p16, 1.0, p16, p16, p16, None) == -1
    d = _lib.VgVitDims(3, 32, 4, 384, 4, 6, 2, 1)
    net = _lib.VgVitNet(d, 16, 16, 16, 0.1, 1, None, None, 0, 0)
    assert lib.vg_vit_r1(C.byref(net), 16, None, 1.0, p16, p16, p16, None) == -1
    assert lib.vg_vit_r1(C.byref(net), 0, p16, 1.0, p16, p16, p16, None) == -1
    nog = _lib.VgVitNet(d, 16, 16, None, 0.1, 1, None, None, 0, 0)
    assert lib.vg_vit_r1(C.byref(nog), 16, p16, 1.0, p16, p16, p16, None) == -1    # no gradient buffer to accumulate into
    net8 = _lib.VgVitNet(d, 16, 16, 16, 0.1, 1, None, None, 1, 0)
    assert lib.vg_vit_r1(C.byref(net8), 16, p16, 1.0, p16, p16, p16, None) == -3   # fp8 attention
    long_ = _lib.VgVitNet(_lib.VgVitDims(3, 224, 16, 768, 12, 2, 2, 1), 16, 16, 16, 0.0, 1, None, None, 0, 0)
    assert lib.vg_vit_r1(C.byref(long_), 16, p16, 1.0, p16, p16, p16, None) == -3  # 197 tokens > 80
