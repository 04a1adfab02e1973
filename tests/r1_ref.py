"""The R1 penalty restated without product code (a plain helper module, imported like second_order_ref).

(a) ``pass3``: pass 3 of ``vg_vit_r1`` (the R1 variant of vg_pen_norm_kernel + vg_pen_sum_kernel) in numpy float64.
(b) ``r1_oracle``: penalty = mean_b ||d sum_k D(x_b)_k / d x_b||^2 and its parameter gradient over oracle.vit_oracle.vit_forward, torch
    autograd with create_graph=True.  The gradient is formed the way the call forms it - the image gradient g contracted with a SEED
    u = d penalty / d g and differentiated again - so a wrong seed can be planted (tests/test_r1_cpu.py does) and caught.
"""
import numpy as np
import torch

from oracle import vit_oracle as vo


def pass3(g, weight):
    """g [B, per], weight -> (pen_img [B], penalty, u [B, per]): n2_b = sum g_b^2, pen_img = n2_b / B, penalty = sum_b pen_img,
    u_b = (2 weight / B) g_b = d(weight * penalty) / d g_b.  No square root, no division by the norm."""
    g = np.asarray(g, dtype=np.float64)
    B = g.shape[0]
    pen_img = (g * g).sum(axis=1) / B
    return pen_img, float(pen_img.sum()), (2.0 * float(weight) / B) * g


def r1_seed(g: torch.Tensor) -> torch.Tensor:
    """d penalty / d g for g [B, per]: pass 3 at weight 1"""
    return torch.from_numpy(pass3(g.detach().double().numpy(), 1.0)[2]).to(g.dtype)


def gp_seed(g: torch.Tensor) -> torch.Tensor:
    """PLANTED MISTAKE: WGAN-GP's seed, (n - 1) / n of R1's"""
    n = g.norm(2, dim=1, keepdim=True)
    return (n - 1) / n * r1_seed(g)


def mean_first_seed(g: torch.Tensor) -> torch.Tensor:
    """PLANTED MISTAKE: the mean over the batch taken before the square, d ||mean_b g_b||^2 / d g_b = 2 / B mean_b g_b"""
    return (2.0 / g.shape[0]) * g.mean(dim=0, keepdim=True).expand_as(g).contiguous()


def case_dims(c) -> vo.VitDims:
    return vo.VitDims(channels=c["channels"], image=c["image"], patch=c["patch"], embed=c["embed"], heads=c["heads"], layers=c["layers"],
                      mlp_ratio=c["mlp_ratio"], classes=c["classes"])


def _image_grad(st, x, dims):
    x = x.detach().clone().requires_grad_(True)
    out = vo.vit_forward(st, x, dims)
    (g,) = torch.autograd.grad(out, x, grad_outputs=torch.ones_like(out), create_graph=True)
    return g.reshape(x.shape[0], -1)


def r1_value(state, dims, x, dtype) -> float:
    st = {k: torch.as_tensor(v).to(dtype) for k, v in state.items()}
    g = _image_grad({k: v.requires_grad_(True) for k, v in st.items()}, torch.as_tensor(x).to(dtype), dims)
    return float(g.detach().pow(2).sum(dim=1).mean())


def r1_oracle(state, dims, x, dtype, seed=r1_seed):
    """(penalty, {name: d penalty / d theta or None}) in ``dtype``; state: name -> array or tensor, x [B, C, IH, IH]"""
    st = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    g = _image_grad(st, torch.as_tensor(x).to(dtype), dims)
    pen = float(g.detach().pow(2).sum(dim=1).mean())
    names = list(st)
    grads = torch.autograd.grad((seed(g.detach()) * g).sum(), [st[k] for k in names], allow_unused=True)
    return pen, dict(zip(names, grads))
