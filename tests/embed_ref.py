"""float64 restatement of the discriminator's patch embedding and its backward, with the rounding points of
oracle/bf16_model.py: vit_embed.  A plain helper module, imported like norm_ref.

Forward: the image and conv1.weight enter as bf16 values; everything up to the one rounding of X[0] is exact here (float64):
X[0] = rne_bf16(mask * cat(cls, tiles @ W^T + bias + pos)).  The function returns the value BEFORE that rounding next to the gathered
patch rows, so a test can compare at a tier or round it itself.

Backward: g = dL/dX[0] (bf16 values) times the same mask, then
    d conv_w = sum_{b, s >= 1} g[b, s, :]^T tiles[b, s - 1, :]        d conv_b = sum_{b, s >= 1} g[b, s, :]
    d pos[s - 1] = sum_b g[b, s, :]                                   d cls = sum_b g[b, 0, :]
    d image = un-patchify(g[:, 1:] @ W)
Next to every sum over the batch comes the 2-norm of its terms, elementwise: the scale of the rounding noise of a sum of random-sign
terms, and of the error a mis-scaling would cause (tests/test_blocks_gpu.py judges the SLN scalars the same way).
"""
import torch

from exact_util import BF, rne

F64 = torch.float64


def gather(img, P):
    """[B, C, IH, IW] -> [B, NP, C P P] patch rows in (c, py, px) order, patches row-major over the grid"""
    B, C, IH, IW = img.shape
    gh, gw = IH // P, IW // P
    return img.reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * P * P)


def scatter(rows, C, IH, P):
    """inverse of gather: [B, NP, C P P] -> [B, C, IH, IH]"""
    B = rows.shape[0]
    g = IH // P
    return rows.reshape(B, g, g, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, IH, IH)


def embed_fwd(img, conv_w, conv_b, pos, cls, P, mask=None):
    """img fp32- or bf16-valued [B, C, IH, IH]; conv_w [E, C, P, P], conv_b [E], pos [1, NP, E], cls [1, 1, E] fp32-valued; mask
    [B, S, E] of 0 / keep or None.  Returns apatch (bf16-valued, float64) and x = X[0] before its rounding to bf16."""
    B = img.shape[0]
    E = conv_w.shape[0]
    apatch = gather(rne(img.double(), BF).double(), P)
    w = rne(conv_w.double(), BF).double().reshape(E, -1)
    tok = apatch @ w.t() + conv_b.double() + pos.double().reshape(1, -1, E)
    x = torch.cat([cls.double().reshape(1, 1, E).expand(B, 1, E), tok], dim=1)
    if mask is not None:
        x = x * mask.double()
    return {"apatch": apatch, "x": x}


def embed_bwd(g, apatch, conv_w, C, IH, P, mask=None):
    """g: dL/dX[0] [B, S, E], bf16-valued; apatch as embed_fwd returns it.  Returns the five gradients (float64, no rounding),
    nrm_*: the elementwise 2-norm of the terms of each sum over the batch, and mag_*: the sum of their absolute values."""
    E = conv_w.shape[0]
    g = g.double()
    if mask is not None:
        g = g * mask.double()
    gp = g[:, 1:]                                   # [B, NP, E]
    w = rne(conv_w.double(), BF).double().reshape(E, -1)
    out = {
        "d_w": torch.einsum("bne,bnk->ek", gp, apatch), "nrm_w": torch.einsum("bne,bnk->ek", gp * gp, apatch * apatch).sqrt(),
        "d_b": gp.sum((0, 1)), "nrm_b": (gp * gp).sum((0, 1)).sqrt(),
        "d_pos": gp.sum(0), "nrm_pos": (gp * gp).sum(0).sqrt(),
        "d_cls": g[:, 0].sum(0), "nrm_cls": (g[:, 0] * g[:, 0]).sum(0).sqrt(),
        "d_img": scatter(gp @ w, C, IH, P),
        # sums of the absolute values of the same terms: what bounds the rounding of any fp32 evaluation of the sums
        "mag_w": torch.einsum("bne,bnk->ek", gp.abs(), apatch.abs()), "mag_b": gp.abs().sum((0, 1)), "mag_pos": gp.abs().sum(0),
        "mag_cls": g[:, 0].abs().sum(0),
    }
    return out


def tier_err(got, ref, tier, nrm=None):
    """largest |got - ref| as a fraction of tier * scale; scale = max|ref|, elementwise raised to the 2-norm of the terms (nrm) where
    that exceeds it.  <= 1 passes."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite values"
    scale = torch.full_like(ref, max(float(ref.abs().max()), 1e-12))
    if nrm is not None:
        scale = torch.maximum(scale, nrm.double())
    return float(((got - ref).abs() / (tier * scale)).max())


__all__ = [n for n in dir() if not n.startswith("_")]
