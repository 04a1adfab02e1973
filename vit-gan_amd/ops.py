"""torch.autograd.Functions over the single-operator C ABI (bf16 compute, fp32 accumulate).

These give every reference block (EmbedLayer, SelfAttention, Encoder, Classifier) a standalone
HIP path with autograd.  The whole-network passes in ``modules.py`` bypass them (one C call per
forward/backward); they are used when a block is called on its own, or when dropout is active.
There is no CPU path: a non-cuda tensor raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib

BF = torch.bfloat16


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the HIP path needs cuda tensors (got {t.device}); there is no CPU fallback")


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(BF).contiguous()


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _pad_rows(w: torch.Tensor, mult: int = 8) -> torch.Tensor:
    n = w.shape[0]
    if n % mult == 0:
        return w
    out = torch.zeros((n + mult - n % mult,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    out[:n] = w
    return out


def _wgrad(dy_b, x_b, M, N, K):
    """dW[N,K] = dy^T x via the split-K MFMA kernel (deterministic)."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    splits = max(1, min(8, 512 // max(tiles, 1), max(1, (M // 64) // 4)))
    dW = torch.empty(N, K, dtype=torch.float32, device=dy_b.device)
    slab = torch.empty(splits * N * K, dtype=torch.float32, device=dy_b.device)
    _lib.call("vg_linear_wgrad", _lib.ptr(dy_b), _lib.ptr(x_b), _lib.ptr(dW), _lib.ptr(slab), slab.numel(), M, N, K, splits, 0, _lib.stream())
    return dW


def _bias_grad(dy_b, M, N):
    parts = _lib.lib().vg_colsum_bf16_parts(M)
    ws = torch.empty(parts * N, dtype=torch.float32, device=dy_b.device)
    db = torch.empty(N, dtype=torch.float32, device=dy_b.device)
    _lib.call("vg_colsum_bf16", _lib.ptr(dy_b), N, M, N, _lib.ptr(ws), _lib.ptr(db), 0, _lib.stream())
    return db


class LinearFn(torch.autograd.Function):
    """y = x W^T + b (+ res).  F.linear of src/v2/modules.py:128-139,161."""

    @staticmethod
    def forward(ctx, x, weight, bias, res):
        _need_cuda(x, "linear")
        K0 = x.shape[-1]
        N0 = weight.shape[0]
        xb = _bf(x).reshape(-1, K0)
        M = xb.shape[0]
        wb = _pad_rows(_bf(weight))
        if K0 % 8:  # zero-pad the reduction dim (e.g. Linear(classes_count=10, ...))
            xb = _pad_rows(xb.t().contiguous()).t().contiguous()
            wb = _pad_rows(wb.t().contiguous()).t().contiguous()
        K = xb.shape[1]
        N = wb.shape[0]
        bb = None if bias is None else _pad_rows(_f32(bias))
        rb = None if res is None else _bf(res).reshape(M, N0)
        if rb is not None and N != N0:
            raise RuntimeError("residual with a padded output is not supported")
        y = torch.empty(M, N, dtype=BF, device=x.device)
        _lib.call("vg_linear_fwd", _lib.ptr(xb), _lib.ptr(wb), _lib.ptr(bb), _lib.ptr(rb), _lib.ptr(y), None, None, M, N, K, 0, 0.0, _lib.stream())
        ctx.save_for_backward(xb, wb)
        ctx.dims = (M, N, K, N0, K0, bias is not None, res is not None, x.shape, x.dtype)
        return y[:, :N0].reshape(x.shape[:-1] + (N0,)).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        M, N, K, N0, K0, has_b, has_r, xshape, xdtype = ctx.dims
        dyb = _bf(dy).reshape(M, N0)
        if N != N0:
            t = torch.zeros(M, N, dtype=BF, device=dy.device)
            t[:, :N0] = dyb
            dyb = t
        dx = torch.empty(M, K, dtype=BF, device=dy.device)
        _lib.call("vg_linear_dgrad", _lib.ptr(dyb), _lib.ptr(wb), _lib.ptr(dx), M, N, K, 0, None, None, 0.0, _lib.stream())
        dW = _wgrad(dyb, xb, M, N, K)[:N0, :K0]
        db = _bias_grad(dyb, M, N)[:N0] if has_b else None
        dres = dy if has_r else None
        return dx[:, :K0].reshape(xshape).to(xdtype), dW, db, dres


class MlpFn(torch.autograd.Function):
    """y = act(x W1^T + b1) W2^T + b2 with act in {gelu, tanh}: fc1/GELU/fc2 of the encoder block
    (src/v2/modules.py:173-182) and Linear/Tanh/Linear of the classifier (:196-198)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act):
        _need_cuda(x, "mlp")
        K = x.shape[-1]
        Hd, N0 = w1.shape[0], w2.shape[0]
        xb = _bf(x).reshape(-1, K)
        M = xb.shape[0]
        w1b, w2b = _bf(w1), _pad_rows(_bf(w2))
        N = w2b.shape[0]
        b1f, b2f = _f32(b1), _pad_rows(_f32(b2))
        a = torch.empty(M, Hd, dtype=BF, device=x.device)
        z = torch.empty(M, Hd, dtype=BF, device=x.device) if act == 1 else None
        y = torch.empty(M, N, dtype=BF, device=x.device)
        _lib.call("vg_linear_fwd", _lib.ptr(xb), _lib.ptr(w1b), _lib.ptr(b1f), None, _lib.ptr(a), _lib.ptr(z), None, M, Hd, K, act, 0.0, _lib.stream())
        _lib.call("vg_linear_fwd", _lib.ptr(a), _lib.ptr(w2b), _lib.ptr(b2f), None, _lib.ptr(y), None, None, M, N, Hd, 0, 0.0, _lib.stream())
        ctx.save_for_backward(xb, w1b, w2b, a, z if z is not None else a)
        ctx.dims = (M, K, Hd, N, N0, act, x.shape, x.dtype)
        return y[:, :N0].reshape(x.shape[:-1] + (N0,)).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xb, w1b, w2b, a, z = ctx.saved_tensors
        M, K, Hd, N, N0, act, xshape, xdtype = ctx.dims
        dyb = _bf(dy).reshape(M, N0)
        if N != N0:
            t = torch.zeros(M, N, dtype=BF, device=dy.device)
            t[:, :N0] = dyb
            dyb = t
        dz = torch.empty(M, Hd, dtype=BF, device=dy.device)
        mode = 4 if act == 1 else 6  # gelu'(z) / 1 - tanh^2
        _lib.call("vg_linear_dgrad", _lib.ptr(dyb), _lib.ptr(w2b), _lib.ptr(dz), M, N, Hd, mode, _lib.ptr(z), None, 0.0, _lib.stream())
        dx = torch.empty(M, K, dtype=BF, device=dy.device)
        _lib.call("vg_linear_dgrad", _lib.ptr(dz), _lib.ptr(w1b), _lib.ptr(dx), M, Hd, K, 0, None, None, 0.0, _lib.stream())
        dW2 = _wgrad(dyb, a, M, N, Hd)[:N0]
        db2 = _bias_grad(dyb, M, N)[:N0]
        dW1 = _wgrad(dz, xb, M, Hd, K)
        db1 = _bias_grad(dz, M, Hd)
        return dx.reshape(xshape).to(xdtype), dW1, db1, dW2, db2, None


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm(E), eps 1e-5 (src/v2/modules.py:168,172,225)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _need_cuda(x, "layernorm")
        E = x.shape[-1]
        xb = _bf(x).reshape(-1, E)
        R = xb.shape[0]
        g, b = _f32(gamma), _f32(beta)
        y = torch.empty(R, E, dtype=BF, device=x.device)
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        _lib.call("vg_layernorm_fwd", _lib.ptr(xb), E, _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), E, _lib.ptr(mean), _lib.ptr(rstd), R, E, eps, _lib.stream())
        ctx.save_for_backward(xb, g, mean, rstd)
        ctx.dims = (R, E, x.shape, x.dtype)
        return y.reshape(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xb, g, mean, rstd = ctx.saved_tensors
        R, E, xshape, xdtype = ctx.dims
        dyb = _bf(dy).reshape(R, E)
        parts = _lib.lib().vg_layernorm_bwd_parts(R)
        part = torch.empty(parts, 3 * E, dtype=torch.float32, device=dy.device)
        dx = torch.empty(R, E, dtype=BF, device=dy.device)
        _lib.call("vg_layernorm_bwd", _lib.ptr(dyb), _lib.ptr(xb), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(g), None, _lib.ptr(dx), _lib.ptr(part), R, E,
                  _lib.stream())
        dg = torch.empty(E, dtype=torch.float32, device=dy.device)
        db = torch.empty(E, dtype=torch.float32, device=dy.device)
        _lib.call("vg_colsum_f32", _lib.ptr(part), parts, 3 * E, _lib.ptr(dg), E, _lib.ptr(db), E, None, E, None, 0, 0, _lib.stream())
        return dx.reshape(xshape).to(xdtype), dg, db, None


class AttentionFn(torch.autograd.Function):
    """softmax(scale * score(q, k)) v over heads; qkv [B,S,3E] (Q|K|V thirds, head-major) -> [B,S,E].
    lp = 1: score = q k^T (src/v2/modules.py:142-159, v1 attention.py:69-70); lp = 2: score = cdist(q, k), the v1
    discriminator's L2 attention (attention.py:66-67)."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, lp=1):
        _need_cuda(qkv, "attention")
        if lp not in (1, 2):
            raise ValueError(f"Unsupported norm for attention: lp={lp} but should be 1 or 2")
        B, S, E3 = qkv.shape
        E = E3 // 3
        HE = E // heads
        qb = _bf(qkv).reshape(B * S, E3)
        out = torch.empty(B * S, E, dtype=BF, device=qkv.device)
        lse = torch.empty(B, heads, S, dtype=torch.float32, device=qkv.device)
        _lib.call("vg_attention_fwd" if lp == 1 else "vg_attention_l2_fwd", _lib.ptr(qb), _lib.ptr(out), _lib.ptr(lse), B, heads, S, HE, scale, _lib.stream())
        ctx.save_for_backward(qb, out, lse)
        ctx.dims = (B, heads, S, HE, scale, qkv.dtype, lp)
        return out.reshape(B, S, E).to(qkv.dtype)

    @staticmethod
    def backward(ctx, dout):
        qb, out, lse = ctx.saved_tensors
        B, H, S, HE, scale, dt, lp = ctx.dims
        dob = _bf(dout).reshape(B * S, H * HE)
        dqkv = torch.empty_like(qb)
        _lib.call("vg_attention_bwd" if lp == 1 else "vg_attention_l2_bwd", _lib.ptr(qb), _lib.ptr(out), _lib.ptr(dob), _lib.ptr(lse), _lib.ptr(dqkv), B, H, S,
                  HE, scale, _lib.stream())
        return dqkv.reshape(B, S, 3 * H * HE).to(dt), None, None, None


class UnfoldTokensFn(torch.autograd.Function):
    """v1 overlapping-window tokeniser (src/v1/patch_encoder.py:54-73): [B,C,IH,IH] -> [B, n*n, C*W*W], the reference's
    flat view of the double unfold; backward gathers every covering window per pixel."""

    @staticmethod
    def forward(ctx, images, patch, overlap):
        _need_cuda(images, "unfold_tokens")
        B, C, IH, IW = images.shape
        assert IH == IW, "The provided images are not square shaped"
        W = patch + 2 * overlap
        stride = (IH - patch - 2 * overlap) // patch + 1
        n = (IH - (W - 1) - 1) // stride + 1
        is_bf = images.dtype == BF
        src = images.contiguous() if is_bf else images.float().contiguous()
        out = torch.empty(B, n * n, C * W * W, dtype=BF, device=images.device)
        _lib.call("vg_unfold_tokens_fwd", _lib.ptr(src), int(is_bf), _lib.ptr(out), B, C, IH, patch, overlap, _lib.stream())
        ctx.geo = (B, C, IH, patch, overlap, images.dtype)
        return out.to(images.dtype)

    @staticmethod
    def backward(ctx, dtok):
        B, C, IH, patch, overlap, dt = ctx.geo
        d = _bf(dtok).contiguous()
        dimg = torch.empty(B, C, IH, IH, dtype=BF, device=dtok.device)
        _lib.call("vg_unfold_tokens_bwd", _lib.ptr(d), _lib.ptr(dimg), B, C, IH, patch, overlap, _lib.stream())
        return dimg.to(dt), None, None


def unfold_tokens(images, patch: int, overlap: int):
    return UnfoldTokensFn.apply(images, patch, overlap)


def linear(x, weight, bias=None, res=None):
    return LinearFn.apply(x, weight, bias, res)


def mlp(x, w1, b1, w2, b2, act: str):
    return MlpFn.apply(x, w1, b1, w2, b2, {"gelu": 1, "tanh": 3}[act])


def layer_norm(x, gamma, beta, eps: float = 1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


def attention(qkv, heads: int, scale: Optional[float] = None, lp: int = 1):
    if scale is None:
        scale = 1.0 / math.sqrt(qkv.shape[-1] // 3 // heads)
    return AttentionFn.apply(qkv, heads, scale, lp)


AUG_MEMBERS = {"color": 1, "translation": 2, "cutout": 4}  # policy bits of vg_diffaug_fwd


def parse_aug_policy(policy) -> int:
    """``"color,translation,cutout"`` (any comma-separated subset, "" = none) or the bit mask itself -> the policy bits."""
    if isinstance(policy, int) and not isinstance(policy, bool):
        if not 0 <= policy <= 7:
            raise ValueError(f"augmentation policy bits must be in [0, 7], got {policy}")
        return policy
    if not isinstance(policy, str):
        raise ValueError(f"augmentation policy must be a comma-separated subset of {', '.join(AUG_MEMBERS)}, got {policy!r}")
    bits = 0
    for name in (s.strip() for s in policy.split(",")):
        if name == "" and policy.strip() == "":
            continue
        if name not in AUG_MEMBERS:
            raise ValueError(f"unknown augmentation {name!r}: the policy is a comma-separated subset of {', '.join(AUG_MEMBERS)}")
        bits |= AUG_MEMBERS[name]
    return bits


def parse_aug_p(aug_p) -> float:
    """The application probability of the augmentation members as a float in [0, 1]; anything else (NaN included) is a ValueError."""
    try:
        p = float(aug_p)
    except (TypeError, ValueError):
        raise ValueError(f"aug_p must be a probability in [0, 1], got {aug_p!r}") from None
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"aug_p must be a probability in [0, 1], got {aug_p!r}")
    return p


def parse_ada_options(aug_p, ada_target, ada_interval, ada_kimg, policy: int, loss: str):
    """``(aug_p0, ada_target, ada_interval, ada_kimg)`` of the gated augmentation and its controller, checked as GanEngine and
    train_model both state them; ``policy`` is the parsed ``diffaug`` mask.  ``aug_p0`` is None when neither ``aug_p`` nor ADA is on
    (the ungated kernels), else the fixed or starting probability (``aug_p=None``: 1.0 without ADA, 0.0 with it)."""
    try:
        target, kimg = float(ada_target), float(ada_kimg)
    except (TypeError, ValueError):
        raise ValueError(f"ada_target and ada_kimg are numbers, got {ada_target!r}, {ada_kimg!r}") from None
    if not 0.0 <= target < 1.0:
        raise ValueError(f"ada_target must be in [0, 1) (0 = no adaptive augmentation), got {ada_target!r}")
    ada = target > 0.0
    if (aug_p is not None or ada) and not policy:
        raise ValueError("aug_p / ada_target: the augmentation probability gates the members of diffaug; name them in diffaug")
    p0 = parse_aug_p(aug_p) if aug_p is not None else (0.0 if ada else None)
    if isinstance(ada_interval, bool) or not isinstance(ada_interval, int) or ada_interval < 1:
        raise ValueError(f"ada_interval must be a positive integer, got {ada_interval!r}")
    if not (0.0 < kimg < float("inf")):
        raise ValueError(f"ada_kimg must be positive and finite, got {ada_kimg!r}")
    if ada and loss == "wasserstein":
        raise ValueError("ada_target: a Wasserstein critic's sign carries no overfitting signal; use loss='ns' or 'hinge', or a fixed aug_p")
    return p0, target, int(ada_interval), kimg


class DiffAugmentFn(torch.autograd.Function):
    """T = cutout o translation o contrast o saturation o brightness per image (include/vitgan_hip.h, vg_diffaug_fwd); T is affine
    in x, so the backward is the adjoint kernel on dy with the same (policy, seed, site, step) and nothing is saved.  With ``p`` (a
    one-element cuda fp32 tensor) the gated kernels vg_diffaug_p_fwd / vg_diffaug_p_bwd run instead."""

    @staticmethod
    def forward(ctx, x, policy, seed, site, step, p=None):
        _need_cuda(x, "diff_augment")
        B, Cc, IH, IW = x.shape
        assert IH == IW, "The provided images are not square shaped"
        if step is not None and (not step.is_cuda or step.dtype != torch.int32):
            raise ValueError("diff_augment: step is the device step counter, a cuda int32 tensor")
        xb = _bf(x)
        y = torch.empty_like(xb)
        if p is None:
            _lib.call("vg_diffaug_fwd", _lib.ptr(xb), _lib.ptr(y), None, B, Cc, IH, policy, seed, site, _lib.ptr(step), _lib.stream())
        else:
            _lib.call("vg_diffaug_p_fwd", _lib.ptr(xb), _lib.ptr(y), None, B, Cc, IH, policy, seed, site, _lib.ptr(step), _lib.ptr(p), _lib.stream())
        # the adjoint must see the counter value (and the probability) of THIS forward, whatever the caller does to them before backward()
        ctx.key = (policy, seed, site, None if step is None else step.clone(), x.dtype, None if p is None else p.clone())
        return y.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        policy, seed, site, step, dt, p = ctx.key
        B, Cc, IH, _ = dy.shape
        d = _bf(dy)
        dx = torch.empty_like(d)
        if p is None:
            _lib.call("vg_diffaug_bwd", _lib.ptr(d), _lib.ptr(dx), 0, B, Cc, IH, policy, seed, site, _lib.ptr(step), _lib.stream())
        else:
            _lib.call("vg_diffaug_p_bwd", _lib.ptr(d), _lib.ptr(dx), 0, B, Cc, IH, policy, seed, site, _lib.ptr(step), _lib.ptr(p), _lib.stream())
        return dx.to(dt), None, None, None, None, None


def diff_augment(x, policy, seed: int, site: int, step: Optional[torch.Tensor] = None, p=None):
    """Differentiable augmentation of images [B, C, IH, IH]: ``policy`` a comma-separated subset of color, translation, cutout (or
    its bit mask); the transform of image n is a pure function of (seed, site, step[0], n) - ``step``: a cuda int32 counter, or None.
    ``p``: None = every member on every image (vg_diffaug_fwd); a float in [0, 1] or a one-element cuda fp32 tensor = every member
    applied per image with that probability (vg_diffaug_p_fwd: the kernel reads the tensor itself, so a captured launch follows it)."""
    policy = parse_aug_policy(policy)
    if p is not None:
        if torch.is_tensor(p):
            if p.numel() != 1 or p.dtype != torch.float32 or p.device != x.device:
                raise ValueError("diff_augment: p as a tensor is ONE fp32 element on the images' device")
            p = p.detach().reshape(1)
        else:
            p = parse_aug_p(p)
            _need_cuda(x, "diff_augment")
            p = torch.full((1,), p, dtype=torch.float32, device=x.device)
    return DiffAugmentFn.apply(x, policy, int(seed) & 0xFFFFFFFFFFFFFFFF, int(site), step, p)


def parse_bcr_weights(bcr):
    """``(lambda_real, lambda_fake)`` of the consistency loss -> two floats; negative or non-finite weights are a ValueError."""
    try:
        w_real, w_fake = (float(v) for v in bcr)
    except (TypeError, ValueError):
        raise ValueError(f"bcr must be a pair of weights (lambda_real, lambda_fake), got {bcr!r}") from None
    if not (math.isfinite(w_real) and math.isfinite(w_fake) and w_real >= 0.0 and w_fake >= 0.0):
        raise ValueError(f"bcr: the weights (lambda_real, lambda_fake) must be finite and non-negative, got {bcr!r}")
    return w_real, w_fake


def parse_r1_options(gamma, interval, gp_weight=0.0):
    """``(r1_gamma, r1_interval)`` of the R1 penalty and its lazy schedule, checked as GanEngine and train_model both state them:
    gamma finite and >= 0 (0 = off), interval a positive integer - and 1 when the penalty is off; not together with ``gp_weight``."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"r1_gamma must be a finite, non-negative number, got {gamma!r}") from None
    if not (math.isfinite(g) and g >= 0.0):
        raise ValueError(f"r1_gamma must be a finite, non-negative number, got {gamma!r}")
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise ValueError(f"r1_interval must be a positive integer, got {interval!r}")
    if interval != 1 and g == 0.0:
        raise ValueError(f"r1_interval={interval!r} without a penalty (r1_gamma=0) would do nothing; set r1_gamma")
    if g > 0.0 and float(gp_weight) != 0.0:
        raise ValueError("r1_gamma: one gradient penalty per step - R1 and gp_weight share the penalty workspaces; switch one of them off")
    return g, int(interval)


def r1_due(step_index: int, interval: int) -> bool:
    """Lazy regularisation: is the R1 penalty due on step ``step_index`` (1-based: the engine's ``steps`` after its increment)?  The
    first step of a run is due, then every ``interval``-th one after it."""
    return (int(step_index) - 1) % int(interval) == 0


LR_KINDS = _lib.LR_KINDS  # VG_LR_* of include/vitgan_hip.h: {"constant": 0, "linear": 1, "cosine": 2}


def parse_lr_schedule(kind, warmup, total, final):
    """``(kind, warmup, total, final)`` of the learning-rate schedule, checked as GanEngine and train_model both state them, or None when
    no schedule is asked for (``kind=""`` and ``warmup=0``: the rates stay host floats).  kind: "" | "constant" | "linear" | "cosine" -
    "" with a warm-up means "constant"; warmup: a non-negative integer, the steps of linear warm-up; total: a non-negative integer, the
    step from which the factor is ``final`` - a decaying kind needs total > warmup; final: a number in [0, 1].  A constant schedule
    reads neither total nor final: they come back as 0 and 0.0, so two such runs carry the same options."""
    if not isinstance(kind, str) or (kind and kind not in LR_KINDS):
        raise ValueError(f"lr_schedule must be one of '', {', '.join(repr(k) for k in LR_KINDS)}, got {kind!r}")
    for name, v in (("lr_warmup", warmup), ("lr_total", total)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
            raise ValueError(f"{name} must be a non-negative integer (steps), got {v!r}")
    try:
        fin = float(final)
    except (TypeError, ValueError):
        raise ValueError(f"lr_final must be a number in [0, 1], got {final!r}") from None
    if not 0.0 <= fin <= 1.0:
        raise ValueError(f"lr_final must be a number in [0, 1] (the factor from lr_total on), got {final!r}")
    if not kind and warmup == 0:
        if total != 0 or fin != 0.0:
            raise ValueError(f"lr_total={total!r} / lr_final={final!r} without a schedule would do nothing; name one in lr_schedule")
        return None
    kind = kind or "constant"
    if kind == "constant":
        return kind, int(warmup), 0, 0.0
    if total <= warmup:
        raise ValueError(f"lr_schedule={kind!r}: the decay runs from step lr_warmup to step lr_total and needs lr_total > lr_warmup, "
                         f"got lr_total={total!r}, lr_warmup={warmup!r}")
    return kind, int(warmup), int(total), fin


def lr_sched_struct(base, kind, warmup, total, final) -> "_lib.VgLrSched":
    """One slot's VgLrSched from a base rate and a parsed schedule (``parse_lr_schedule``'s tuple; the kind by name or number)."""
    return _lib.VgLrSched(float(base), LR_KINDS.get(kind, kind), int(warmup), int(total), float(final))


def lr_schedule(step: torch.Tensor, d, g, scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The two learning rates in force at the device step counter ``step`` (a cuda int32 tensor; a value below 1 counts as 1), one
    vg_lr_schedule launch: ``d`` / ``g`` = (base, kind, warmup, total, final) of slot 0 (the discriminator) and slot 1 (the generator),
    ``scale``: the two device multipliers (fp32 [2]; None = ones), ``out``: fp32 [2] to write (returned; None = a fresh tensor).
    Every argument the kernel would misread is refused by the C call (HipError, argument validation)."""
    if not torch.is_tensor(step) or not step.is_cuda or step.dtype != torch.int32 or step.numel() < 1:
        raise ValueError("lr_schedule: step is the device step counter, a cuda int32 tensor")
    for name, t in (("scale", scale), ("out", out)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != 2 or not t.is_contiguous() or t.device != step.device):
            raise ValueError(f"lr_schedule: {name} is a contiguous fp32 tensor of two elements on the counter's device")
    scale = torch.ones(2, dtype=torch.float32, device=step.device) if scale is None else scale
    out = torch.empty(2, dtype=torch.float32, device=step.device) if out is None else out
    sd, sg = lr_sched_struct(*d), lr_sched_struct(*g)
    _lib.call("vg_lr_schedule", C.byref(sd), C.byref(sg), _lib.ptr(step), _lib.ptr(scale), _lib.ptr(out), _lib.stream())
    return out


def parse_telemetry(telemetry) -> int:
    """``GanEngine(telemetry=...)``: the capacity of the per-step rings, an integer >= 1, or 0 (the default) for none.  Anything else -
    a bool, a float, a negative number - is the caller's error; host only."""
    if isinstance(telemetry, bool) or not isinstance(telemetry, int) or not 0 <= telemetry < 2 ** 24:
        raise ValueError(f"telemetry must be 0 (off) or the ring capacity, an integer >= 1 (steps kept between two history() calls), got {telemetry!r}")
    return int(telemetry)


GRAD_CHUNK = 4096  # elements per chunk of vg_grad_stats at most


def grad_chunks(slots, limit: int = GRAD_CHUNK):
    """The chunk table of vg_grad_stats from a slot table (``flat.vit_slots`` / ``flat.gen_slots`` / a FlatParams' ``slots``, the class
    table included when it has one): ``(chunks, seg_first, keys)`` - chunks int32 [n_chunks, 3] = (first element, count, segment) with
    count <= ``limit``, seg_first int32 [n_seg + 1], keys the segment names.  One segment per slot in the table's own order (the
    state_dict's); a chunk never crosses a slot, the chunks of a slot are adjacent and ascending, and nothing between two slots (the
    layouts' alignment padding) is covered.  Host only (numpy)."""
    import numpy as np
    if isinstance(limit, bool) or not isinstance(limit, int) or not 1 <= limit <= GRAD_CHUNK:
        raise ValueError(f"grad_chunks: limit must be in [1, {GRAD_CHUNK}], got {limit!r}")
    rows, seg_first, keys = [], [0], []
    for s, (key, (off, shape)) in enumerate(slots.items()):
        n = 1
        for d in shape:
            n *= int(d)
        if n < 1 or off < 0 or off + n >= 2 ** 31:
            raise ValueError(f"grad_chunks: slot {key!r} = ({off}, {tuple(shape)}) is empty or outside a 2^31-element buffer")
        starts = np.arange(int(off), int(off) + n, limit, dtype=np.int64)
        counts = np.minimum(limit, int(off) + n - starts)
        rows.append(np.stack([starts, counts, np.full_like(starts, s)], axis=1))
        seg_first.append(seg_first[-1] + len(starts))
        keys.append(key)
    if not rows:
        raise ValueError("grad_chunks: an empty slot table")
    return np.concatenate(rows).astype(np.int32), np.asarray(seg_first, dtype=np.int32), keys


class GradStatsPlan:
    """The device side of one buffer's vg_grad_stats: the chunk table, the segment index, the scratch and the outputs, allocated once."""

    def __init__(self, slots, total: int, device, limit: int = GRAD_CHUNK):
        chunks, seg_first, self.keys = grad_chunks(slots, limit)
        self.total, self.n_chunks, self.n_seg = int(total), int(chunks.shape[0]), len(self.keys)
        if int((chunks[:, 0].astype("int64") + chunks[:, 1]).max()) > self.total:
            raise ValueError("grad_stats: a slot ends behind the buffer")
        self.chunks = torch.from_numpy(chunks).to(device).contiguous()
        self.seg_first = torch.from_numpy(seg_first).to(device)
        self.scratch = torch.zeros(2 * self.n_chunks, dtype=torch.float32, device=device)
        self.norm_seg = torch.zeros(self.n_seg, dtype=torch.float32, device=device)
        self.totals = torch.zeros(4, dtype=torch.float32, device=device)  # (sum of norms, l2, non-finite elements, 0)

    def enqueue(self, grad: torch.Tensor, gscale: float, st) -> None:
        _lib.call("vg_grad_stats", _lib.ptr(grad), self.total, _lib.ptr(self.chunks), self.n_chunks, _lib.ptr(self.seg_first), self.n_seg, float(gscale),
                  _lib.ptr(self.scratch), _lib.ptr(self.norm_seg), _lib.ptr(self.totals), st)


def grad_stats(flat_grad: torch.Tensor, slots, gscale: float = 1.0, limit: int = GRAD_CHUNK):
    """Per-tensor gradient norms of one flat fp32 gradient buffer (vg_grad_stats; nothing synchronises): a dict with ``norms``
    [n_seg] = gscale ||g_s||_2 per slot of ``slots`` in its order, ``keys``, and the device scalars ``sum_norms`` (the sum of those,
    ``sum(p.grad.norm() for p in parameters)``), ``l2`` (the norm of the whole gradient, what ``clip_grad_norm_`` sees) and
    ``nonfinite`` (NaN / Inf elements, saturating at 2^24).  Padding between slots is never read."""
    _need_cuda(flat_grad, "grad_stats")
    if flat_grad.dtype != torch.float32 or flat_grad.dim() != 1 or not flat_grad.is_contiguous():
        raise ValueError("grad_stats: flat_grad is a contiguous one-dimensional fp32 tensor")
    plan = GradStatsPlan(slots, flat_grad.numel(), flat_grad.device, limit)
    plan.enqueue(flat_grad, gscale, _lib.stream())
    return {"norms": plan.norm_seg, "keys": plan.keys, "sum_norms": plan.totals[0], "l2": plan.totals[1], "nonfinite": plan.totals[2]}


def logit_stats(x: torch.Tensor):
    """``(mean, frac_pos, frac_neg)`` of the logits ``x`` (any shape, 1 to 16384 elements), a device tensor of three floats
    (vg_logit_stats): the fractions of elements > 0 and < 0 - exact zeros and NaN count in neither."""
    _need_cuda(x, "logit_stats")
    xs = _f32(x).reshape(-1)
    out = torch.zeros(3, 4, dtype=torch.float32, device=x.device)
    _lib.call("vg_logit_stats", _lib.ptr(xs), None, xs.numel(), 0, _lib.ptr(out), _lib.stream())
    return out[0, :3]


class ConsistencyLossFn(torch.autograd.Function):
    """Balanced consistency regularisation between D(x) and D(T(x)) (include/vitgan_hip.h, vg_bcr_loss): one launch computes both segment
    means and both gradients, so the backward only scales what the forward saved."""

    @staticmethod
    def forward(ctx, logits_x, logits_a, n_real, w_real, w_fake):
        _need_cuda(logits_x, "consistency_loss")
        if logits_x.shape != logits_a.shape or logits_x.dim() != 2 or logits_a.device != logits_x.device:
            raise ValueError("consistency_loss: logits_x and logits_a are [n, Kc] tensors of one shape on one device")
        n, Kc = logits_x.shape
        if not 0 < n_real < n:
            raise ValueError(f"consistency_loss: n_real must leave a real and a fake segment, got {n_real} of {n} rows")
        lx, la = logits_x.detach().float().contiguous(), logits_a.detach().float().contiguous()
        dx, da = torch.empty_like(lx), torch.empty_like(la)
        parts = torch.empty(2, dtype=torch.float32, device=lx.device)
        _lib.call("vg_bcr_loss", _lib.ptr(lx), _lib.ptr(la), _lib.ptr(dx), _lib.ptr(da), _lib.ptr(parts), n_real, n - n_real, Kc, w_real, w_fake, 0, 0, 1.0,
                  _lib.stream())
        ctx.save_for_backward(dx, da)
        ctx.dts = (logits_x.dtype, logits_a.dtype)
        ctx.mark_non_differentiable(parts)
        return w_real * parts[0] + w_fake * parts[1], parts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dparts):
        dx, da = ctx.saved_tensors
        return (dx * dout).to(ctx.dts[0]), (da * dout).to(ctx.dts[1]), None, None, None


def consistency_loss(logits_x, logits_a, n_real: int, w_real: float, w_fake: float):
    """``(loss, parts)``: loss = w_real L_real + w_fake L_fake with L_s = 1/B_s sum_{n in s} |D(x_n) - D(a_n)|^2 over the first ``n_real``
    rows (real) and the rest (fake) of the logits [n, Kc] on a batch and on its augmented partner; ``parts`` = the two unweighted
    means [L_real, L_fake] (not differentiable).  Both inputs receive gradient: there is no stop-gradient."""
    w_real, w_fake = parse_bcr_weights((w_real, w_fake))
    return ConsistencyLossFn.apply(logits_x, logits_a, int(n_real), w_real, w_fake)


# ---- class conditioning (include/vitgan_hip.h: vg_draw_labels, vg_class_add, vg_class_grad, vg_gan_loss_cond)
_LOSS_KINDS = {"ns": 0, "hinge": 1, "wasserstein": 2}
_LOSS_ROLES = {"d_real": 0, "d_fake": 1, "g": 2, 0: 0, 1: 1, 2: 2}


def check_labels(labels, n: int, K: int, what: str, device=None) -> torch.Tensor:
    """``labels`` as the kernels read them - a contiguous int32 [n] tensor - after the host-side checks the wrappers owe their callers:
    an integer dtype, the shape, the device and every value in [0, K).  It reads the values, so it synchronises; the kernels clamp
    on their own and never index with a bad label, so ``GanEngine.step`` does without it."""
    if not torch.is_tensor(labels) or labels.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"{what}: labels must be an integer tensor, got {getattr(labels, 'dtype', type(labels))!r}")
    if labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError(f"{what}: labels must have shape [{n}], got {tuple(labels.shape)}")
    if device is not None and labels.device != device:
        raise ValueError(f"{what}: labels must be on {device}, got {labels.device}")
    if not 1 <= int(K) <= 16:
        raise ValueError(f"{what}: the number of classes must be in [1, 16], got {K!r}")
    if n and (int(labels.min()) < 0 or int(labels.max()) >= K):
        raise ValueError(f"{what}: labels must be in [0, {K}), got values in [{int(labels.min())}, {int(labels.max())}]")
    return labels.detach().to(torch.int32).contiguous()


class ConditionalGanLossFn(torch.autograd.Function):
    """The label-selected loss D(x, y) = D(x)[y] on a K-way head: one launch computes the mean loss and the gradient of every logit
    (+0 off the label), so the backward only scales what the forward saved."""

    @staticmethod
    def forward(ctx, logits, labels, kind, role):
        lg = logits.detach().float().contiguous()
        n, Kc = lg.shape
        dl, sel = torch.empty_like(lg), torch.empty(n, dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        _lib.call("vg_gan_loss_cond", _lib.ptr(lg), _lib.ptr(labels), _lib.ptr(dl), _lib.ptr(sel), _lib.ptr(out), n, Kc, kind, role, 1.0, _lib.stream())
        ctx.save_for_backward(dl)
        ctx.dt = logits.dtype
        ctx.mark_non_differentiable(sel)
        return out[0], sel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dsel):
        (dl,) = ctx.saved_tensors
        return (dl * dout).to(ctx.dt), None, None, None


def conditional_gan_loss(logits, labels, kind="ns", role="d_real", return_selected: bool = False):
    """The GAN loss of ``kind`` ("ns", "hinge", "wasserstein") in ``role`` ("d_real" / 0, "d_fake" / 1, "g" / 2) on the label-selected
    logits s_i = logits[i, labels[i]] of a [n, Kc] head: the mean over the n samples, differentiable in ``logits``.  ``labels``: an
    integer tensor [n] on the logits' device, every value in [0, Kc) (checked here: this call synchronises).  ``return_selected``
    also returns s (not differentiable)."""
    _need_cuda(logits, "conditional_gan_loss")
    if logits.dim() != 2:
        raise ValueError("conditional_gan_loss: logits is a [n, Kc] tensor")
    if kind not in _LOSS_KINDS or role not in _LOSS_ROLES:
        raise ValueError(f"conditional_gan_loss: kind must be one of {sorted(_LOSS_KINDS)} and role one of d_real, d_fake, g")
    y = check_labels(labels, logits.shape[0], logits.shape[1], "conditional_gan_loss", logits.device)
    loss, sel = ConditionalGanLossFn.apply(logits, y, _LOSS_KINDS[kind], _LOSS_ROLES[role])
    return (loss, sel) if return_selected else loss


def draw_labels(n: int, K: int, seed: int, site: int, step: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """``n`` class labels uniform over [0, K), int32 on the device: a pure function of (seed, site, step[0], index) - ``step``: a cuda
    int32 counter (its device is the result's), or None with ``device``."""
    if step is not None and (not step.is_cuda or step.dtype != torch.int32):
        raise ValueError("draw_labels: step is the device step counter, a cuda int32 tensor")
    if n < 1 or not 1 <= int(K) <= 16:
        raise ValueError(f"draw_labels: n >= 1 and 1 <= K <= 16, got n={n!r}, K={K!r}")
    dev = step.device if step is not None else torch.device("cuda" if device is None else device)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("vg_draw_labels", _lib.ptr(out), n, int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(site), _lib.ptr(step), _lib.stream())
    return out


def class_add(wmod, table, labels):
    """wmod [B, N] + table[labels] ([K, N]) in bf16 with fp32 addition (vg_class_add, out of place here): a new bf16 tensor."""
    _need_cuda(wmod, "class_add")
    if wmod.dim() != 2 or table.dim() != 2 or table.shape[1] != wmod.shape[1] or wmod.shape[1] % 8:
        raise ValueError("class_add: wmod [B, N] and table [K, N] with N % 8 == 0")
    y = check_labels(labels, wmod.shape[0], table.shape[0], "class_add", wmod.device)
    out, tb = _bf(wmod).clone(), _bf(table)
    _lib.call("vg_class_add", _lib.ptr(out), _lib.ptr(tb), _lib.ptr(y), out.shape[0], out.shape[1], tb.shape[0], _lib.stream())
    return out


def class_grad(dw, labels, K: int, out: Optional[torch.Tensor] = None):
    """The class table's gradient [K, N] of dw [B, N] fp32: row k = the sum of the rows of class k in ascending order (vg_class_grad).
    ``out``: an fp32 [K, N] tensor to ACCUMULATE into (returned); None = a fresh tensor, overwritten."""
    _need_cuda(dw, "class_grad")
    if dw.dim() != 2 or dw.shape[1] % 4:
        raise ValueError("class_grad: dw is [B, N] with N % 4 == 0")
    y = check_labels(labels, dw.shape[0], K, "class_grad", dw.device)
    d = _f32(dw)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (K, d.shape[1]) or not out.is_contiguous() or out.device != d.device):
        raise ValueError(f"class_grad: out is a contiguous fp32 [{K}, {d.shape[1]}] tensor on the gradient's device")
    res = torch.empty(K, d.shape[1], dtype=torch.float32, device=d.device) if out is None else out
    _lib.call("vg_class_grad", _lib.ptr(d), _lib.ptr(y), _lib.ptr(res), d.shape[0], d.shape[1], int(K), int(out is not None), _lib.stream())
    return res


def _spectral_one(W, u, sigma0):
    """A one-matrix SpectralState holding (u, sigma0) for the fp32 matrix W [N, K] (a contiguous cuda tensor)."""
    from .spectral import SpectralState
    _need_cuda(W, "spectral")
    if W.dim() != 2 or W.dtype != torch.float32 or not W.is_contiguous():
        raise ValueError("spectral: W is a contiguous fp32 [N, K] matrix")
    N, K = W.shape
    st = SpectralState([(0, N, K)], N * K, W.device)
    st.u(0).copy_(u.reshape(N))
    st.sigma0(0).fill_(float(sigma0))
    return st


def spectral_sigma(W, u):
    """One power iteration on W [N, K] from u [N] (vg_spectral_update): (sigma, u', v') with v' = W^T u / |W^T u|, sigma = |W v'|,
    u' = W v' / sigma."""
    st = _spectral_one(W, u, 1.0)
    st.update(W.reshape(-1), torch.empty(W.numel(), dtype=torch.bfloat16, device=W.device))
    return st.sigma(0).clone(), st.u(0).clone(), st.v(0).clone()


def spectral_normalize(W, u, sigma0, grad=None):
    """The same iteration and the normalised bf16 shadow bf16(fp32(sigma0 / sigma) * W).  With ``grad`` = dL/dW_eff [N, K] also the
    raw-weight gradient s (G - (<G, W> / sigma) u' v'^T) from the pair that produced the shadow (vg_spectral_project).
    Returns (shadow, sigma, u', v') or (shadow, sigma, u', v', projected)."""
    st = _spectral_one(W, u, sigma0)
    shadow = torch.empty(W.numel(), dtype=torch.bfloat16, device=W.device)
    st.update(W.reshape(-1), shadow)
    out = (shadow.view_as(W), st.sigma(0).clone(), st.u(0).clone(), st.v(0).clone())
    if grad is None:
        return out
    g = grad.detach().to(torch.float32).contiguous().clone().reshape(-1)
    st.project(g, W.reshape(-1))
    return out + (g.view_as(W),)
