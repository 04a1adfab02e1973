"""An on-device Frechet distance: the quality score behind ``train_model``'s ``FID:`` field, best-FID checkpoints and ``lr_plateau``.

The reference scores a run with torchmetrics' ``FrechetInceptionDistance`` on fetched Inception weights (src/v2/utils.py:155-175).
The weights are the one part that cannot be had offline; the rest of the metric is arithmetic, and it lives here:

  * ``FeatureMoments``: streaming fp64 first and second moments of feature vectors.  On the device the update is ONE launch of
    ``vg_moments_update`` (csrc/metrics.hip: fp64 MFMA, no fp64 copy of the batch, deterministic) and the mean / covariance come from
    ``vg_moments_finish``; a CPU tensor takes a plain torch-fp64 path with the same formulas, for host-side use and tests.  Sums are
    what make the metric data-parallel: ``all_reduce`` is one fp64 all-reduce of ``sum | gram | n``.
  * ``frechet_distance``: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) on the host in fp64, the last term in its symmetric
    form (two ``eigh``; no device ``linalg``, no complex arithmetic).
  * ``FrechetDistance``: the evaluator, callable as ``fid_fn(gan, epoch) -> float``.  The feature network is a FROZEN ViT on this
    project's own kernels (``vg_vit_features``: the tensor the classifier's fc1 reads) - by default a fixed-seed randomly
    initialised one (``FrechetDistance.random_vit``), random-embedding Frechet distances as in Naeem et al. 2020 - or any callable
    ``images -> [n, d]``: with Inception weights on disk the same accumulator gives the true FID.

A random-ViT distance ranks the checkpoints of a run against each other; it is NOT comparable with published FID numbers.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import Any, Callable, Dict, Iterable, Optional, Union

import numpy as np
import torch
from torch import nn

from . import _lib
from .config import Config
from .data import DeviceDataset

D_MIN, D_MAX = 16, 2048  # vg_moments_update: d % 16 == 0 inside these


def _check_d(d: int) -> int:
    if isinstance(d, bool) or int(d) != d or not D_MIN <= int(d) <= D_MAX or int(d) % 16:
        raise ValueError(f"the feature width must be a multiple of 16 in [{D_MIN}, {D_MAX}] (vg_moments_update), got {d!r}")
    return int(d)


class FeatureMoments:
    """Streaming fp64 moments of [n, d] feature batches: ``sum`` [d], ``gram`` = sum_i x_i (x) x_i [d, d] and the count ``n``, in one
    fp64 buffer ``sum | gram | n`` on ``device``.  ``mean`` = sum / n and ``cov`` = (gram - n mean (x) mean) / (n - 1), torchmetrics'
    one-pass formula, are computed on request.  Nothing is kept per sample."""

    def __init__(self, d: int, device="cpu"):
        self.d = _check_d(d)
        self._buf = torch.zeros(self.d + self.d * self.d + 1, dtype=torch.float64, device=torch.device(device))
        self.device = self._buf.device  # with its index: "cuda" is the current device
        self._n = 0

    # -- views ---------------------------------------------------------------------------------
    @property
    def sum(self) -> torch.Tensor:
        return self._buf[:self.d]

    @property
    def gram(self) -> torch.Tensor:
        return self._buf[self.d:self.d + self.d * self.d].view(self.d, self.d)

    @property
    def n(self) -> int:
        return self._n

    # -- accumulation ----------------------------------------------------------------------------
    def update(self, feats: torch.Tensor) -> "FeatureMoments":
        """``feats``: [n, d] fp32 (bf16 and fp16 are widened first), any n >= 1, on this accumulator's device."""
        if feats.dim() != 2 or feats.shape[1] != self.d or feats.shape[0] < 1:
            raise ValueError(f"update: features must be [n >= 1, {self.d}], got {tuple(feats.shape)}")
        if feats.dtype in (torch.bfloat16, torch.float16):
            feats = feats.float()
        if feats.dtype != torch.float32:
            raise TypeError(f"update: features must be fp32, bf16 or fp16, got {feats.dtype}")
        if feats.device != self.device:
            raise ValueError(f"update: the features are on {feats.device}, the accumulator on {self.device}")
        feats = feats.detach()
        n = int(feats.shape[0])
        if self.device.type == "cuda":
            if feats.stride(1) != 1 or feats.stride(0) < self.d:
                feats = feats.contiguous()
            with torch.cuda.device(self.device):
                _lib.call("vg_moments_update", feats.data_ptr(), feats.stride(0), n, self.d, self.sum.data_ptr(), self.gram.data_ptr(), _lib.stream())
        else:
            x = feats.double()
            self.sum.add_(x.sum(0))
            self.gram.add_(x.t() @ x)
        self._n += n
        return self

    def merge(self, other: "FeatureMoments") -> "FeatureMoments":
        """Add another accumulator's sums (same width); moments are additive over disjoint sample sets."""
        if other.d != self.d:
            raise ValueError(f"merge: widths differ, {self.d} and {other.d}")
        self._buf[:-1].add_(other._buf[:-1].to(self.device))
        self._n += other._n
        return self

    def all_reduce(self, group=None) -> "FeatureMoments":
        """Sum the accumulators of every rank of ``group``: one fp64 all-reduce of ``sum | gram | n``."""
        import torch.distributed as dist
        self._buf[-1] = float(self._n)
        dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=group)
        self._n = int(round(float(self._buf[-1])))
        return self

    # -- results -----------------------------------------------------------------------------------
    def _finish(self):
        if self._n < 2:
            raise ValueError(f"mean and covariance need at least 2 samples, the accumulator holds {self._n}")
        if self.device.type == "cuda":
            mean = torch.empty(self.d, dtype=torch.float64, device=self.device)
            cov = torch.empty(self.d, self.d, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.call("vg_moments_finish", self.sum.data_ptr(), self.gram.data_ptr(), self._n, self.d, mean.data_ptr(), cov.data_ptr(), _lib.stream())
            return mean, cov
        nn_ = float(self._n)
        mean = self.sum / nn_
        return mean, (self.gram - nn_ * (mean.unsqueeze(1) * mean.unsqueeze(0))) / (nn_ - 1.0)

    @property
    def mean(self) -> torch.Tensor:
        return self._finish()[0]

    @property
    def cov(self) -> torch.Tensor:
        return self._finish()[1]

    def moments(self):
        """(mean [d], cov [d, d]) as fp64 numpy arrays on the host."""
        mean, cov = self._finish()
        return mean.cpu().numpy(), cov.cpu().numpy()

    # -- persistence ---------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        return {"d": self.d, "n": self._n, "sum": self.sum.detach().cpu().clone(), "gram": self.gram.detach().cpu().clone()}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        if int(state["d"]) != self.d:
            raise ValueError(f"load_state_dict: the state is of width {state['d']}, the accumulator of {self.d}")
        self.sum.copy_(torch.as_tensor(state["sum"], dtype=torch.float64).reshape(self.d))
        self.gram.copy_(torch.as_tensor(state["gram"], dtype=torch.float64).reshape(self.d, self.d))
        self._n = int(state["n"])


def _sym_eigh_clipped(a: np.ndarray):
    w, v = np.linalg.eigh(0.5 * (a + a.T))
    return np.clip(w, 0.0, None), v


def frechet_terms(mu1, cov1, mu2, cov2):
    """(mean_term, trace_term) of the distance below; their sum, clamped at 0, is the distance."""
    mu1, mu2, cov1, cov2 = (np.asarray(torch.as_tensor(t).detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
                            for t in (mu1, mu2, cov1, cov2))
    d = mu1.shape[0]
    if mu1.shape != (d,) or mu2.shape != (d,) or cov1.shape != (d, d) or cov2.shape != (d, d):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {cov1.shape}, {mu2.shape}, {cov2.shape} are not [d], [d, d] twice")
    w, v = _sym_eigh_clipped(cov1)
    r = (v * np.sqrt(w)) @ v.T  # R = cov1^(1/2)
    lam, _ = _sym_eigh_clipped(r @ cov2 @ r)  # the eigenvalues of cov1 cov2, through a symmetric matrix
    diff = mu1 - mu2
    return float(diff @ diff), float(np.trace(cov1) + np.trace(cov2) - 2.0 * np.sqrt(lam).sum())


def frechet_distance(mu1, cov1, mu2, cov2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), on the host in fp64 (tensors are copied to the CPU).  The last term in its
    symmetric form: with R = S1^(1/2) from ``eigh`` (eigenvalues clipped at 0) it is sum sqrt(clip(eigvalsh(R S2 R), 0)) - the same
    eigenvalues as torchmetrics' ``eigvals(S1 S2)``, without complex arithmetic.  Clamped at 0."""
    a, b = frechet_terms(mu1, cov1, mu2, cov2)
    return max(a + b, 0.0)


# ------------------------------------------------------------------------------------------------------------ pairs of features
# What the moments throw away.  Squared Euclidean distances in fp64, every comparison inclusive:
#   rad2_k(x_i; X)  the k-th smallest of { |x_i - x_j|^2 : j != i } - self excluded BY INDEX, a duplicate elsewhere is a neighbour at 0
#   precision       the share of fake g with |g - r_j|^2 <= rad2_k(r_j; R) for some real r_j          (Kynkaanniemi et al. 2019)
#   recall          the share of real r with |r - g_i|^2 <= rad2_k(g_i; G) for some fake g_i          (the same paper)
#   density         1 / (k M) sum_i #{ j : |g_i - r_j|^2 <= rad2_k(r_j; R) }, M fakes                 (Naeem et al. 2020)
#   coverage        the share of real r_j with min_i |r_j - g_i|^2 <= rad2_k(r_j; R)                  (the same paper)
#   KID             the unbiased MMD^2 estimate with kappa(a, b) = (a.b / d + 1)^3 over the FULL sets (Binkowski et al. 2018):
#                   ONE estimate, not the mean over subsets that the paper's code reports
# On the device each is one launch of csrc/pairwise.hip (fp64 MFMA, no n x n buffer); a CPU tensor takes plain torch fp64.
K_MAX = 8  # vg_knn_radii keeps the k smallest in registers


def _check_feats(x: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1:
        raise ValueError(f"{what}: features must be an [n >= 1, d] tensor, got {tuple(getattr(x, 'shape', ())) or type(x).__name__}")
    _check_d(x.shape[1])
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: features must be fp32, bf16 or fp16, got {x.dtype}")
    x = x.detach()
    if x.is_cuda and (x.stride(1) != 1 or x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _check_pair(q: torch.Tensor, c: torch.Tensor, what: str):
    q, c = _check_feats(q, what), _check_feats(c, what)
    if q.shape[1] != c.shape[1]:
        raise ValueError(f"{what}: the widths differ, {q.shape[1]} and {c.shape[1]}")
    if q.device != c.device:
        raise ValueError(f"{what}: the two sets are on {q.device} and {c.device}")
    return q, c


def _check_k(k, n: int, what: str) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K_MAX:
        raise ValueError(f"{what}: k must be an integer in [1, {K_MAX}], got {k!r}")
    if k >= n:
        raise ValueError(f"{what}: k = {k} needs more than k rows, got {n}")
    return k


def _pair_ws(nq: int, nc: int, k: int, device) -> torch.Tensor:
    nbytes = _lib.lib().vg_pair_ws_bytes(nq, nc, k)
    if nbytes <= 0:
        raise RuntimeError("vg_pair_ws_bytes failed")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _cpu_d2(q: torch.Tensor, c: torch.Tensor):
    """blocks (lo, d2 [b, nc]) of squared distances from DIFFERENCES in fp64, at most 2^24 elements at a time"""
    q64, c64 = q.double(), c.double()
    step = max(1, (1 << 24) // max(1, c64.shape[0] * c64.shape[1]))
    for lo in range(0, q64.shape[0], step):
        yield lo, ((q64[lo:lo + step, None, :] - c64[None, :, :]) ** 2).sum(-1)


def knn_radii(x: torch.Tensor, k: int) -> torch.Tensor:
    """fp64 [n]: the squared distance from each row of ``x`` [n, d] to its k-th nearest OTHER row (1 <= k <= 8, k < n)."""
    x = _check_feats(x, "knn_radii")
    n, d = int(x.shape[0]), int(x.shape[1])
    k = _check_k(k, n, "knn_radii")
    if x.is_cuda:
        rad2 = torch.empty(n, dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            ws = _pair_ws(n, n, k, x.device)
            _lib.call("vg_knn_radii", x.data_ptr(), x.stride(0), n, d, k, rad2.data_ptr(), ws.data_ptr(), _lib.stream())
        return rad2
    out = []
    for lo, d2 in _cpu_d2(x, x):
        rows = torch.arange(d2.shape[0])
        d2[rows, lo + rows] = float("inf")
        out.append(torch.kthvalue(d2, k, dim=1).values)
    return torch.cat(out)


def ball_counts(q: torch.Tensor, c: torch.Tensor, rad2_c: torch.Tensor):
    """(count int32 [nq], min_d2 fp64 [nq]): for each row of ``q`` the number of centres ``c_j`` with |q - c_j|^2 <= rad2_c[j], and its
    squared distance to the nearest centre.  No self-exclusion: the two sets are different sets."""
    q, c = _check_pair(q, c, "ball_counts")
    nq, nc, d = int(q.shape[0]), int(c.shape[0]), int(q.shape[1])
    if not torch.is_tensor(rad2_c) or rad2_c.dtype != torch.float64 or tuple(rad2_c.shape) != (nc,) or rad2_c.device != c.device:
        raise ValueError(f"ball_counts: rad2_c must be an fp64 [{nc}] tensor on {c.device}, got {getattr(rad2_c, 'dtype', None)} "
                         f"{tuple(getattr(rad2_c, 'shape', ()))} on {getattr(rad2_c, 'device', None)}")
    rad2_c = rad2_c.detach().contiguous()
    if q.is_cuda:
        count = torch.empty(nq, dtype=torch.int32, device=q.device)
        min_d2 = torch.empty(nq, dtype=torch.float64, device=q.device)
        with torch.cuda.device(q.device):
            ws = _pair_ws(nq, nc, 0, q.device)
            _lib.call("vg_ball_counts", q.data_ptr(), q.stride(0), nq, c.data_ptr(), c.stride(0), nc, d, rad2_c.data_ptr(), count.data_ptr(), min_d2.data_ptr(),
                      ws.data_ptr(), _lib.stream())
        return count, min_d2
    counts, mins = [], []
    for _, d2 in _cpu_d2(q, c):
        counts.append((d2 <= rad2_c[None, :]).sum(1).to(torch.int32))
        mins.append(d2.min(1).values)
    return torch.cat(counts), torch.cat(mins)


def poly_kernel_sum(q: torch.Tensor, c: torch.Tensor, skip_diagonal: bool = False) -> torch.Tensor:
    """fp64 scalar tensor: sum_ij (q_i . c_j / d + 1)^3, with ``skip_diagonal`` without the terms i == j."""
    q, c = _check_pair(q, c, "poly_kernel_sum")
    nq, nc, d = int(q.shape[0]), int(c.shape[0]), int(q.shape[1])
    if q.is_cuda:
        out = torch.empty(1, dtype=torch.float64, device=q.device)
        with torch.cuda.device(q.device):
            ws = _pair_ws(nq, nc, 0, q.device)
            _lib.call("vg_poly_kernel_sum", q.data_ptr(), q.stride(0), nq, c.data_ptr(), c.stride(0), nc, d, int(bool(skip_diagonal)), out.data_ptr(),
                      ws.data_ptr(), _lib.stream())
        return out[0]
    kap = (q.double() @ c.double().t() / float(d) + 1.0) ** 3
    total = kap.sum()
    return total - torch.diagonal(kap).sum() if skip_diagonal else total


def _prdc_from(count_g: torch.Tensor, count_r: torch.Tensor, min_r: torch.Tensor, rad2_r: torch.Tensor, k: int) -> Dict[str, float]:
    """the four ratios from the two launches' outputs: integer counts over integer sizes, one division each"""
    M, N = int(count_g.shape[0]), int(count_r.shape[0])
    return {"precision": int((count_g > 0).sum()) / M, "recall": int((count_r > 0).sum()) / N,
            "density": int(count_g.sum(dtype=torch.int64)) / (k * M), "coverage": int((min_r <= rad2_r).sum()) / N}


def prdc(real: torch.Tensor, fake: torch.Tensor, k: int) -> Dict[str, float]:
    """``dict(precision, recall, density, coverage)`` of ``fake`` [M, d] against ``real`` [N, d] with k-th-neighbour radii (the
    definitions above).  Precision and recall depend on N and M: compare runs at the same sizes only."""
    real, fake = _check_pair(real, fake, "prdc")
    k = _check_k(k, min(int(real.shape[0]), int(fake.shape[0])), "prdc")
    rad2_r, rad2_g = knn_radii(real, k), knn_radii(fake, k)
    count_g, _ = ball_counts(fake, real, rad2_r)
    count_r, min_r = ball_counts(real, fake, rad2_g)
    return _prdc_from(count_g, count_r, min_r, rad2_r, k)


def _kid_from(s_gg: float, s_rr: float, s_gr: float, M: int, N: int) -> float:
    return s_gg / (M * (M - 1)) + s_rr / (N * (N - 1)) - 2.0 * s_gr / (M * N)


def kid(real: torch.Tensor, fake: torch.Tensor) -> float:
    """The unbiased MMD^2 estimate with the cubic kernel (a.b / d + 1)^3 over the FULL sets - one estimate, not the subset-bootstrap
    mean of Binkowski et al.'s code; both sets need at least 2 rows."""
    real, fake = _check_pair(real, fake, "kid")
    M, N = int(fake.shape[0]), int(real.shape[0])
    if M < 2 or N < 2:
        raise ValueError(f"kid: both sets need at least 2 rows, got {N} real and {M} fake")
    return _kid_from(float(poly_kernel_sum(fake, fake, True)), float(poly_kernel_sum(real, real, True)), float(poly_kernel_sum(fake, real)), M, N)


# ------------------------------------------------------------------------------------------------------------------ feature nets
def _vit_dims_tuple(dims) -> tuple:
    return tuple(int(getattr(dims, k)) for k in ("C", "IH", "P", "E", "H", "L", "R", "Kc"))


class FrozenViTFeatures:
    """A frozen copy of a ``VisionTransformer``'s flat parameters, evaluated with ``vg_vit_features`` (dropout 0): images
    [n, C, IH, IH] fp32 or bf16 on the device -> fp32 [n, E], the tensor the classifier's fc1 reads (``vit.norm(x)[:, 0, :]``)."""

    def __init__(self, vit, tag: Optional[str] = None):
        from .modules import VisionTransformer
        if hasattr(vit, "vit") and isinstance(vit.vit, VisionTransformer):  # ViTDiscriminator
            vit = vit.vit
        if not isinstance(vit, VisionTransformer):
            raise TypeError(f"expected a ViTDiscriminator or VisionTransformer, got {type(vit).__name__}")
        if vit.precision != "bf16":
            raise ValueError("vg_vit_features is built on the bf16 engine; set precision = 'bf16' on the feature network")
        if not vit._flat.aliased():
            vit._flat.named = dict(vit.named_parameters())
            vit._flat.rebuild()
        self.dims = _lib.VgVitDims(*_vit_dims_tuple(vit._dims))
        self.attn_fp8 = int(vit.attention_fp8)
        self.flat = vit._flat.flat.detach().clone()  # the copy: later training of the source does not move the features
        self.d = _check_d(self.dims.E)
        self.shadow: Optional[torch.Tensor] = None
        digest = hashlib.sha1(self.flat.cpu().numpy().tobytes()).hexdigest()[:16]
        self.tag = tag or ("vit:" + "x".join(str(v) for v in _vit_dims_tuple(self.dims)) + f":fp8={self.attn_fp8}:sha1={digest}")

    def to(self, device) -> "FrozenViTFeatures":
        device = torch.device(device)
        if self.flat.device != device or self.shadow is None:
            self.flat = self.flat.to(device)
            self.shadow = None
        return self

    def __call__(self, images: torch.Tensor, dense_top: bool = False) -> torch.Tensor:
        if not images.is_cuda:
            raise RuntimeError("the ViT feature network runs on the HIP engine: it needs cuda tensors; there is no CPU fallback")
        self.to(images.device)
        d = self.dims
        if images.dim() != 4 or tuple(images.shape[1:]) != (d.C, d.IH, d.IH):
            raise ValueError(f"the feature network reads [n, {d.C}, {d.IH}, {d.IH}] images, got {tuple(images.shape)}")
        if images.dtype not in (torch.float32, torch.bfloat16):
            images = images.float()
        x = images.detach().contiguous()
        B = int(x.shape[0])
        with torch.cuda.device(x.device):
            if self.shadow is None:  # the bf16 operands of the GEMMs, cast once: the parameters never change
                self.shadow = torch.empty(self.flat.numel(), dtype=torch.bfloat16, device=x.device)
                _lib.call("vg_cast_f32_bf16", self.flat.data_ptr(), self.shadow.data_ptr(), self.flat.numel(), _lib.stream())
            nbytes = _lib.lib().vg_vit_ws_bytes(C.byref(d), B)
            if nbytes <= 0:
                raise RuntimeError("vg_vit_ws_bytes failed")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            logits = torch.empty(B, d.Kc, dtype=torch.float32, device=x.device)
            feats = torch.empty(B, d.E, dtype=torch.float32, device=x.device)
            net = _lib.VgVitNet(d, self.flat.data_ptr(), self.shadow.data_ptr(), None, 0.0, 0, None, None, self.attn_fp8, int(dense_top))
            _lib.call("vg_vit_features", C.byref(net), B, x.data_ptr(), int(x.dtype == torch.bfloat16), ws.data_ptr(), logits.data_ptr(), feats.data_ptr(),
                      _lib.stream())
        return feats


def _config_vit_dims(config_or_dims) -> Dict[str, int]:
    if isinstance(config_or_dims, Config):
        c = config_or_dims
        return dict(n_channels=c.input_channels, embed_dim=c.embeddings_dimension, n_layers=c.transformer_blocks_count,
                    n_attention_heads=c.attention_heads_count, forward_mul=c.mlp_ratio, image_size=c.image_size, patch_size=c.patch_size)
    keys = ("n_channels", "embed_dim", "n_layers", "n_attention_heads", "forward_mul", "image_size", "patch_size")
    if not isinstance(config_or_dims, dict) or set(config_or_dims) != set(keys):
        raise TypeError(f"random_vit takes a Config or a dict with the keys {keys}, got {config_or_dims!r}")
    return {k: int(config_or_dims[k]) for k in keys}


def _table(mean, std) -> torch.Tensor:
    """the decode table of data.DeviceDataset: bf16(((v / 255) - mean) / std) as torch's fp32 computes it, [C, 256], as fp32"""
    v = torch.arange(256, dtype=torch.float32) / 255
    m_, s_ = (torch.tensor(t, dtype=torch.float32).reshape(-1, 1) for t in (mean, std))
    return ((v.reshape(1, 256) - m_) / s_).to(torch.bfloat16).float()


def quantize_images(x: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """What the reference does to a batch before Inception (src/v2/utils.py:165-166), then the dataset's decode: clamp to [-1, 1],
    ``((x * 0.5 + 0.5) * 255).to(uint8)`` (its truncation), and back through ``lut`` [C or 1, 256] - so generated images take exactly
    the values the real set's images can take."""
    q = ((x.float().clamp(-1.0, 1.0) * 0.5 + 0.5) * 255).to(torch.uint8).long()
    lut = lut.to(x.device)
    c = torch.arange(x.shape[1], device=x.device).reshape(1, -1, 1, 1).expand_as(q) % lut.shape[0]
    return lut[c, q].contiguous()


class FrechetDistance:
    """``FrechetDistance(features)(gan, epoch) -> float``: the Frechet distance between the feature moments of a real set
    (``fit_real``) and of ``n_fake`` images of ``gan.generator``.

    ``features``: a ``ViTDiscriminator`` / ``VisionTransformer`` - its flat parameters are COPIED AND FROZEN here, so a live
    discriminator given to it stops moving at construction time - or the result of ``FrechetDistance.random_vit`` (the default the
    trainer builds), or any callable ``images -> [n, d]`` tensor with d % 16 == 0 (``tag`` then names it in the statistics file).
    NEVER score a run by the discriminator it is training: features that move with training make the curve meaningless.

    ``n_fake`` latents come from a generator seeded by ``seed``: the same z at every call, so the epoch-to-epoch curve carries no
    sampling noise; a class-conditional generator gets the labels i % K.  The generator runs in eval mode under ``no_grad`` in batches
    of ``batch`` (a smaller last one), each batch goes through the feature network into a ``FeatureMoments``.  ``quantize``: the
    reference's uint8 treatment of the images (``quantize_images``) through the real set's own decode table.  ``ema``: score the
    averaged generator where the trainer keeps one (False: the raw one).  After a call ``last`` holds
    ``dict(distance, mean_term, trace_term, n_real, n_fake)``.

    ``manifold_k`` (1..8) and ``kid`` switch on what a single distance cannot say - whether a run lost fidelity or coverage:
    precision / recall / density / coverage with k-th-neighbour radii, and the full-set KID (the definitions above ``knn_radii``).
    With either on, ``fit_real`` also keeps up to ``bank_real`` real feature rows on the device - of a ``DeviceDataset`` the images
    at the evenly spaced indices floor(j N / n_keep), of an iterable the first n_keep seen; they are rows of the pass it makes anyway -
    with their radii and their kernel self-sum, computed once; a call keeps the fake features of its ONE generator pass (no launch of
    the generator or the feature net is added) and ``last`` gains ``precision, recall, density, coverage, kid`` (NaN for the half that is
    off), ``manifold_k`` and ``n_real_bank``.  The return value stays the Frechet distance.  Like it, these numbers rank the epochs
    of one run on a random ViT; they are not comparable with published values, and precision / recall depend on N and M.  Every rank
    of a multi-rank run evaluates alike; nothing here is sharded."""

    def __init__(self, features, n_fake: int = 10000, batch: int = 256, seed: int = 0, quantize: bool = True, ema: bool = True,
                 tag: Optional[str] = None, manifold_k: int = 0, kid: bool = False, bank_real: int = 10000):
        if isinstance(manifold_k, bool) or not isinstance(manifold_k, int) or not 0 <= manifold_k <= K_MAX:
            raise ValueError(f"manifold_k must be an integer in [0, {K_MAX}] (0: off), got {manifold_k!r}")
        if not isinstance(kid, bool):
            raise ValueError(f"kid must be a bool, got {kid!r}")
        if isinstance(bank_real, bool) or not isinstance(bank_real, int) or bank_real < 2:
            raise ValueError(f"bank_real must be an integer >= 2, got {bank_real!r}")
        if manifold_k and isinstance(n_fake, int) and manifold_k >= n_fake:
            raise ValueError(f"manifold_k = {manifold_k} needs more than k generated images, n_fake is {n_fake!r}")
        self.manifold_k, self.kid, self.bank_real = manifold_k, kid, bank_real
        self.bank: Optional[Dict[str, Any]] = None  # feats fp32 [n_keep, d]; rad2 fp64 [n_keep] with its k; self_sum
        self.fake_feats: Optional[torch.Tensor] = None  # the last call's features, kept only with an option on
        if isinstance(n_fake, bool) or int(n_fake) != n_fake or n_fake < 2:
            raise ValueError(f"n_fake must be an integer >= 2, got {n_fake!r}")
        if isinstance(batch, bool) or int(batch) != batch or batch < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        if isinstance(features, FrozenViTFeatures):
            self.features: Callable = features
            self.tag = tag or features.tag
        elif isinstance(features, nn.Module) and (hasattr(features, "vit") or hasattr(features, "_flat")):
            self.features = FrozenViTFeatures(features, tag)
            self.tag = self.features.tag
        elif callable(features):
            self.features = features
            self.tag = tag or f"callable:{getattr(features, '__qualname__', type(features).__name__)}"
        else:
            raise TypeError(f"features must be a ViTDiscriminator, a VisionTransformer or a callable, got {type(features).__name__}")
        self.n_fake, self.batch, self.seed, self.quantize, self.ema = int(n_fake), int(batch), int(seed), bool(quantize), bool(ema)
        self.lut = _table([0.5], [0.5])  # Normalize(0.5, 0.5), every channel; fit_real takes a DeviceDataset's own table
        self.real: Optional[Dict[str, Any]] = None  # mean, cov (fp64 numpy), n, d
        self.fake: Optional[FeatureMoments] = None  # the accumulator of the last call
        self.last: Optional[Dict[str, float]] = None

    @classmethod
    def random_vit(cls, config_or_dims, seed: int = 0, latent_seed: int = 0, **kw) -> "FrechetDistance":
        """The evaluator on a fixed-seed randomly initialised ViT of the given geometry (a ``Config`` or a dict of the
        ``VisionTransformer`` arguments n_channels, embed_dim, n_layers, n_attention_heads, forward_mul, image_size, patch_size), built
        under a forked CPU generator: the global RNG stream is left as it was.  ``seed`` (the network's) and the dims go into the tag,
        and with it into the statistics file; ``latent_seed`` is the evaluator's own ``seed``, the other arguments are its own too."""
        from .modules import VisionTransformer
        dims = _config_vit_dims(config_or_dims)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            vit = VisionTransformer(n_classes=1, dropout=0.0, **dims)
        tag = f"random-vit:seed={int(seed)}:" + ",".join(f"{k}={v}" for k, v in dims.items())
        return cls(FrozenViTFeatures(vit, tag), seed=latent_seed, **kw)

    # -- the real side -----------------------------------------------------------------------------------
    def _feats(self, images: torch.Tensor) -> torch.Tensor:
        f = self.features(images)
        if not torch.is_tensor(f) or f.dim() != 2 or f.shape[0] != images.shape[0]:
            raise ValueError(f"the feature function must return an [n, d] tensor for n images, got {getattr(f, 'shape', type(f))}")
        _check_d(f.shape[1])
        return f

    def _accumulate(self, acc: Optional[FeatureMoments], images: torch.Tensor, keep: Optional[list] = None, rows=None) -> FeatureMoments:
        """one feature pass over ``images`` into ``acc``; with ``keep``, its rows ``rows`` (all of them: None) are kept as fp32"""
        f = self._feats(images)
        if acc is None:
            acc = FeatureMoments(f.shape[1], f.device)
        if keep is not None and (rows is None or len(rows)):
            keep.append((f if rows is None else f[torch.as_tensor(rows, device=f.device)]).detach().float())
        return acc.update(f)

    @property
    def _wants_bank(self) -> bool:
        return bool(self.manifold_k) or self.kid

    def _bank_ready(self, device) -> Dict[str, Any]:
        """the real bank on ``device`` with what the options need: radii at this evaluator's k, the kernel self-sum - computed once"""
        b = self.bank
        if b is None:
            raise RuntimeError(f"FrechetDistance: {'manifold_k' if self.manifold_k else 'kid'} needs the real feature bank and there "
                               "is none; call fit_real, or load_real a file written with the option on")
        if b["feats"].device != device:
            b["feats"] = b["feats"].to(device)
            b["rad2"] = None if b["rad2"] is None else b["rad2"].to(device)
        if self.manifold_k and (b["rad2"] is None or b["k"] != self.manifold_k):
            b["rad2"], b["k"] = knn_radii(b["feats"], self.manifold_k), self.manifold_k  # ValueError: k >= the rows kept
        if self.kid and b["self_sum"] is None:
            b["self_sum"] = float(poly_kernel_sum(b["feats"], b["feats"], True))
        return b

    def fit_real(self, source: Union[DeviceDataset, Iterable]) -> "FrechetDistance":
        """The real set's moments, cached.  A ``DeviceDataset`` is visited in storage order, unflipped, ALL N images - the tail that
        ``steps_per_epoch`` drops from training included - through its decode table, which also becomes the table of ``quantize``.
        Anything else is an iterable of image batches (or ``(images, labels)`` pairs): uint8 batches go through the table, float
        batches through ``quantize_images`` when ``quantize`` is on."""
        acc: Optional[FeatureMoments] = None
        keep: Optional[list] = [] if self._wants_bank else None
        kept = 0
        with torch.no_grad():
            if isinstance(source, DeviceDataset):
                self.lut = source.lut.detach().float().cpu()
                n_keep = min(self.bank_real, source.N)
                picks = [(j * source.N) // n_keep for j in range(n_keep)] if keep is not None else []
                for lo in range(0, source.N, self.batch):
                    hi = min(lo + self.batch, source.N)
                    rows = [p - lo for p in picks[kept:kept + self.batch] if p < hi] if keep is not None else None
                    kept += len(rows or ())
                    acc = self._accumulate(acc, source.decode(torch.arange(lo, hi)), keep, rows)
            else:
                for item in source:
                    x = item[0] if isinstance(item, (tuple, list)) else item
                    x = torch.as_tensor(x)
                    if x.dtype == torch.uint8:
                        lut = self.lut.to(x.device)
                        c = torch.arange(x.shape[1], device=x.device).reshape(1, -1, 1, 1).expand_as(x) % lut.shape[0]
                        x = lut[c, x.long()].contiguous()
                    elif self.quantize:
                        x = quantize_images(x, self.lut)
                    for lo in range(0, x.shape[0], self.batch):
                        part = x[lo:lo + self.batch]
                        take = min(part.shape[0], self.bank_real - kept) if keep is not None else 0
                        kept += take
                        acc = self._accumulate(acc, part, keep if take else None, None if take == part.shape[0] else list(range(take)))
        if acc is None or acc.n < 2:
            raise ValueError("fit_real: the source held fewer than 2 images")
        mean, cov = acc.moments()
        self.real = {"mean": mean, "cov": cov, "n": acc.n, "d": acc.d}
        if keep is not None:
            self.bank = {"feats": torch.cat(keep).contiguous(), "rad2": None, "k": 0, "self_sum": None}
            self._bank_ready(self.bank["feats"].device)
        return self

    def save_real(self, path: str) -> None:
        """mean, cov, n, d, the feature net's tag and the decode table as an ``.npz``; with a real feature bank also ``bank_feats``,
        ``bank_k``, ``bank_rad2`` and ``bank_self_sum`` (NaN: not computed)."""
        if self.real is None:
            raise RuntimeError("save_real: no real statistics; call fit_real first")
        extra = {}
        if self.bank is not None:
            b = self.bank
            extra = {"bank_feats": b["feats"].cpu().numpy(), "bank_k": np.int64(b["k"] if b["rad2"] is not None else 0),
                     "bank_rad2": b["rad2"].cpu().numpy() if b["rad2"] is not None else np.zeros(0),
                     "bank_self_sum": np.float64(float("nan") if b["self_sum"] is None else b["self_sum"])}
        with open(path, "wb") as handle:  # a handle: numpy appends no suffix
            np.savez(handle, mean=self.real["mean"], cov=self.real["cov"], n=np.int64(self.real["n"]), d=np.int64(self.real["d"]),
                     tag=np.array(self.tag), lut=self.lut.numpy(), **extra)

    def load_real(self, path: str) -> "FrechetDistance":
        """Statistics written by ``save_real``; a file made under another feature network (tag) raises, and so does a file without the
        real feature bank when ``manifold_k`` or ``kid`` is on (the message names the option)."""
        with np.load(path, allow_pickle=False) as z:
            tag = str(z["tag"])
            if tag != self.tag:
                raise ValueError(f"load_real: {path} holds the statistics of feature net {tag!r}, this evaluator's is {self.tag!r}")
            self.real = {"mean": z["mean"].astype(np.float64), "cov": z["cov"].astype(np.float64), "n": int(z["n"]), "d": int(z["d"])}
            self.lut = torch.from_numpy(z["lut"].astype(np.float32))
            self.bank = None
            if "bank_feats" in z.files:
                k, ss = int(z["bank_k"]), float(z["bank_self_sum"])
                self.bank = {"feats": torch.from_numpy(z["bank_feats"].astype(np.float32)), "k": k,
                             "rad2": torch.from_numpy(z["bank_rad2"].astype(np.float64)) if k else None, "self_sum": None if ss != ss else ss}
            elif self._wants_bank:
                raise ValueError(f"load_real: {path} holds no real feature bank, which {'manifold_k' if self.manifold_k else 'kid'} needs; "
                                 "write it with fit_real and save_real on an evaluator with the option on")
        return self

    # -- the generated side ------------------------------------------------------------------------------
    def latents(self, generator: nn.Module, device: torch.device):
        """The evaluation's inputs, batch by batch: (z [b, latent], labels int32 [b] or None).  A function of ``seed``, ``n_fake``,
        ``batch`` and the device alone."""
        latent = int(getattr(generator, "latent"))
        K = int(getattr(generator, "n_classes", 0) or 0)
        g = torch.Generator(device=device).manual_seed(self.seed)
        for lo in range(0, self.n_fake, self.batch):
            b = min(self.batch, self.n_fake - lo)
            z = torch.randn(b, latent, device=device, generator=g)
            yield z, ((torch.arange(lo, lo + b, device=device) % K).to(torch.int32) if K else None)

    def __call__(self, gan, epoch: int = 0) -> float:
        if self.real is None:
            raise RuntimeError("FrechetDistance: no real statistics; call fit_real (or load_real) first")
        G = gan.generator if hasattr(gan, "generator") else gan
        p = next(iter(G.parameters()), None)
        device = p.device if p is not None else torch.device("cpu")
        was = G.training
        G.eval()
        if self._wants_bank and self.bank is None:
            self._bank_ready(device)  # raises, naming the option
        acc: Optional[FeatureMoments] = None
        keep: Optional[list] = [] if self._wants_bank else None
        try:
            with torch.no_grad():
                for z, labels in self.latents(G, device):
                    x = G(z) if labels is None else G(z, labels)
                    x = quantize_images(x, self.lut) if self.quantize else x.float()
                    acc = self._accumulate(acc, x, keep)
        finally:
            G.train(was)
        if acc.d != self.real["d"]:
            raise ValueError(f"the real statistics are of width {self.real['d']}, the features of width {acc.d}")
        self.fake = acc
        mean, cov = acc.moments()
        a, b = frechet_terms(self.real["mean"], self.real["cov"], mean, cov)
        self.last = {"distance": max(a + b, 0.0), "mean_term": a, "trace_term": b, "n_real": self.real["n"], "n_fake": acc.n}
        if keep is not None:
            self.last.update(self._pair_metrics(torch.cat(keep).contiguous()))
        return self.last["distance"]

    def _pair_metrics(self, fake: torch.Tensor) -> Dict[str, Any]:
        """the manifold metrics and KID of the kept fake features against the real bank: the fakes' radii, two ball-count launches
        (fakes in the reals' balls; reals in the fakes' balls, with each real's nearest fake), two kernel sums"""
        bank = self._bank_ready(fake.device)
        real = bank["feats"]
        self.fake_feats = fake
        nan = float("nan")
        out: Dict[str, Any] = {"precision": nan, "recall": nan, "density": nan, "coverage": nan, "kid": nan,
                               "manifold_k": self.manifold_k, "n_real_bank": int(real.shape[0])}
        if self.manifold_k:
            count_g, _ = ball_counts(fake, real, bank["rad2"])
            count_r, min_r = ball_counts(real, fake, knn_radii(fake, self.manifold_k))
            out.update(_prdc_from(count_g, count_r, min_r, bank["rad2"], self.manifold_k))
        if self.kid:
            M, N = int(fake.shape[0]), int(real.shape[0])
            out["kid"] = _kid_from(float(poly_kernel_sum(fake, fake, True)), bank["self_sum"], float(poly_kernel_sum(fake, real)), M, N)
        return out


__all__ = ["FeatureMoments", "FrechetDistance", "FrozenViTFeatures", "frechet_distance", "frechet_terms", "quantize_images",
           "knn_radii", "ball_counts", "poly_kernel_sum", "prdc", "kid"]
