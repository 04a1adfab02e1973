"""``train_model(config=None)``: the entry point of the reference's ``main-v2.py`` (src/v2/training.py:34) on the
HIP engine, with the reference's trainer shell around the hot path.

Kept from the reference:
  * ``Config`` handling (``Config() if not config else Config(**config)``, training.py:130);
  * two AdamW optimizers (lr from the config, weight_decay 1e-3, :150-157) and the alternating step (:176-211) - both
    inside ``GanEngine``;
  * the output tree of src/v2/utils.py:13-20,176-182: ``$SCRATCH/output/<start time>/{images,input,noise,checkpoints}``;
  * ``log`` (utils.py:185-189): ``[YYYY-mm-dd HH:MM:SS.mmm] message`` on the console and appended to ``training.log``;
  * per epoch (:163-166,171-172): a fixed-noise sample grid ``images/samples_epoch_<e>.png``, the noise itself
    ``noise/noise_epoch_<e>.png`` and the first input batch ``input/input_epoch_<e>.png``, written as PNG grids with
    ``nrow = floor(sqrt(batch_size))`` and min-max normalisation (what ``vutils.save_image(..., normalize=True)`` does);
  * the epoch line ``Epoch [e/E] | Disc Loss: ..., Gen Loss: ... | FID: ...`` (:227-230), ``best_model_epoch_<e>_fid_<n>.pth``
    checkpoints when the FID improves (:216-226) and, in ``finally``, ``final_model.ckpt`` + a last sample grid +
    the run-time line (:252-268);
  * exceptions raised inside the loop are logged, not re-raised (:248-251) - EXCEPT errors of the HIP engine itself
    (``_lib.HipError``: a failed launch or rejected kernel arguments), which are logged and then re-raised without
    writing a checkpoint: a broken kernel must not look like a finished run.

Substitutions (documented in DESIGN.md):
  * data: CIFAR-10 needs a download (utils.py:109-114); pass ``data_loader`` (any iterable of ``(images, labels)``
    batches, e.g. the reference's own DataLoader) or get synthetic uniform [-1,1] batches, the range of its
    ``Normalize(0.5, 0.5)``;
  * FID needs Inception weights that cannot be fetched offline (utils.py:155-175): pass ``fid_fn(gan, epoch) -> float``
    to enable it, or ``fid="random-vit"`` for the Frechet distance on a frozen random ViT (metrics.py; it ranks a run's epochs, it is
    not the published FID); without either the score is NaN and no "best" checkpoint is written;
  * the generator is the v1 SLN/SIREN network (the v2 ``ViTGenerator`` tail raises) and the loss is
    BCE-with-logits on a 1-logit discriminator (the v2 ``criterion`` call raises).
"""
from __future__ import annotations

import datetime
import math
import os
import struct
import traceback
import zlib
from typing import Any, Callable, Dict, Iterable, Optional, Tuple, Union

import torch
from torch import nn

from . import _lib
from .config import Config
from .data import DeviceDataset
from .engine import GanEngine
from .modules import ViTGAN, generator_from_config

START_TIME = datetime.datetime.now()
FID_KINDS = ("", "random-vit")  # train_model(fid=...)
FID_SEED = 0                    # of the random feature net and of the evaluation's latents


class RunDirs:
    """The reference's module-level path constants (src/v2/utils.py:13-20), bound to one run."""

    def __init__(self, base: Optional[str] = None, start: Optional[datetime.datetime] = None):
        self.base = base if base is not None else os.getenv("SCRATCH", ".")
        self.start = start or START_TIME
        self.output = os.path.join(self.base, "output")
        self.save = os.path.join(self.output, self.start.strftime("%Y%m%d-%H%M%S"))
        self.images = os.path.join(self.save, "images")
        self.input = os.path.join(self.save, "input")
        self.noise = os.path.join(self.save, "noise")
        self.checkpoints = os.path.join(self.save, "checkpoints")

    def construct(self) -> None:  # utils.py:176-182
        for d in (self.output, self.save, self.images, self.input, self.noise, self.checkpoints):
            os.makedirs(d, exist_ok=True)


_log_file: Optional[str] = None


def log(message: str) -> None:
    """utils.py:185-189 without the rich markup pass."""
    stamp = datetime.datetime.now().strftime("[%F %T.%f")[:-3] + "]"
    line = f"{stamp} {message}"
    print(line, flush=True)
    if _log_file is not None:
        with open(_log_file, "a", encoding="utf-8") as handle:
            handle.write(line + "\n")


# ---- PNG grids (torchvision is not a dependency) ---------------------------------------------------------------
def make_grid(images: torch.Tensor, nrow: int, padding: int = 2, normalize: bool = True) -> torch.Tensor:
    """[B,C,H,W] -> [C, rows*(H+p)+p, cols*(W+p)+p] like ``torchvision.utils.make_grid``: ``nrow`` images per row,
    ``padding`` zero pixels around each, and with ``normalize`` the WHOLE batch shifted/scaled by its min / max."""
    x = images.detach().float().cpu()
    if x.dim() != 4:
        raise ValueError("expected a [B,C,H,W] batch")
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    if normalize:
        lo, hi = float(x.min()), float(x.max())
        x = ((x - lo) / max(hi - lo, 1e-5)).clamp(0, 1)
    B, C, H, W = x.shape
    cols = min(max(nrow, 1), B)
    rows = int(math.ceil(B / cols))
    grid = torch.zeros(C, rows * (H + padding) + padding, cols * (W + padding) + padding)
    for i in range(B):
        r, c = divmod(i, cols)
        y0, x0 = r * (H + padding) + padding, c * (W + padding) + padding
        grid[:, y0:y0 + H, x0:x0 + W] = x[i]
    return grid


def write_png(path: str, chw: torch.Tensor) -> None:
    """8-bit RGB PNG of a [3,H,W] tensor in [0,1] (round-half-up like ``mul(255).add_(0.5).clamp_(0,255)``)."""
    img = chw.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()
    H, W, C = img.shape
    if C != 3:
        raise ValueError("RGB only")
    raw = bytearray()
    data = img.numpy().tobytes()
    for y in range(H):
        raw.append(0)  # filter type 0 per scanline
        raw += data[y * W * 3:(y + 1) * W * 3]

    def chunk(tag: bytes, payload: bytes) -> bytes:
        return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(bytes(raw), 6)) + chunk(b"IEND", b""))


def save_images(save_path: str, images: torch.Tensor, batch_size: int) -> None:
    """training.py:47-50."""
    write_png(save_path, make_grid(images, nrow=max(1, math.floor(math.sqrt(batch_size))), normalize=True))


def save_figures(save_dir: str, **series) -> None:
    """utils.py:46-98: loss / FID curves, written only when matplotlib is importable and the series are non-empty."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except Exception:  # plotting is optional
        return
    if series.get("gen_losses") and series.get("disc_losses"):
        plt.figure(figsize=(10, 5))
        plt.title("Generator and Discriminator Loss During Training")
        plt.plot(series["gen_losses"], label="G Loss")
        plt.plot(series["disc_losses"], label="D Loss")
        plt.xlabel("Iterations"); plt.ylabel("Loss"); plt.legend()
        plt.savefig(os.path.join(save_dir, "losses.png")); plt.close()
    fids = [f for f in series.get("fid_scores", []) if f == f]
    if fids:
        plt.figure(figsize=(10, 5))
        plt.title("FID Score During Training")
        plt.plot(fids, label="FID Score")
        plt.xlabel("Iterations"); plt.ylabel("FID"); plt.legend()
        plt.savefig(os.path.join(save_dir, "fid_score.png")); plt.close()
    # the two figures of the per-step record (utils.py:71-97): only when their series are present
    if len(series.get("gradient_norms_gen", ())) and len(series.get("gradient_norms_disc", ())):
        plt.figure(figsize=(10, 5))
        plt.title("Gradient Norms During Training")
        plt.plot(series["gradient_norms_gen"], label="Gen Grad Norm")
        plt.plot(series["gradient_norms_disc"], label="Disc Grad Norm")
        plt.xlabel("Iterations"); plt.ylabel("Gradient Norm"); plt.legend()
        plt.savefig(os.path.join(save_dir, "gradient_norms.png")); plt.close()
    if len(series.get("disc_real_accuracies", ())) and len(series.get("disc_fake_accuracies", ())):
        plt.figure(figsize=(10, 5))
        plt.title("Discriminator Accuracy During Training")
        plt.plot(series["disc_real_accuracies"], label="Disc Real Acc")
        plt.plot(series["disc_fake_accuracies"], label="Disc Fake Acc")
        plt.xlabel("Iterations"); plt.ylabel("Accuracy"); plt.legend()
        plt.savefig(os.path.join(save_dir, "accuracies.png")); plt.close()


def get_data_loader(c: Config):
    """utils.py:100-121 (CIFAR-10, Resize/ToTensor/Normalize(0.5), shuffle, 4 workers, drop_last).  Needs torchvision
    and a reachable / pre-downloaded dataset, neither of which this build depends on."""
    try:
        import torchvision.datasets as datasets
        import torchvision.transforms as transforms
    except ImportError as e:
        raise ImportError("get_data_loader needs torchvision; pass train_model(data_loader=...) or use the synthetic default") from e
    from torch.utils.data import DataLoader
    tf = transforms.Compose([transforms.Resize(c.image_size), transforms.ToTensor(),
                             transforms.Normalize([0.5] * c.input_channels, [0.5] * c.input_channels)])
    ds = datasets.CIFAR10(root=os.path.expanduser("~/rep/me/vit-gan/data/cifar-10-python/"), train=True, download=True, transform=tf)
    return DataLoader(ds, batch_size=c.batch_size, shuffle=True, num_workers=4, drop_last=True)


class Plateau:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor, patience)`` with its defaults (relative threshold 1e-4, no
    cooldown) as a host-side rule: ``step(metric)`` says whether the rates are to be reduced now."""

    def __init__(self, factor: float, patience: int, threshold: float = 1e-4):
        self.factor, self.patience, self.threshold = factor, patience, threshold
        self.best, self.bad = float("inf"), 0

    def step(self, metric: float) -> bool:
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1  # (a NaN score is a bad epoch, as in torch)
        if self.bad > self.patience:
            self.bad = 0
            return True
        return False


def parse_lr_plateau(lr_plateau, fid_fn) -> Optional[Plateau]:
    """``(factor, patience)`` of ``train_model(lr_plateau=...)`` as a ``Plateau`` (None = off); host only."""
    if lr_plateau is None:
        return None
    try:
        factor, patience = lr_plateau
        factor = float(factor)
    except (TypeError, ValueError):
        raise ValueError(f"lr_plateau must be a pair (factor, patience), got {lr_plateau!r}") from None
    if not 0.0 < factor < 1.0:
        raise ValueError(f"lr_plateau: the factor must be in (0, 1), got {lr_plateau[0]!r}")
    if isinstance(patience, bool) or not isinstance(patience, int) or patience < 0:
        raise ValueError(f"lr_plateau: the patience must be a non-negative integer (epochs), got {patience!r}")
    if fid_fn is None:
        raise ValueError("lr_plateau: the plateau rule watches the FID hook's score; pass fid_fn")
    return Plateau(factor, patience)


class MissingLabelsError(ValueError):
    """a conditional run was given a data loader without labels: the caller's error, raised out of ``train_model``"""


class SyntheticLoader:
    """``steps`` batches of uniform [-1,1] images (the range of Normalize(0.5, 0.5)) generated on the device.  ``labels=K > 0``: every
    batch comes with int64 labels uniform over [0, K) from the same generator (0, the default: ``None`` in their place)."""

    def __init__(self, c: Config, steps: int, device: torch.device, seed: int = 1234, labels: int = 0):
        self.c, self.steps, self.device, self.labels = c, steps, device, int(labels)
        self.gen = torch.Generator(device=device).manual_seed(seed)

    def __len__(self) -> int:
        return self.steps

    def __iter__(self):
        c = self.c
        for _ in range(self.steps):
            x = torch.rand(c.batch_size, c.input_channels, c.image_size, c.image_size, device=self.device, generator=self.gen)
            y = torch.randint(0, self.labels, (c.batch_size,), device=self.device, generator=self.gen) if self.labels else None
            yield x * 2 - 1, y


def trainable_config(c: Config, conditional: bool = False) -> Config:
    """The configuration ``train_model`` builds ``ViTGAN`` from: a 1-logit discriminator (the executable loss, SURVEY 8
    row a12) and a generator that can produce an image - the reference's default "v2" tail raises, so it is
    replaced by the SLN/SIREN network (row-token layout at 32x32, patch grid beyond).  ``conditional``: ``classes_count`` stays -
    the K-way head is the conditional discriminator."""
    kind = c.generator_kind
    if kind == "v2":
        kind = "sln_siren" if c.image_size <= 32 else "sln_siren_patch"
    return c.model_copy(update={"generator_kind": kind} if conditional else {"classes_count": 1, "generator_kind": kind})


def discriminator_state(gan_state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``ViTDiscriminator`` keys (``vit.*``) out of a ``ViTGAN`` checkpoint (``discriminator.vit.*``, ``generator.*``) as
    written by ``train_model`` / src/v2/training.py:220-226,263 - for ``D.load_state_dict(..., strict=True)``."""
    pre = "discriminator."
    return {k[len(pre):]: v for k, v in gan_state.items() if k.startswith(pre)}


def train_model(config: Optional[Dict[str, Any]] = None, steps_per_epoch: int = 50, max_epochs: Optional[int] = None,
                loss: str = "ns", device: str = "cuda:0", seed: int = 0, data_loader: Optional[Iterable] = None,
                fid_fn: Optional[Callable[[nn.Module, int], float]] = None, output_base: Optional[str] = None,
                save_artifacts: bool = True, clip_d: Optional[float] = None, clip_g: Optional[float] = None,
                diversity_weight: float = 0.0, instance_noise: float = 0.0, gp_weight: float = 0.0, diffaug: str = "",
                ema_decay: float = 0.0, ema_start: int = 0, spectral_norm: str = "", bcr=(0.0, 0.0), bcr_aug: str = "",
                aug_p: Optional[float] = None, ada_target: float = 0.0, ada_interval: int = 4, ada_kimg: float = 500.0,
                r1_gamma: float = 0.0, r1_interval: int = 1, conditional: bool = False,
                lr_schedule: str = "", lr_warmup: int = 0, lr_total: Optional[int] = None, lr_final: float = 0.0,
                lr_plateau: Optional[Tuple[float, int]] = None, dataset: Optional[DeviceDataset] = None,
                fid: str = "", fid_samples: int = 10000, manifold_k: int = 0, kid: bool = False,
                telemetry: Union[bool, int] = False):
    """``loss``: "ns" (default: the executable v1 loss), "hinge", or "wasserstein" - the critic losses of the reference's
    unreached step (training.py:67-125); ``clip_d`` / ``clip_g``: its clip_grad_norm_ limits (5.0 / 0.5 there);
    ``diversity_weight``: its diversity term (0.1 there); ``instance_noise``: sigma of the noise on D's inputs (0.1
    there); ``gp_weight``: the weight of its gradient penalty (``c.lambda_gp``, a field the reference's Config lacks);
    ``diffaug``: differentiable augmentation of the discriminator's inputs, a comma-separated subset of color, translation, cutout
    (``GanEngine(diffaug=...)``; the reference has none);
    ``ema_decay`` / ``ema_start``: an exponential moving average of the generator's weights, kept inside the step
    (``GanEngine(ema_decay=...)``; the reference has none).  When it is on, the sample grids and ``fid_fn`` see the AVERAGED
    generator - an eval-mode ``SirenGenerator`` refreshed from the engine before each use, returned as ``"generator_ema"`` -
    and ``generator_ema.pth`` (its state_dict) is written beside ``final_model.ckpt`` and beside each best-FID checkpoint.
    ``engine_state.pth`` (``GanEngine.state_dict()``: optimizer moments, step counter, the average) is written beside
    ``final_model.ckpt`` in every run; the ``gan.state_dict()`` files keep the reference's keys.
    ``spectral_norm``: "qkv" or "all" - spectral normalisation of the discriminator's weights inside the step
    (``GanEngine(spectral_norm=...)``).  When it is on, the best-FID and final checkpoints hold the discriminator's EFFECTIVE weights
    (``GanEngine.effective_state_dict()``), so they load into a plain ``ViTGAN`` - or the reference's - and compute the trained
    function; the raw weights a resumed run needs (with ``engine_state.pth``) go to ``discriminator_raw.pth`` beside
    ``final_model.ckpt``, and ``training.log`` says so.
    ``bcr`` / ``bcr_aug``: the weights (lambda_real, lambda_fake) of balanced consistency regularisation of the discriminator and, when
    ``diffaug`` is off, its transform (``GanEngine(bcr=..., bcr_aug=...)``; the reference has none).  When it is on, every epoch's line
    of ``training.log`` also carries the two consistency losses (the unweighted means over the real and the fake images).
    ``aug_p`` / ``ada_target`` / ``ada_interval`` / ``ada_kimg``: the application probability of ``diffaug``'s members and its adaptive
    controller (``GanEngine(aug_p=..., ada_target=...)``; the reference has none).  With ``ada_target > 0`` every epoch's line also
    carries the probability in force and the overfitting signal r_t of the last update.
    ``r1_gamma`` / ``r1_interval``: the zero-centred R1 penalty on real images and its lazy-regularisation interval
    (``GanEngine(r1_gamma=..., r1_interval=...)``; the reference has none).  When it is on, every epoch's line also carries the last
    computed unweighted penalty.
    ``conditional``: class-conditional training (``GanEngine(n_classes=...)``; the reference has none that runs) with
    ``classes_count`` classes (at most 16): the loader's labels go to the step - a loader that yields ``None`` in their place, like the
    default ``SyntheticLoader`` without ``labels=K``, is an error; when no loader is given the synthetic one draws labels itself -
    and image i of every sample grid is of class ``i % classes_count``.  The checkpoints then also hold
    ``generator.class_embedding.weight``.
    ``lr_schedule`` / ``lr_warmup`` / ``lr_total`` / ``lr_final``: a learning-rate schedule evaluated on the device
    (``GanEngine(lr_schedule=...)``: "constant", "linear" or "cosine" with ``lr_warmup`` steps of linear warm-up, falling to ``lr_final``
    times the base rate at step ``lr_total``); ``lr_total=None`` means the whole run, ``epochs * len(loader)`` steps.  When it is on, a
    header line of ``training.log`` states the schedule and every epoch's line carries the two rates in force.
    ``lr_plateau``: ``(factor, patience)``, the reference's intended ``ReduceLROnPlateau(mode="min")`` on the FID hook
    (src/v2/training.py:15,215-216; torch's default relative threshold 1e-4, no cooldown, no floor): when ``fid_fn``'s score has not
    improved for more than ``patience`` epochs, both rates' multipliers are multiplied by ``factor``
    (``GanEngine.set_lr_scale``).  It needs ``fid_fn`` (or ``fid=``), and it switches the device-resident rates on (``lr_schedule=""`` then means
    "constant").
    ``dataset``: a ``DeviceDataset`` (data.py) instead of ``data_loader`` (giving both is an error): the set lives on the device and
    every step fetches its own batch (``GanEngine(dataset=...)``).  An epoch is then ``dataset.steps_per_epoch(batch_size)`` steps, and
    ``input_epoch_<e>.png`` shows the batch the epoch's first step trains on, decoded on the host side from the same rule
    (``dataset.decode(dataset.indices(...), dataset.flips(...))``).  A conditional run takes the set's labels.
    ``fid`` / ``fid_samples``: ``fid="random-vit"`` (and no ``fid_fn``) builds the FID hook itself: ``metrics.FrechetDistance`` on a
    fixed-seed randomly initialised, frozen ViT of the model's own geometry, ``fid_samples`` generated images per evaluation from fixed
    latents, scored on the averaged generator when ``ema_decay`` is on.  The real statistics come from ``dataset`` (all N images) or
    else from one pass over the loader before the first step; they are written to ``real_stats.npz`` in the run's directory, and a
    header line of ``training.log`` names the feature net, its seed, n_real and n_fake.  With it the epoch line's ``FID:`` is a number,
    the best-FID checkpoints are written and ``lr_plateau`` needs no ``fid_fn``.  The score ranks the epochs of a run; it is NOT
    comparable with published FID numbers (those need Inception weights: pass them as a callable).  The hook NEVER
    defaults to the discriminator being trained - features that move with training would make the curve meaningless; a user who hands
    ``FrechetDistance`` the live ``D`` gets a copy frozen at that moment.  ``fid=""`` (default): everything as before, ``FID: nan``.

    ``manifold_k`` / ``kid`` (only with ``fid="random-vit"``): ``manifold_k`` in 1..8 adds precision, recall, density and coverage
    with k-th-neighbour radii, ``kid=True`` the full-set KID, both from the features of the same evaluation pass against up to 10000
    real feature rows kept by ``fit_real`` (metrics.py has the definitions).  One more header line names them, the epoch line ENDS in
    `` | P: .. R: .. D: .. C: ..`` and / or `` | KID: ..``, and each entry of the returned history gains a third element, the dict
    of these values.  They tell a loss of fidelity from a loss of coverage - mode collapse - which one distance cannot; like it they
    rank the epochs of one run only.  Every rank evaluates alike.  Off (default): nothing changes.

    ``telemetry``: the step records itself on the device (``GanEngine(telemetry=...)``): ``True`` keeps one epoch's steps, an integer
    that many.  At the epoch's synchronisation point the trainer reads ``eng.history()``, extends the reference's per-step series
    (``gradient_norms_gen`` / ``gradient_norms_disc``: the sums of the per-tensor norms; ``disc_real_accuracies`` /
    ``disc_fake_accuracies``, src/v2/training.py:80-84,112-123), hands them to ``save_figures`` (``gradient_norms.png``,
    ``accuracies.png``) and rewrites ``telemetry.npz`` in the run's directory: ``step``, every field of the record, the per-tensor norms
    ``grad_norms_d`` / ``grad_norms_g`` with ``keys_d`` / ``keys_g``, cumulative over the run.  The epoch line gains the reference's own
    commented fields (training.py:229) from the epoch's last step, `` | Disc Real Acc: .. | Disc Fake Acc: .. | Grad Norm Gen: .. | Grad
    Norm Disc: ..``; the first non-finite gradient is logged once (``Non-finite gradient at step N``) and a warning line says when
    records fell out of a ring shorter than the epoch.  The returned dict gains ``"telemetry"``, the cumulative record.  ``False``
    (default): the lines, files and series are exactly what they were."""
    global _log_file
    if fid not in FID_KINDS:
        raise ValueError(f"fid must be one of {FID_KINDS}, got {fid!r}")
    if fid and fid_fn is not None:
        raise ValueError("fid: the trainer builds the FID hook itself; pass either fid or fid_fn, not both")
    if fid and (isinstance(fid_samples, bool) or not isinstance(fid_samples, int) or fid_samples < 2):
        raise ValueError(f"fid_samples must be an integer >= 2, got {fid_samples!r}")
    if isinstance(manifold_k, bool) or not isinstance(manifold_k, int) or not 0 <= manifold_k <= 8:
        raise ValueError(f"manifold_k must be an integer in [0, 8] (0: off), got {manifold_k!r}")
    if not isinstance(kid, bool):
        raise ValueError(f"kid must be a bool, got {kid!r}")
    if (manifold_k or kid) and fid != "random-vit":
        raise ValueError('manifold_k / kid: these metrics are computed by the evaluator the trainer builds; pass fid="random-vit" with them')
    if manifold_k and manifold_k >= fid_samples:
        raise ValueError(f"manifold_k = {manifold_k} needs more than k generated images, fid_samples is {fid_samples}")
    if dataset is not None:  # the caller's errors whatever the machine: before the device check
        if data_loader is not None:
            raise ValueError("dataset: the step fetches its own batches from the dataset; pass either dataset or data_loader, not both")
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"dataset must be a DeviceDataset, got {type(dataset).__name__}")
    from .ops import parse_aug_policy, parse_bcr_weights
    parse_aug_policy(diffaug)  # a bad policy string is the caller's error whatever the machine: before the device check
    bcr_on = parse_bcr_weights(bcr) != (0.0, 0.0)
    if parse_aug_policy(bcr_aug) and diffaug:
        raise ValueError("bcr_aug: with diffaug on, diffaug's own transform is the consistency partner; leave bcr_aug empty")
    if bool(parse_aug_policy(bcr_aug)) != (bcr_on and not parse_aug_policy(diffaug)):
        raise ValueError("bcr: consistency weights need a transform (diffaug, or bcr_aug without it), and bcr_aug needs non-zero weights in bcr")
    from .spectral import parse_spectral_set
    parse_spectral_set(spectral_norm)
    # the probability's and the controller's argument errors are the caller's whatever the machine: before the device check
    from .ops import parse_ada_options
    parse_ada_options(aug_p, ada_target, ada_interval, ada_kimg, parse_aug_policy(diffaug), loss)
    from .ops import parse_r1_options
    parse_r1_options(r1_gamma, r1_interval, gp_weight)
    if telemetry is not False and telemetry is not True:
        from .ops import parse_telemetry
        if parse_telemetry(telemetry) < 1:
            raise ValueError(f"telemetry must be False, True (a ring of one epoch's steps) or a capacity >= 1, got {telemetry!r}")
    plateau = parse_lr_plateau(lr_plateau, fid_fn if fid_fn is not None else (fid or None))
    if not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
    if int(ema_start) != ema_start or ema_start < 0:
        raise ValueError(f"ema_start must be a non-negative integer, got {ema_start!r}")
    c = Config() if not config else Config(**config)
    conditional = bool(conditional)
    K = int(c.classes_count) if conditional else 0
    if conditional and not 1 <= K <= 16:
        raise ValueError(f"conditional: classes_count must be in [1, 16] (the width of the head kernels), got {c.classes_count!r}")
    if conditional and (float(gp_weight) != 0.0 or float(r1_gamma) > 0.0):
        raise ValueError("conditional: the gradient penalties (gp_weight, r1_gamma) are not built for the label-selected logit; switch them off")
    epochs = c.epochs if max_epochs is None else min(c.epochs, max_epochs)
    # the schedule's argument errors are the caller's whatever the machine: before the device check (None = the whole run)
    from .ops import parse_lr_schedule
    if plateau is not None and not lr_schedule and not lr_warmup:
        lr_schedule = "constant"  # the multipliers live with the device-resident rates
    if dataset is not None:
        if (dataset.C, dataset.IH) != (c.input_channels, c.image_size):
            raise ValueError(f"dataset: its images are {dataset.C} x {dataset.IH} x {dataset.IH}, the configuration says "
                             f"{c.input_channels} x {c.image_size} x {c.image_size}")
        if (dataset.labels is not None) != conditional:
            raise ValueError("dataset: a conditional run needs a dataset with labels, an unconditional one a dataset without them "
                             f"(conditional={conditional}, labels {'present' if dataset.labels is not None else 'absent'})")
        steps_per_epoch = dataset.steps_per_epoch(c.batch_size)  # ValueError: fewer images than one batch
    if lr_total is None:
        per_epoch = len(data_loader) if data_loader is not None else steps_per_epoch
        lr_total = epochs * per_epoch if (lr_schedule or lr_warmup) else 0
    lr_opts = parse_lr_schedule(lr_schedule, lr_warmup, lr_total, lr_final)
    tel_cap = 0 if telemetry is False else int(telemetry)
    if telemetry is True:  # one epoch's steps
        tel_cap = max(1, len(data_loader) if data_loader is not None and hasattr(data_loader, "__len__") else steps_per_epoch)
    if not torch.cuda.is_available():
        raise RuntimeError("train_model needs an MI355X: the HIP engine has no CPU path")
    dev = torch.device(device)
    torch.manual_seed(seed)
    dirs = RunDirs(output_base, datetime.datetime.now())
    if save_artifacts:
        dirs.construct()
        _log_file = os.path.join(dirs.save, "training.log")
    gan = ViTGAN(trainable_config(c, conditional), conditional).to(dev).train()  # modules.ViTGAN(c).to(device); gan.train(), training.py:145,148
    D, G = gan.discriminator, gan.generator
    eng = GanEngine(D, G, batch=c.batch_size, loss=loss, lr_d=c.discriminator_learning_rate, lr_g=c.generator_learning_rate,
                    weight_decay=1e-3, seed=seed, clip_d=clip_d, clip_g=clip_g, diversity_weight=diversity_weight,
                    instance_noise=instance_noise, gp_weight=gp_weight, diffaug=diffaug, ema_decay=ema_decay, ema_start=ema_start,
                    spectral_norm=spectral_norm, bcr=bcr, bcr_aug=bcr_aug, aug_p=aug_p, ada_target=ada_target, ada_interval=ada_interval,
                    ada_kimg=ada_kimg, r1_gamma=r1_gamma, r1_interval=r1_interval, n_classes=K,
                    lr_schedule=lr_schedule, lr_warmup=lr_warmup, lr_total=lr_total, lr_final=lr_final, dataset=dataset,
                    **({"telemetry": tel_cap} if tel_cap else {}))

    def gan_checkpoint():  # gan.state_dict(), the discriminator's normalised matrices as the network applies them
        sd = gan.state_dict()
        if eng.spec is not None:
            for k, v in eng.effective_state_dict().items():
                sd["discriminator." + k] = v
        return sd
    G_ema: Optional[nn.Module] = None
    gan_ema: Optional[nn.Module] = None
    if eng.ema_g is not None:  # the averaged generator as a module of its own: same constructor arguments, eval mode, never trained
        G_ema = generator_from_config(trainable_config(c, conditional), K).to(dev).eval()
        gan_ema = nn.Module()  # what fid_fn receives: .generator = the averaged network, .discriminator = D
        gan_ema.generator, gan_ema.discriminator = G_ema, D

    def refresh_ema():
        if G_ema is not None:
            G_ema.load_state_dict(eng.ema_state_dict(), strict=True)
    loader = data_loader if data_loader is not None else SyntheticLoader(c, steps_per_epoch, dev, labels=K)
    fid_eval = None
    if fid:  # the hook the trainer builds: a frozen random ViT of the model's geometry, never the discriminator in training
        from .metrics import FrechetDistance
        more = {"manifold_k": manifold_k, "kid": kid} if (manifold_k or kid) else {}  # off: the constructor call of before
        fid_eval = FrechetDistance.random_vit(trainable_config(c, conditional), seed=FID_SEED, n_fake=fid_samples, latent_seed=FID_SEED, **more)

    def dataset_epoch():  # the steps of one epoch: the engine fetches; the first one carries the batch it will train on, for the input grid
        for i in range(steps_per_epoch):
            first = None
            if i == 0 and save_artifacts:
                at = (eng.steps, c.batch_size, eng.sync.rank, eng.world, eng.data_seed)
                first = dataset.decode(dataset.indices(*at), dataset.flips(*at))
            yield first, None
    if dataset is not None:
        loader = None
    # the fixed sample grid of a conditional run: image i is of class i % K
    grid_labels = (torch.arange(c.batch_size, device=dev) % K).to(torch.int32) if conditional else None

    def construct_noise():  # the v1 generator's latent, gan.py:231-232 (the v2 noise is image-shaped, training.py:35-42)
        return torch.randn(c.batch_size, G.latent, device=dev)

    def save_samples(label: Union[str, int], noise: torch.Tensor):  # training.py:52-57
        if not save_artifacts:
            return
        if G_ema is not None:  # from the averaged weights
            refresh_ema()
            with torch.no_grad():
                samples = G_ema(noise, grid_labels).detach().float().cpu() * 0.5 + 0.5
        else:
            was = G.training
            G.eval()
            with torch.no_grad():
                samples = G(noise, grid_labels).detach().float().cpu() * 0.5 + 0.5
            G.train(was)
        save_images(os.path.join(dirs.images, f"samples_epoch_{label}.png"), samples, c.batch_size)

    def noise_as_image(noise: torch.Tensor) -> torch.Tensor:  # the latent is a vector here: show it as 1x32x32 tiles
        side = int(math.isqrt(noise.shape[1]))
        return noise[:, :side * side].reshape(noise.shape[0], 1, side, side)

    best_fid = float("inf")
    disc_losses, gen_losses, fid_scores, history = [], [], [], []
    tel: Dict[str, Any] = {}  # the cumulative per-step record (telemetry on): name -> numpy array, plus keys_d / keys_g
    nonfinite_logged = False

    def tel_series():  # the reference's per-step series for save_figures; nothing when off
        if not tel:
            return {}
        return {"gradient_norms_gen": tel["gnorm_g_sum"].tolist(), "gradient_norms_disc": tel["gnorm_d_sum"].tolist(),
                "disc_real_accuracies": tel["d_real_acc"].tolist(), "disc_fake_accuracies": tel["d_fake_acc"].tolist()}
    epoch = 0
    fatal: Optional[BaseException] = None
    try:
        log(f"Starting training at: {datetime.datetime.now()}")
        log("Parameters:\n" + str(c))
        if diffaug:
            log(f"Differentiable augmentation: {diffaug}")
        if eng.gated:
            log(f"Augmentation probability: {eng.aug_p0:g}" + (f", adaptive: target r_t {eng.ada_target:g}, every {eng.ada_interval} steps, "
                                                              f"{eng.ada_kimg:g} kimg from 0 to 1" if eng.ada else " (fixed)"))
        if eng.bcr:
            log(f"Balanced consistency regularisation: lambda_real {eng.bcr_w[0]:g}, lambda_fake {eng.bcr_w[1]:g}, partner "
                + (f"diffaug's own transform ({diffaug})" if diffaug else f"bcr_aug {bcr_aug}"))
        if eng.spec is not None:
            log(f"Spectral normalisation of the discriminator: set '{spectral_norm}', {eng.spec.n} matrices; checkpoints hold the EFFECTIVE "
                "weights sigma0 W / sigma (discriminator_raw.pth: the raw weights for a resumed run)")
        if conditional:
            log(f"Class-conditional training: {K} classes, label-selected discriminator logit, class-modulated generator")
        if eng.r1:
            log(f"R1 penalty on real images: gamma {eng.r1_gamma:g}, every {eng.r1_interval} step(s) with weight {0.5 * eng.r1_gamma * eng.r1_interval:g}")
        if lr_opts is not None:
            kind, warm, total, fin = lr_opts
            log(f"Learning-rate schedule: {kind}, {warm} warm-up step(s)" + (f", to {fin:g} x base at step {total}" if kind != "constant" else "")
                + f"; base rates D {eng.hyp['lr_d']:g}, G {eng.hyp['lr_g']:g}"
                + (f"; on a plateau of the FID (patience {plateau.patience}) both x {plateau.factor:g}" if plateau is not None else ""))
        if fid_eval is not None:  # before the first step: the real statistics (every image of the set, or one pass over the loader)
            fid_eval.fit_real(dataset if dataset is not None else loader)
            if save_artifacts:
                fid_eval.save_real(os.path.join(dirs.save, "real_stats.npz"))
            log(f"Frechet distance: feature net {fid_eval.tag}, latent seed {fid_eval.seed}, n_real {fid_eval.real['n']}, "
                f"n_fake {fid_eval.n_fake}; real statistics in real_stats.npz; not comparable with published FID")
            if fid_eval.bank is not None:
                log(f"Manifold metrics: {fid_eval.bank['feats'].shape[0]} real feature rows kept"
                    + (f"; precision / recall / density / coverage with k = {manifold_k}" if manifold_k else "")
                    + ("; KID, cubic kernel, one estimate over the full sets" if kid else "") + "; they rank this run's epochs only")
            fid_fn = fid_eval
        for epoch in range(epochs):
            noise = construct_noise()
            if save_artifacts:
                save_images(os.path.join(dirs.noise, f"noise_epoch_{epoch}.png"), noise_as_image(noise), c.batch_size)
            save_samples(epoch, noise)
            losses = None
            for i, (real_images, real_labels) in enumerate(loader if dataset is None else dataset_epoch()):
                if i == 0 and save_artifacts:
                    save_images(os.path.join(dirs.input, f"input_epoch_{epoch}.png"), real_images, c.batch_size)
                if dataset is not None:
                    losses = eng.step()
                    continue
                if conditional and real_labels is None:
                    raise MissingLabelsError("conditional: the data loader yields no labels (SyntheticLoader draws them with labels=classes_count)")
                losses = eng.step(real_images.to(dev), labels=real_labels.to(dev)) if conditional else eng.step(real_images.to(dev))
            if losses is None:
                raise RuntimeError("the data loader produced no batch")
            d_real, d_fake, g = losses.tolist()  # the only host sync of the epoch (training.py:228)
            disc_losses.append(d_real + d_fake)
            gen_losses.append(g)
            history.append((d_real + d_fake, g))
            if fid_fn is not None:
                refresh_ema()
            scored = gan if (gan_ema is None or getattr(fid_fn, "ema", True) is False) else gan_ema
            fid_score = float(fid_fn(scored, epoch)) if fid_fn is not None else float("nan")
            fid_scores.append(fid_score)
            if fid_score < best_fid:
                best_fid = fid_score
                if save_artifacts:
                    torch.save(gan_checkpoint(), os.path.join(dirs.checkpoints, f"best_model_epoch_{epoch}_fid_{int(fid_score)}.pth"))
                    if G_ema is not None:  # refreshed just above, for fid_fn
                        torch.save(G_ema.state_dict(), os.path.join(dirs.checkpoints, "generator_ema.pth"))
            cr = tel_line = ""  # tel_line: the record's four fields, a variable of its own (the blocks below own ``cr``)
            if tel_cap:  # the epoch's steps, read at the synchronisation point above
                import numpy as np
                rec = eng.history()
                dropped = rec.pop("dropped")
                for k_, v_ in rec.items():
                    tel[k_] = v_ if (k_ not in tel or k_.startswith("keys_")) else np.concatenate([tel[k_], v_])
                if dropped:
                    log(f"Warning: telemetry ring of {tel_cap} step(s) is shorter than the epoch: {dropped} step record(s) were dropped")
                if eng.first_nonfinite_step is not None and not nonfinite_logged:
                    nonfinite_logged = True
                    log(f"Non-finite gradient at step {eng.first_nonfinite_step}")
                if save_artifacts:
                    np.savez(os.path.join(dirs.save, "telemetry.npz"), **{k_: np.asarray(v_) for k_, v_ in tel.items()})
                if len(rec["step"]):
                    tel_line = (f" | Disc Real Acc: {rec['d_real_acc'][-1]:.4f} | Disc Fake Acc: {rec['d_fake_acc'][-1]:.4f}"
                           f" | Grad Norm Gen: {rec['gnorm_g_sum'][-1]:.4f} | Grad Norm Disc: {rec['gnorm_d_sum'][-1]:.4f}")
            if eng.bcr:
                cr_real, cr_fake = eng.bcr_losses.tolist()
                cr = f" | Consistency real: {cr_real:.6f}, fake: {cr_fake:.6f}"
            if eng.ada:
                cr += f" | ada_p: {eng.ada_p:.6f}, ada_rt: {eng.ada_rt:.4f}"
            if eng.r1:
                cr += f" | R1: {float(eng.r1_loss):.6f}"
            if eng.lr_opts is not None:  # the rates this epoch's last step ran at
                cr += " | lr_d: {:.9e}, lr_g: {:.9e}".format(*eng.lr)
            if plateau is not None and plateau.step(fid_score):  # takes effect from the next step on
                sd_, sg_ = eng.lr_scales
                eng.set_lr_scale(d=sd_ * plateau.factor, g=sg_ * plateau.factor)
                cr += f" | FID plateau: rate multipliers now {sd_ * plateau.factor:g}, {sg_ * plateau.factor:g}"
            if fid_eval is not None and fid_eval.bank is not None:  # last on the line
                q = {k_: fid_eval.last[k_] for k_ in ("precision", "recall", "density", "coverage", "kid")}
                history[-1] = history[-1] + (q,)
                if manifold_k:
                    cr += " | P: {precision:.4f} R: {recall:.4f} D: {density:.4f} C: {coverage:.4f}".format(**q)
                if kid:
                    cr += f" | KID: {q['kid']:.6e}"
            log(f"Epoch [{epoch}/{epochs}] | Disc Loss: {d_real + d_fake:.8f}, Gen Loss: {g:.4f} | FID: {fid_score:.4f}{tel_line}{cr}")
            if save_artifacts:
                save_figures(dirs.save, disc_losses=disc_losses, gen_losses=gen_losses, fid_scores=fid_scores, **tel_series())
    except KeyboardInterrupt as ke:
        log(f"{ke} raised!")
    except _lib.HipError as e:  # a failed launch / rejected kernel arguments is never a "successful" run
        log(f"HIP engine error: {e}\n{traceback.format_exc()}")
        fatal = e
    except MissingLabelsError as e:
        log(f"{e}")
        fatal = e
    except Exception as e:  # the reference logs and carries on to `finally` (training.py:250-251)
        log(f"Exception: {e}\n{traceback.format_exc()}")
    finally:
        model_path = os.path.join(dirs.save, "final_model.ckpt")
        if save_artifacts and fatal is None:  # no further GPU work, no checkpoint of a broken run
            save_figures(dirs.save, disc_losses=disc_losses, gen_losses=gen_losses, fid_scores=fid_scores, **tel_series())
            torch.save(gan_checkpoint(), model_path)
            if eng.spec is not None:
                torch.save(D.state_dict(), os.path.join(dirs.save, "discriminator_raw.pth"))
            torch.save(eng.state_dict(), os.path.join(dirs.save, "engine_state.pth"))
            save_samples(epoch, construct_noise())
            if G_ema is not None:  # refreshed by save_samples
                torch.save(G_ema.state_dict(), os.path.join(dirs.save, "generator_ema.pth"))
        took = datetime.datetime.now() - dirs.start
        if fatal is None and save_artifacts:
            log(f"Run took {took}. Saving the model to: {model_path}")
        elif fatal is not None:  # the log of a failed run must not claim a checkpoint that was never written
            log(f"Run took {took}. NO checkpoint was written: the run ended on {type(fatal).__name__}")
        else:
            log(f"Run took {took}.")
        _log_file = None
    if fatal is not None:
        raise fatal
    out = {"discriminator": D, "generator": G, "gan": gan, "engine": eng, "history": history, "dirs": dirs}
    if G_ema is not None:
        refresh_ema()
        out["generator_ema"] = G_ema
    if fid_eval is not None:
        out["fid"] = fid_eval
    if tel_cap:
        out["telemetry"] = tel
    return out
