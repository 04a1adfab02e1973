"""DeviceDataset: a uint8 image set kept in device memory, from which the fused step fetches its own real batch.

The reference feeds CIFAR-10 through a host ``DataLoader`` (src/v2/utils.py:100-121: ``ToTensor``, ``Normalize(0.5)``, shuffle,
drop_last).  Here the whole set (150 MB as uint8) lives on the device and ONE launch, ``vg_dataset_fetch``, draws, decodes and labels
the batch of a step from the device step counter - the rule is in include/vitgan_hip.h; ``indices`` / ``flips`` below are its host
mirrors and ``decode`` is the host form of the decode (the same table), so ``decode(indices(s, B), flips(s, B))`` is bit for bit the
batch step ``s`` trains on.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Union

import numpy as np
import torch

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SITE_PERM, SITE_FLIP = 4, 5  # the engine's site numbering: 0-2 the augmentations, 3 the fake labels
LDS_MAX = 160 * 1024         # one image plus the table must fit one CU's LDS
LAYOUTS = {"nchw": 0, "nhwc": 1}


def _site_key(seed: int, site: int) -> int:
    z = (int(seed) + 0x9E3779B97F4A7C15 * (site + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def _h(key, idx):
    """the counter hash of the kernels (vg_drop_word) on uint64 arrays holding 32-bit values"""
    m = np.uint64(M32)
    x = (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.asarray(key, dtype=np.uint64)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def data_seed(seed: int) -> int:
    """The dataset's stream of an engine built with ``seed``: WITHOUT the rank, so all ranks walk one permutation."""
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x2545F4914F6CDD1D) & M64


def perm_epoch(p, N: int, epoch: int, seed: int) -> np.ndarray:
    """The keyed bijection of [0, N) at the positions ``p``: a 4-round Feistel network on 2k bits, cycle-walked."""
    N = int(N)
    k = max(1, ((N - 1).bit_length() + 1) // 2)
    m = np.uint64((1 << k) - 1)
    ke = _h(_h(_site_key(seed, SITE_PERM), 0), int(epoch) & M32)
    keys = [_h(ke, r + 1) for r in range(4)]
    x = np.array(p, dtype=np.uint64).reshape(-1)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint64(k), v & m
        for key in keys:
            L, R = R, L ^ (_h(key, R) & m)
        x[todo] = (L << np.uint64(k)) | R
        todo = x >= np.uint64(N)
    return x.astype(np.int64)


class DeviceDataset:
    """``images``: uint8 tensor or array, [N, C, H, W] or [N, H, W, C] with H == W (``layout``: "nchw", "nhwc" or "auto" = the one whose
    channel axis is <= 4; a tie raises).  ``labels``: integers [N] or None.  ``mean`` / ``std``: a number or one per channel - the
    ``Normalize`` behind ``ToTensor``.  ``flip``: mirror an image left to right with probability 1/2, drawn per visit.  ``shuffle``:
    visit the set in a fresh keyed permutation every epoch (off: in storage order).  ``device``: where the set lives; an engine moves it
    to its own device (``to``), once, and it stays uint8 there."""

    def __init__(self, images, labels=None, layout: str = "auto", mean: Union[float, Sequence[float]] = 0.5,
                 std: Union[float, Sequence[float]] = 0.5, flip: bool = False, shuffle: bool = True, device=None):
        images = torch.as_tensor(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f"images must be a uint8 [N, C, H, W] or [N, H, W, C] tensor, got {images.dtype} {tuple(images.shape)}")
        first, last = images.shape[1] <= 4, images.shape[3] <= 4
        if layout == "auto":
            if first == last:
                raise ValueError(f"layout='auto' cannot tell the channel axis of {tuple(images.shape)}; pass layout='nchw' or 'nhwc'")
            layout = "nchw" if first else "nhwc"
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'auto', 'nchw' or 'nhwc', got {layout!r}")
        self.layout = LAYOUTS[layout]
        N, (C, H, W) = int(images.shape[0]), (images.shape[1:] if self.layout == 0 else (images.shape[3], images.shape[1], images.shape[2]))
        if H != W:
            raise ValueError(f"images must be square, got {H} x {W}")
        self.N, self.C, self.IH = N, int(C), int(H)
        per = self.C * self.IH * self.IH
        if self.C > 4 or (self.IH * self.IH) % 8 or per % 16 or per + 512 * self.C > LDS_MAX or N >= 2 ** 31:
            raise ValueError(f"DeviceDataset: vg_dataset_fetch takes C <= 4, IH*IH % 8 == 0, C*IH*IH % 16 == 0, one image plus the table "
                             f"inside {LDS_MAX} bytes and N < 2^31; got N={N}, C={self.C}, IH={self.IH}")
        self.images = images.contiguous()
        self.labels: Optional[torch.Tensor] = None
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.is_floating_point() or labels.dtype == torch.bool or tuple(labels.shape) != (N,):
                raise ValueError(f"labels must be an integer tensor of shape [{N}], got {labels.dtype} {tuple(labels.shape)}")
            self.labels = labels.to(torch.int32).contiguous()
        self.mean, self.std = self._per_channel(mean, "mean"), self._per_channel(std, "std")
        if any(not s > 0.0 for s in self.std):
            raise ValueError(f"std must be positive, got {std!r}")
        self.flip, self.shuffle = bool(flip), bool(shuffle)
        self.flags = int(self.shuffle) | (int(self.flip) << 1)
        # the decode table: ToTensor and Normalize as torch's fp32 computes them, then the rounding the step's bf16 cast applies
        v = torch.arange(256, dtype=torch.float32) / 255
        m_, s_ = (torch.tensor(t, dtype=torch.float32).reshape(-1, 1) for t in (self.mean, self.std))
        self.lut_bf16 = ((v.reshape(1, 256) - m_) / s_).to(torch.bfloat16).contiguous()  # [C, 256]: what the kernel reads
        self.lut = self.lut_bf16.float()
        if device is not None:
            self.to(device)

    def _per_channel(self, v, what: str):
        try:
            out = [float(v)] * self.C if not isinstance(v, (list, tuple, np.ndarray, torch.Tensor)) else [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a number or one per channel, got {v!r}") from None
        if len(out) != self.C or not all(np.isfinite(out)):
            raise ValueError(f"{what} must be a finite number or {self.C} of them (one per channel), got {v!r}")
        return out

    @classmethod
    def from_cifar10_bin(cls, directory: str, train: bool = True, **kw) -> "DeviceDataset":
        """The CIFAR-10 binary version from a directory already on disk (``data_batch_1..5.bin`` or ``test_batch.bin``: records of one
        label byte and 3072 bytes CHW).  It never downloads: a missing file is an error."""
        names = [f"data_batch_{i}.bin" for i in range(1, 6)] if train else ["test_batch.bin"]
        parts = []
        for name in names:
            path = os.path.join(directory, name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{path} is missing (the CIFAR-10 binary batches are read from disk, never downloaded)")
            raw = np.fromfile(path, dtype=np.uint8)
            if raw.size == 0 or raw.size % 3073:
                raise ValueError(f"{path}: {raw.size} bytes is not a whole number of 3073-byte records")
            parts.append(raw.reshape(-1, 3073))
        rec = np.concatenate(parts)
        kw.setdefault("layout", "nchw")
        return cls(torch.from_numpy(rec[:, 1:].reshape(-1, 3, 32, 32).copy()), torch.from_numpy(rec[:, 0].astype(np.int32)), **kw)

    def to(self, device) -> "DeviceDataset":
        """Move the set (uint8), its labels and the table to ``device`` in place; a no-op when it is there."""
        device = torch.device(device)
        self.images = self.images.to(device)
        self.lut_bf16, self.lut = self.lut_bf16.to(device), self.lut.to(device)
        if self.labels is not None:
            self.labels = self.labels.to(device)
        return self

    def __len__(self) -> int:
        return self.N

    def steps_per_epoch(self, B: int, world: int = 1) -> int:
        """Whole global batches per epoch; the remainder is dropped, as with ``drop_last``."""
        B, world = int(B), int(world)
        if B < 1 or world < 1:
            raise ValueError(f"steps_per_epoch: B and world must be positive, got {B}, {world}")
        nb = self.N // (B * world)
        if nb < 1:
            raise ValueError(f"the dataset holds {self.N} images, fewer than one global batch of {B} x {world}")
        return nb

    def _positions(self, step: int, B: int, rank: int, world: int):
        if not 0 <= int(rank) < int(world):
            raise ValueError(f"rank {rank} is outside [0, {world})")
        nb = self.steps_per_epoch(B, world)
        s = int(step) & M32
        epoch, j = divmod(s, nb)
        return epoch, (j * int(world) + int(rank)) * int(B) + np.arange(int(B), dtype=np.int64)

    def indices(self, step: int, B: int, rank: int = 0, world: int = 1, seed: int = 0) -> torch.Tensor:
        """The B dataset indices (int64, CPU) rank ``rank`` fetches at device step counter ``step`` (0 on the first step); ``seed``: the
        kernel's seed argument - an engine's is ``engine.data_seed``.  A pure host mirror of the kernel's rule."""
        epoch, p = self._positions(step, B, rank, world)
        return torch.from_numpy(perm_epoch(p, self.N, epoch, seed) if self.shuffle else p)

    def flips(self, step: int, B: int, rank: int = 0, world: int = 1, seed: int = 0) -> torch.Tensor:
        """Which of those B images are mirrored left to right (bool, CPU); all False with ``flip=False``."""
        epoch, p = self._positions(step, B, rank, world)
        if not self.flip:
            return torch.zeros(int(B), dtype=torch.bool)
        kf = _h(_h(_site_key(seed, SITE_FLIP), 0), epoch & M32)
        return torch.from_numpy((_h(kf, p.astype(np.uint64)) >> np.uint64(31)).astype(bool))

    def decode(self, indices, flips=None) -> torch.Tensor:
        """fp32 [n, C, IH, IH] of the images ``indices`` through the table (every value is a bf16), mirrored where ``flips`` says so; on
        the device the set lives on."""
        dev = self.images.device
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).to(dev)
        x = self.images[idx]
        if self.layout == 1:
            x = x.permute(0, 3, 1, 2)
        if flips is not None:
            f = torch.as_tensor(flips, dtype=torch.bool).reshape(-1, 1, 1, 1).to(dev)
            x = torch.where(f, x.flip(3), x)
        c = torch.arange(self.C, device=dev).reshape(1, -1, 1, 1).expand_as(x)
        return self.lut[c, x.long()].contiguous()
