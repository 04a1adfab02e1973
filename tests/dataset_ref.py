"""The device-resident dataset's rule restated off the device, from the text of include/vitgan_hip.h alone (a plain helper module,
imported like cond_ref / diffaug_ref; no product code): the keyed permutation of an epoch - a 4-round Feistel network on 2k bits with
cycle walking - the positions of a rank's batch, the flip draws and the decode table, in plain Python integers and numpy uint32
arithmetic modulo 2^32.  ``perm_epoch`` takes ``walk=False`` to plant the defect "p % N in place of cycle walking"."""
import numpy as np
import torch

from drop_ref import M32, h, site_key  # noqa: F401  (the host key and the counter hash of the dropout masks)
SITE_PERM, SITE_FLIP = 4, 5
SIZES = (1, 2, 3, 5, 16, 17, 50, 53, 1000, 4096, 4097, 50000, 65537, 2 ** 20)
EPOCHS = (0, 1, 7, 12345)


def half_width(N: int) -> int:
    """k = max(1, ceil(bitlength(N - 1) / 2))"""
    return max(1, -(-int(N - 1).bit_length() // 2))


def feistel_pass(x, k: int, keys):
    m = np.uint32((1 << k) - 1)
    L, R = x >> np.uint32(k), x & m
    for key in keys:
        L, R = R, L ^ (h(key, R) & m)
    return (L << np.uint32(k)) | R


def perm_epoch(p, N: int, epoch: int, seed: int, walk: bool = True, count=None):
    """index of the positions ``p`` in epoch ``epoch``; ``count`` (a list) receives the mean number of passes per position"""
    k = half_width(N)
    ke = h(h(site_key(seed, SITE_PERM), 0), epoch & M32)
    keys = [h(ke, r + 1) for r in range(4)]
    x = np.array(p, dtype=np.uint32).reshape(-1)
    if not walk:  # the planted defect: one pass, folded into the range
        return (feistel_pass(x, k, keys).astype(np.int64) % N)
    todo, passes = np.ones(x.shape, dtype=bool), 0
    while todo.any():
        passes += int(todo.sum())
        x[todo] = feistel_pass(x[todo], k, keys)
        todo = x >= N
    if count is not None:
        count.append(passes / max(1, x.size))
    return x.astype(np.int64)


def perm_epochs(p: int, N: int, epochs, seed: int):
    """the index at ONE position ``p`` in every epoch of ``epochs`` (the same rule, the epochs as the vector axis)"""
    k = half_width(N)
    ke = h(h(site_key(seed, SITE_PERM), 0), np.asarray(epochs, dtype=np.uint32))
    keys = [h(ke, r + 1) for r in range(4)]
    x = np.full(ke.shape, p, dtype=np.uint32)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        x[todo] = feistel_pass(x[todo], k, [key[todo] for key in keys])
        todo = x >= N
    return x.astype(np.int64)


def positions(step: int, N: int, B: int, rank: int = 0, world: int = 1):
    """(epoch, the B positions of rank ``rank``) at device step counter ``step``"""
    nb = N // (B * world)
    epoch, j = divmod(step & M32, nb)
    return epoch, (j * world + rank) * B + np.arange(B, dtype=np.int64)


def indices(step: int, N: int, B: int, rank: int = 0, world: int = 1, seed: int = 0, shuffle: bool = True, walk: bool = True):
    epoch, p = positions(step, N, B, rank, world)
    return perm_epoch(p, N, epoch, seed, walk) if shuffle else p


def flips(step: int, N: int, B: int, rank: int = 0, world: int = 1, seed: int = 0, flip: bool = True):
    epoch, p = positions(step, N, B, rank, world)
    if not flip:
        return np.zeros(B, dtype=bool)
    kf = h(h(site_key(seed, SITE_FLIP), 0), epoch & M32)
    return (h(kf, p.astype(np.uint32)) >> np.uint32(31)).astype(bool)


def table(mean, std) -> torch.Tensor:
    """fp32 [C, 256]: ToTensor and Normalize in torch fp32, then the bf16 rounding of the step's input cast"""
    rows = [(((torch.arange(256, dtype=torch.float32) / 255) - m) / s).to(torch.bfloat16).float() for m, s in zip(mean, std)]
    return torch.stack(rows)


def decode(images: torch.Tensor, layout: int, idx, flip, mean, std) -> torch.Tensor:
    """torch gather, flip and table on the host: fp32 [n, C, IH, IH]"""
    x = images[torch.as_tensor(np.asarray(idx), dtype=torch.int64)]
    if layout == 1:
        x = x.permute(0, 3, 1, 2)
    x = x.contiguous()
    for n, f in enumerate(np.asarray(flip).reshape(-1)):
        if f:
            x[n] = x[n].flip(2)
    lut = table(mean, std)
    return torch.stack([lut[c][x[:, c].long()] for c in range(x.shape[1])], dim=1)
