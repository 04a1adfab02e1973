"""numpy / fp64 restatements for the Frechet-distance tests: two-pass mean and covariance, the Gram update, the one-pass finish, the
reference's uint8 treatment of images and the Frechet formula in torchmetrics' OWN form, eigvals(S1 S2).sqrt().real.sum().  A plain
helper module (imported like dataset_ref); nothing here imports the product code."""
import numpy as np


def two_pass(x):
    """(mean [d], cov [d, d]) of the rows of x, fp64, the textbook way: centre first, then (Xc^T Xc) / (n - 1)"""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    xc = x - mean
    return mean, xc.T @ xc / (x.shape[0] - 1)


def gram_update(sum_, gram, x):
    """sum + sum_i x_i and gram + X^T X in fp64"""
    x = np.asarray(x, dtype=np.float64)
    return sum_ + x.sum(0), gram + x.T @ x


def gram_update_int(sum_, gram, x):
    """the same in int64, for integer-valued features: exact"""
    x = np.asarray(x).astype(np.int64)
    return sum_ + x.sum(0), gram + x.T @ x


def finish(sum_, gram, n):
    """torchmetrics' one-pass formula: mean = sum / n, cov = (gram - n mean (x) mean) / (n - 1)"""
    mean = sum_ / n
    return mean, (gram - n * np.outer(mean, mean)) / (n - 1)


def frechet_torchmetrics(mu1, cov1, mu2, cov2):
    """torchmetrics.image.fid._compute_fid: a = |mu1 - mu2|^2, b = tr S1 + tr S2, c = eigvals(S1 S2).sqrt().real.sum(); a + b - 2 c"""
    mu1, mu2, cov1, cov2 = (np.asarray(t, dtype=np.float64) for t in (mu1, mu2, cov1, cov2))
    a = ((mu1 - mu2) ** 2).sum()
    b = np.trace(cov1) + np.trace(cov2)
    c = np.sqrt(np.linalg.eigvals(cov1 @ cov2).astype(np.complex128)).real.sum()
    return float(a + b - 2 * c)


def frechet_sqrtm(mu1, cov1, mu2, cov2):
    """the original form (Heusel et al. 2017): tr (S1 S2)^(1/2) by scipy.linalg.sqrtm"""
    from scipy import linalg
    mu1, mu2, cov1, cov2 = (np.asarray(t, dtype=np.float64) for t in (mu1, mu2, cov1, cov2))
    root = linalg.sqrtm(cov1 @ cov2)
    return float(((mu1 - mu2) ** 2).sum() + np.trace(cov1) + np.trace(cov2) - 2 * np.real(np.trace(root)))


def table(mean, std):
    """fp32 [C, 256] decode table: ((v / 255) - mean) / std in fp32, rounded to bf16 (round to nearest even on the top 16 bits)"""
    v = (np.arange(256, dtype=np.float32) / np.float32(255))[None, :]
    m = np.asarray(mean, dtype=np.float32).reshape(-1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(-1, 1)
    t = ((v - m) / s).astype(np.float32)
    bits = t.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(t.shape)


def quantize(x, tab):
    """src/v2/utils.py:165-166 on a float [n, C, H, W] batch, then the table: clamp to [-1, 1], ((x * 0.5 + 0.5) * 255) truncated to
    uint8 (every step in fp32, as torch computes it), tab[c, byte]"""
    x = np.clip(np.asarray(x, dtype=np.float32), np.float32(-1), np.float32(1))
    q = ((x * np.float32(0.5) + np.float32(0.5)) * np.float32(255)).astype(np.uint8)
    c = np.arange(x.shape[1]).reshape(1, -1, 1, 1) % tab.shape[0]
    return tab[np.broadcast_to(c, q.shape), q]
