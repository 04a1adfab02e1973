"""The dropout mask restated off the device, from the text of include/vitgan_hip.h (vg_dropout_apply) alone: a plain helper module,
imported like exact_util; no product code.  Integer numpy arithmetic modulo 2^32 behind the 64-bit host key.  The key and the counter
hash are also what the augmentation, the label draws and the dataset's permutation are built on: diffaug_ref, cond_ref and dataset_ref
import them from here."""
import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def site_key(seed: int, site: int) -> int:
    """key = fold(splitmix64(seed + 0x9E3779B97F4A7C15 (site + 1))) -> 32 bits"""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(site) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def h(k, i):
    """the counter hash, on numpy uint32 arrays (or scalars), modulo 2^32"""
    with np.errstate(over="ignore"):
        x = (np.asarray(i, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.asarray(k, dtype=np.uint32)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x = (x * np.uint32(0x7FEB352D)).astype(np.uint32)
        x ^= x >> np.uint32(15)
        x = (x * np.uint32(0x846CA68B)).astype(np.uint32)
        x ^= x >> np.uint32(16)
    return x


def step_mix(key, step):
    """step_dev ? key ^ (step_dev[0] 0x9E3779B1 + 0x7F4A7C15) : key; ``step`` None = no device counter (not a counter of 0);
    step may be an array"""
    if step is None:
        return np.uint32(key)
    with np.errstate(over="ignore"):
        s = np.asarray(np.asarray(step, dtype=np.uint64) & np.uint64(M32), dtype=np.uint32)
        return np.uint32(key) ^ (s * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15)).astype(np.uint32)


def threshold(p) -> int:
    """the fp32 product 256 p rounded to an integer, halves to even, clamped to [0, 255]"""
    t = np.rint(np.float32(p) * np.float32(256.0))
    return int(min(max(t, 0.0), 255.0))


def scale(thr: int) -> np.float32:
    """the fp32 quotient 256 / (256 - thr); 1 at thr = 0"""
    return np.float32(256.0) / np.float32(256 - thr)


def mask(p, seed: int, site: int, step, n: int):
    """(keep, scale): keep[e] (bool [n]) iff byte (e & 3) of h(k, e >> 2) is >= thr, byte 0 the lowest; scale in fp32"""
    thr = threshold(p)
    e = np.arange(n, dtype=np.uint64)
    word = h(step_mix(site_key(seed, site), step), (e >> np.uint64(2)).astype(np.uint32))
    byte = (word >> (np.uint32(8) * (e & np.uint64(3)).astype(np.uint32))) & np.uint32(0xFF)
    return byte >= np.uint32(thr), scale(thr)
