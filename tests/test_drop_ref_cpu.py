"""drop_ref, the dropout mask restated from include/vitgan_hip.h: the quantisation edges against hand-computed thresholds, the key,
the hash and the byte rule against plain Python integers written out a second time, and the properties the GPU test's cases rely on."""
import numpy as np
import pytest

import drop_ref as R

# p exact in fp32 (or given as fp32), so Python's double and C's float agree on the product 256 p
EDGES = [
    (0.0, 0),
    (1 / 512, 0),                  # 0.5 -> 0: halves go to even
    (3 / 512, 2),                  # 1.5 -> 2
    (1 / 256, 1),
    (0.5, 128),
    (255 / 256, 255),
    (float(np.float32(0.999)), 255),  # 255.744 rounds to 256: clamped
]


@pytest.mark.parametrize("p, thr", EDGES)
def test_threshold_edges(p, thr):
    assert float(np.float32(p)) == p  # the table's premise
    assert R.threshold(p) == thr


def test_scale_is_the_fp32_quotient():
    assert R.scale(0) == np.float32(1.0) and R.scale(128) == np.float32(2.0) and R.scale(255) == np.float32(256.0)
    assert R.scale(26).dtype == np.float32 and float(R.scale(26)) == float(np.float32(256.0 / 230.0))  # 256 / 230: one rounding
    assert R.scale(2) == np.float32(np.float32(256.0) / np.float32(254.0))


def _key_int(seed, site):
    z = (seed + 0x9E3779B97F4A7C15 * (site + 1)) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    return (z ^ (z >> 32)) % 2 ** 32


def _h_int(k, i):
    x = (i * 0x9E3779B1 + k) % 2 ** 32
    x ^= x >> 16
    x = (x * 0x7FEB352D) % 2 ** 32
    x ^= x >> 15
    x = (x * 0x846CA68B) % 2 ** 32
    return x ^ (x >> 16)


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 64 - 1])
@pytest.mark.parametrize("site", [0, 4, 101])
def test_key_hash_and_step_mix_against_plain_integers(seed, site):
    key = R.site_key(seed, site)
    assert key == _key_int(seed, site) and 0 <= key < 2 ** 32
    idx = [0, 1, 2, 255, 256, 2 ** 31, 2 ** 32 - 1]
    assert [int(v) for v in R.h(key, np.array(idx, dtype=np.uint32))] == [_h_int(key, i) for i in idx]
    assert int(R.step_mix(key, None)) == key
    for step in (0, 1, 0xFFFFFFFF):
        assert int(R.step_mix(key, step)) == key ^ ((step * 0x9E3779B1 + 0x7F4A7C15) % 2 ** 32)
    assert int(R.step_mix(key, 0)) != key  # no counter is not a counter of 0


@pytest.mark.parametrize("step", [None, 0, 1, 0xFFFFFFFF])
def test_mask_is_the_byte_rule(step):
    p, seed, site, n = 0.5, 1234, 4, 1028
    keep, scale = R.mask(p, seed, site, step, n)
    assert keep.dtype == bool and keep.shape == (n,) and scale == np.float32(2.0)
    k = _key_int(seed, site)
    if step is not None:
        k ^= (step * 0x9E3779B1 + 0x7F4A7C15) % 2 ** 32
    want = [((_h_int(k, e >> 2) >> (8 * (e & 3))) & 0xFF) >= 128 for e in range(n)]  # byte 0 the lowest
    assert keep.tolist() == want
    assert 0 < keep.sum() < n


def test_mask_edges_and_distinctness():
    keep, scale = R.mask(0.0, 7, 3, None, 1024)
    assert keep.all() and scale == np.float32(1.0)  # thr 0: every byte is >= 0
    keep, scale = R.mask(1 / 512, 7, 3, None, 1024)
    assert keep.all() and scale == np.float32(1.0)  # quantised to no dropout
    k255, s255 = R.mask(255 / 256, 7, 3, None, 1 << 16)
    assert s255 == np.float32(256.0) and abs(int(k255.sum()) - 256) < 80  # survivors: byte 0xFF only, 1 in 256
    a = R.mask(0.5, 7, 3, None, 4096)[0]
    assert not np.array_equal(a, R.mask(0.5, 7, 3, 0, 4096)[0]) and not np.array_equal(a, R.mask(0.5, 7, 4, None, 4096)[0])
    assert not np.array_equal(a, R.mask(0.5, 8, 3, None, 4096)[0])
    assert abs(float(a.mean()) - 0.5) < 0.03
    # a prefix of a longer mask is the shorter mask: the index is the element's position alone
    assert np.array_equal(a[:1020], R.mask(0.5, 7, 3, None, 1020)[0])
