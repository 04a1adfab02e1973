"""The attention kernels, pinned by bytes per entry point: every case of tests/attn_pins.py (forward + backward of the dot-product,
fp8, L2, long and CLS forms, and the double backward, at the sequence lengths where each branch can go wrong) gives the SHA-256
digests of its outputs that tests/golden/attn_digest.json recorded with the library of the commit it names.  No tolerance: the
kernels share their phases and tiles through csrc/vg_attn.h, and a moved fusion or a changed operand order changes a digest."""
import functools
import json

import pytest

import attn_pins as ap

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(ap.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_cases():
    fx = _fixture()
    assert len(fx["commit"]) == 40
    assert len(ap.digest_cases()) == 81
    assert sorted(fx["digests"]) == sorted(ap.digest_cases())
    for case_id, d in fx["digests"].items():
        kind = ap.digest_cases()[case_id][0]
        assert set(d) == ({"d_do", "d_qkv"} if kind == "bwd_bwd" else {"o", "lse", "dqkv"}), case_id


@pytest.mark.parametrize("case_id", list(ap.digest_cases()))
def test_digests_are_the_recorded_ones(case_id):
    want = _fixture()["digests"].get(case_id)
    assert want is not None, f"{case_id} is missing from the fixture"
    got = ap.digest(case_id)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
