"""The launch lists of the C host code, pinned by bytes: every case of tests/host_pins.py (forward + backward of both networks in
every schedule, the gradient penalty and R1) gives the SHA-256 digests - of each output, of the gradient buffer and of each whole
workspace after the last call - that tests/golden/host_digest.json recorded at the commit it names.  No tolerance: a dropped,
added or reordered launch, a wrong block stride or a wrong scratch set changes a digest."""
import functools
import json

import pytest

import host_pins as hp

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(hp.DIGEST_FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_cases():
    fx = _fixture()
    assert len(fx["commit"]) == 40
    assert sorted(fx["digests"]) == sorted(hp.digest_cases())
    for case_id, d in fx["digests"].items():
        kind = hp.digest_cases()[case_id][0]
        want = {"vit": {"logits", "G", "ws"}, "pen": {"penalty_out", "G", "ws", "ws_pen"}, "gen": {"img", "G", "ws"}}[kind]
        assert want <= set(d) <= want | {"d_img"}, case_id
        assert ("d_img" in d) == (kind == "vit" and hp.digest_cases()[case_id][1]["dimg"] == 1), case_id


@pytest.mark.parametrize("case_id", list(hp.digest_cases()))
def test_digests_are_the_recorded_ones(case_id):
    want = _fixture()["digests"].get(case_id)
    assert want is not None, f"{case_id} is missing from the fixture"
    got = hp.digest(case_id)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
