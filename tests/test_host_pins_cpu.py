"""The workspace carve and the flat parameter layouts, pinned value for value: tests/golden/host_carve.json holds, for every
geometry of tests/host_pins.py and B in {1, 4, 8, 16, 256}, the three workspace sizes, every field of vg_vit_ws_map /
vg_gen_ws_map and every field of vg_vit_layout / vg_gen_layout as the commit named in the fixture computed them.  No GPU."""
import json

import host_pins as hp


def _fixture():
    with open(hp.CARVE_FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_geometry_and_batch():
    fx = _fixture()
    assert len(fx["commit"]) == 40
    assert sorted(fx["table"]) == sorted(f"{g}/B{B}" for g in list(hp.VIT) + list(hp.GEN) for B in hp.BATCHES)
    for key, row in fx["table"].items():
        assert row["ws_bytes"] > 0 and row["ws_map"]["total"] == row["ws_bytes"], key
        assert ("penalty_ws_bytes" in row) == key.startswith("V"), key


def test_carve_and_layouts_are_the_recorded_ones():
    fx, got = _fixture()["table"], hp.carve_table()
    assert sorted(got) == sorted(fx)
    for key in fx:
        for part in fx[key]:
            assert got[key][part] == fx[key][part], (key, part, got[key][part], fx[key][part])
