"""The fused step's call sequence, pinned: two eager steps of every configuration of tests/step_trace.py make exactly the C calls -
names, order, scalars, streams, and every pointer as (allocation, byte offset) - that tests/golden/step_trace.json recorded, and an
option that is off leaves the step launch for launch the plain one.  No tolerance: the traces are compared for equality."""
import functools
import json

import pytest

import step_trace as stt

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(stt.FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _plain():
    return stt.trace()


def _first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} calls, expected {len(want)}: {[c[0] for c in got]} against {[c[0] for c in want]}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"call {i}: {g} against {w}"
    return None


def test_fixture_covers_every_configuration():
    fx = _fixture()
    assert sorted(fx["traces"]) == sorted(stt.CONFIGS) and fx["ext_allowed"] == 0 and len(fx["commit"]) == 40
    names = {c[0] for t in fx["traces"].values() for c in t}
    for must in ("vg_vit_backward", "vg_gan_loss", "vg_gan_loss_pair", "vg_bcr_loss", "vg_ada_update", "vg_diffaug_fwd", "vg_diffaug_p_fwd",
                 "vg_diffaug_bwd", "vg_diffaug_p_bwd", "vg_adamw_step", "vg_adamw_ema_step", "vg_grad_clip", "vg_diversity_loss",
                 "vg_vit_penalty", "vg_spectral_project", "vg_spectral_update"):
        assert must in names, must
    assert any(a == "s1" for c in fx["traces"]["two_stream"] for a in c[1])


@pytest.mark.parametrize("name", list(stt.CONFIGS))
def test_step_makes_the_recorded_calls(name):
    fx = _fixture()
    calls, ext = stt.trace(**stt.CONFIGS[name]) if name != "plain" else _plain()
    assert ext == fx["ext_allowed"], f"{ext} pointers outside every known allocation"
    assert _first_difference(calls, fx["traces"][name]) is None, _first_difference(calls, fx["traces"][name])


@pytest.mark.parametrize("name", list(stt.OFF))
def test_an_option_that_is_off_is_the_plain_step(name):
    calls, ext = stt.trace(**stt.OFF[name])
    assert ext == 0
    assert _first_difference(calls, _plain()[0]) is None, _first_difference(calls, _plain()[0])
