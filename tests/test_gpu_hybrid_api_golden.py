"""The public API of ``BatchedHybrid`` and ``DeviceHybrid`` against a recording of it (``tests/golden/hybrid_api_trace.npz``, made
by ``tests/golden/make_hybrid_api_fixture.py`` before the two loops were given one base class): the session of
``tests/support/hybrid_api_scenario.py`` -- ticks, a ``reset()`` in the middle of the episode, ticks again, what the loop and its
tracker hold afterwards, a recorded ``run`` -- is replayed leg by leg and every recorded array compared bit for bit.  The kernels
are those of the recording; what can differ is what the host sets up, restores and accounts for around them."""
import pytest

from support import hybrid_api_scenario as scenario

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recording():
    want = scenario.load()
    scenario.check_not_vacuous(want)
    assert {k.split(".")[0] for k in want} == set(scenario.LEGS)
    return want


@pytest.mark.parametrize("leg", list(scenario.LEGS))
def test_the_leg_replays_the_recording_bit_for_bit(leg, recording):
    want = {k: v for k, v in recording.items() if k.startswith(leg + ".")}
    assert len(want) >= 13 and (leg not in scenario.RUN_LEGS or f"{leg}.run.ref_traj.{scenario.B_RUN - 1}" in want)
    bad = scenario.differences(scenario.run_leg(leg), want)
    assert not bad, bad
