"""``DqnLearner.learn`` against a recording of itself made BEFORE it was written as one loop over two bound strategies
(``tests/golden/dqn_learner_trace.npz``, recorded by ``tests/golden/make_dqn_learner_fixture.py``): every leg of
``tests/support/dqn_learner_scenario.py`` -- eager, graph, PER, the fused one-launch round, fused around the tree, PER inside
the launch, collection inside the launch with the fused and with the plain trainer, the image environment -- run to a checkpoint
in mid-schedule, continued in a fresh learner, and compared bit for bit: the counters and the loss of every round, parameters,
Adam's state, the whole replay ring, the tree, the episode statistics, the stream serials and what ``learn`` returned."""
import pytest

from support import dqn_learner_scenario as scenario

WANT = scenario.load()
LEGS = scenario.legs_of(WANT)


def test_the_recording_pins_something():
    assert set(scenario.OWN_KERNEL_LEGS) <= set(LEGS)
    scenario.check_not_vacuous(WANT, LEGS)


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
def test_learner_replays_its_recording_bit_for_bit(leg):
    got = scenario.run_leg(leg)
    want = {k: v for k, v in WANT.items() if k.startswith(leg + ".")}
    assert len(want) >= 20
    assert scenario.differences(got, want) == []
