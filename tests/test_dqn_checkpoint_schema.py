"""The checkpoint format of ``DqnLearner`` against its recording (``tests/golden/dqn_checkpoint_schema.json``, written by
``tests/golden/make_dqn_checkpoint_schema.py`` on the revision before the replay buffers were merged into one): every nested
key of ``state_dict()`` in order, with the type of numbers and lists and the dtype and shape of tensors, for uniform and
prioritized replay on both environments and the eager, graph and fused updates.  A renamed, missing, extra or reordered key
fails; tensor values are the resume tests' business."""
import pytest

from support import dqn_checkpoint_schema as schema

RECORDED = schema.load()


def test_the_recording_holds_every_leg():
    assert list(RECORDED) == list(schema.LEGS) and all(len(walk) > 70 for walk in RECORDED.values())


def test_a_changed_key_is_a_difference():
    want = RECORDED["ray_per"]
    i = [path for path, _ in want].index("/str:buffer/str:pos")
    assert schema.differences(want, want) == []
    assert schema.differences(want[:i] + [want[i + 1], want[i]] + want[i + 2:], want)[0][0] == i       # reordered
    assert schema.differences(want[:i] + want[i + 1:], want)[0][0] == i                                 # missing
    assert schema.differences(want[:i] + [["/str:buffer/str:extra", "int"]] + want[i:], want)[0][0] == i
    assert schema.differences(want[:-1], want) == [(len(want) - 1, None, want[-1])]


def _compare(leg):
    got = schema.schema(leg)
    bad = schema.differences(got, RECORDED[leg])
    print(f"{leg}: {len(got)} entries, recorded {len(RECORDED[leg])}, {len(bad)} differ")
    assert not bad, bad[:5]


@pytest.mark.parametrize("leg", schema.CPU_LEGS)
def test_checkpoint_keeps_the_recorded_format(leg):
    _compare(leg)


@pytest.mark.gpu
@pytest.mark.parametrize("leg", schema.GPU_LEGS)
def test_checkpoint_keeps_the_recorded_format_on_the_gpu(leg):
    _compare(leg)
