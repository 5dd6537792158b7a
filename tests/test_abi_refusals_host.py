"""The refusals of the side modules' C-ABI entries, without a GPU: every case of tests/support/abi_refusal_cases.py against
``tests/golden/abi_refusals.json`` -- recorded on the revision before the entries' host plumbing moved into csrc/abi_host.hpp --
return code and text character for character; and the seven error slots, which a refusal through another entry leaves alone."""
import itertools

import pytest

from support import abi_refusal_cases as rc


@pytest.fixture(scope="module")
def lib():
    return rc.library()


def text(lib, slot):
    return getattr(lib, rc.SLOTS[slot])().decode()


def test_every_refusal_keeps_its_code_and_its_words(lib):
    want, got = rc.load(), rc.run(lib)
    assert [row[:2] for row in got] == [row[:2] for row in want]              # the same cases in the same order
    assert len(want) == 445 and all(row[2] == -1 and row[3] and "hipSetDevice" not in row[3] for row in want)
    for mine, theirs in zip(got, want):
        assert mine == theirs
    # every source file's entries and every slot are in the recording
    assert {row[0] for row in want} >= {"mpcgpu_env_step_fresh_dev", "mpcgpu_env_step_imgs_fresh_dev", "mpcgpu_collect_rays_dev",
                                       "mpcgpu_per_sample_dev", "mpcgpu_plan_paths_dev", "mpcgpu_map_record_dev",
                                       "mpcgpu_dqn_apply_dev", "mpcgpu_dqn_train_per_dev"}
    assert {slot for _, _, slot, _ in rc.cases(lib)} == set(rc.SLOTS)


def test_entries_say_the_same_words_for_the_same_params():
    """One sentence per params struct, whichever entry and slot says it."""
    rows = rc.load()
    for prefix, sentence in (("params P65", "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
                             ("params capacity0", "invalid mpcgpu_per_params (capacity 1..2^30, update_max_freq >= 1, alpha, epsilon >= 0, "
                                                  "0 <= beta < inf, initial_priority > 0)"),
                             ("per capacity0", "invalid mpcgpu_per_params (capacity 1..2^30, update_max_freq >= 1, alpha, epsilon >= 0, "
                                               "0 <= beta < inf, initial_priority > 0)"),
                             ("params lr0", "invalid mpcgpu_dqn_params (lr, max_grad_norm, eps > 0, 0 <= beta < 1, double_q 0 / 1)"),
                             ("dqn lr0", "invalid mpcgpu_dqn_params (lr, max_grad_norm, eps > 0, 0 <= beta < 1, double_q 0 / 1)")):
        said = [row for row in rows if row[1] == prefix]
        assert said and all(row[3] == sentence for row in said), prefix
    assert len({row[0] for row in rows if row[1] == "params P65"}) == 9      # rays, images, collection and the map record


def test_a_refusal_leaves_every_other_slot_alone(lib):
    """Each ``*_last_error`` export has a slot of its own.  Every slot is given words no other slot holds (the per slot has
    one sentence to say without a device, so the others are chosen around it); then, for every ordered pair of slots, a refusal
    through an entry of the one leaves the other as it was.

    The pair (dqn_per, dqn) fails on the revision the fixture was recorded on: there ``mpcgpu_dqn_train_per_dev`` wrote its
    refusal through the dqn slot and swapped the two strings, so ``mpcgpu_dqn_last_error()`` returned the previous text of the
    dqn_per slot.  It is the one assertion here that revision does not meet."""
    recorded = {(entry, case): words for entry, case, _, words in rc.load()}
    chosen = {}                 # slot -> (call, words), the words of the seven all different
    for entry, case, slot, call in sorted(rc.cases(lib), key=lambda c: c[2] != "per"):
        words = recorded[entry, case]
        if slot not in chosen and words not in [w for _, w in chosen.values()]:
            chosen[slot] = (call, words)
    assert set(chosen) == set(rc.SLOTS)

    def refuse(slot):
        call, words = chosen[slot]
        assert call() == -1 and text(lib, slot) == words

    for slot in rc.SLOTS:
        refuse(slot)
    for mine, theirs in itertools.permutations(rc.SLOTS, 2):
        before = {slot: text(lib, slot) for slot in rc.SLOTS}
        refuse(mine)
        assert text(lib, theirs) == before[theirs], (mine, theirs, before[theirs], text(lib, theirs))
        assert all(text(lib, slot) == before[slot] for slot in rc.SLOTS if slot != mine), mine
    assert len({text(lib, slot) for slot in rc.SLOTS}) == len(rc.SLOTS)
