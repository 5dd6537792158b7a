#!/usr/bin/env python3
"""Recording of ``DqnLearner.learn`` in every combination of its strategies: ``dqn_learner_trace.npz`` for
``tests/test_gpu_dqn_learner_golden.py``.

    python tests/golden/make_dqn_learner_fixture.py            # run the session twice, write the legs on which the two runs agree
    python tests/golden/make_dqn_learner_fixture.py --check    # run it once and compare with the file, bit for bit

Needs a HIP device and the built library.  The session is ``tests/support/dqn_learner_scenario.py``: nine legs (eager, graph, PER,
the fused one-launch round, fused around the tree, PER inside the launch, collection inside the launch with the fused and with the
plain trainer, the image environment), each run to a checkpoint in mid-schedule and continued in a fresh learner.  It uses the
learner's public surface, so this file runs unchanged on any revision, and the committed file is the recording of the revision
BEFORE ``learn`` was written as one loop over two bound strategies.  A leg whose two runs differ is left out of the file and named
on the output; the legs of ``scenario.OWN_KERNEL_LEGS`` run only this project's kernels and have no reason to differ, so the
script ends with an error if one of them does (after writing the others).  What a recording has to contain
(``scenario.check_not_vacuous``) is asserted before anything is written.  Only data is written."""
import argparse
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from support import dqn_learner_scenario as scenario  # noqa: E402

MAX_BYTES = 280_000          # below the largest committed fixture (costgrad_N20.npz, about 290 KB)


def session(legs):
    out = {}
    for leg in legs:
        out.update(scenario.run_leg(leg))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=scenario.FIXTURE)
    args = ap.parse_args()
    if args.check:
        want = scenario.load(args.out)
        bad = scenario.differences(session(scenario.legs_of(want)), want)
        print(f"{args.out}: {len(want)} arrays, legs {scenario.legs_of(want)}, {len(bad)} differ {bad[:8]}")
        sys.exit(1 if bad else 0)
    first = session(scenario.LEGS)
    scenario.check_not_vacuous(first)
    bad = scenario.differences(session(scenario.LEGS), first)
    cut = sorted({key.split(".")[0] for key in bad})
    for leg in cut:
        print(f"    {leg}: two runs differ in {[k for k in bad if k.startswith(leg + '.')][:8]}: left out")
    kept = {k: v for k, v in first.items() if k.split(".")[0] not in cut}
    np.savez_compressed(args.out, **kept)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {len(kept)} arrays, legs {scenario.legs_of(kept)}, {sum(a.nbytes for a in kept.values())} bytes raw, {size} in the file")
    for leg in scenario.legs_of(kept):
        print(f"    {leg}: result {dict(zip(scenario.RESULT_KEYS, kept[leg + '.result.end'].tolist()))}, "
              f"terminal rows {int(kept[leg + '.trace.terminated_rows'][-1])}")
    if size > MAX_BYTES:
        os.remove(args.out)
        sys.exit(f"the recording does not fit {MAX_BYTES} bytes: nothing written")
    if set(cut) & set(scenario.OWN_KERNEL_LEGS):
        sys.exit(f"not reproducible although only this project's kernels run: {sorted(set(cut) & set(scenario.OWN_KERNEL_LEGS))}")


if __name__ == "__main__":
    main()
