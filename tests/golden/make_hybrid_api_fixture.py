#!/usr/bin/env python3
"""Recording of the hybrid decision loops' public API: ``hybrid_api_trace.npz`` for ``tests/test_gpu_hybrid_api_golden.py``.

    python tests/golden/make_hybrid_api_fixture.py            # run the session twice, write the file if the two runs agree
    python tests/golden/make_hybrid_api_fixture.py --check    # run it once and compare with the file, bit for bit

Needs a HIP device and the built library.  The session is ``tests/support/hybrid_api_scenario.py``: ``BatchedHybrid`` in modes
0, 1, 2 and ``DeviceHybrid`` in modes 1, 2 through ticks, a mid-episode ``reset()``, ticks again and a recorded ``run`` -- on the
public API only, so this file runs unchanged on any revision, and the committed file is the recording of the revision BEFORE the
two loops were given one base class.  The solve kernels use no atomics and the session draws no random numbers after its seeded
scenes: two runs give the same bits, and the script refuses to write if they do not.  What a recording has to contain
(``scenario.check_not_vacuous``) is asserted before anything is written.  Only data is written."""
import argparse
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from support import hybrid_api_scenario as scenario  # noqa: E402

MAX_BYTES = 280_000          # below the largest committed fixture (costgrad_N20.npz, about 290 KB)


def session():
    out = {}
    for leg in scenario.LEGS:
        out.update(scenario.run_leg(leg))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=scenario.FIXTURE)
    args = ap.parse_args()
    first = session()
    if args.check:
        want = scenario.load(args.out)
        bad = scenario.differences(first, want)
        print(f"{args.out}: {len(want)} arrays, {len(bad)} differ {bad[:8]}")
        sys.exit(1 if bad else 0)
    scenario.check_not_vacuous(first)
    second = session()
    bad = scenario.differences(second, first)
    if bad:
        for key in bad:                                   # where a stacked field parts: the first call that differs
            a, b = first.get(key), second.get(key)
            if a is not None and b is not None and a.shape == b.shape and a.ndim:
                rows = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
                print(f"    {key}: {len(rows)} of {len(a)} rows differ, first {rows[:1].tolist()}")
        sys.exit(f"two runs of the session differ in {bad[:8]}: nothing written")
    np.savez_compressed(args.out, **first)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {len(first)} arrays, {sum(a.nbytes for a in first.values())} bytes raw, {size} in the file")
    for leg in ("host2", "dev2"):
        on = first[f"{leg}.tick.switch_on"]
        print(f"    {leg}: robot-ticks on the proposal {int(on.sum())} of {on.size}; run: steps {first[leg + '.run.steps'].tolist()}, "
              f"success {first[leg + '.run.success'].tolist()}")
    if size > MAX_BYTES:
        os.remove(args.out)
        sys.exit(f"the recording does not fit {MAX_BYTES} bytes: nothing written")


if __name__ == "__main__":
    main()
