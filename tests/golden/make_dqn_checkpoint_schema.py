#!/usr/bin/env python3
"""Recording of the DQN checkpoint format: ``dqn_checkpoint_schema.json`` for ``tests/test_dqn_checkpoint_schema.py``.

    python tests/golden/make_dqn_checkpoint_schema.py            # walk every leg's checkpoint and write the file
    python tests/golden/make_dqn_checkpoint_schema.py --check    # walk them and compare with the file, entry for entry

Needs a HIP device and the built library.  The legs and the walk are ``tests/support/dqn_checkpoint_schema.py``: learners
built through ``DqnLearner``'s public arguments only -- so this file runs unchanged on any revision, and the committed file
is the recording of the revision BEFORE the replay buffers and the two trainers' shared host code were merged.  For every
leg it holds the nested keys of ``learner.state_dict()`` in order, with the Python type of numbers and lists and the dtype
and shape of tensors; no tensor values (they depend on the processor, and the resume tests pin them)."""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from support import dqn_checkpoint_schema as schema  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=schema.FIXTURE)
    args = ap.parse_args()
    got = {leg: schema.schema(leg) for leg in schema.LEGS}
    if args.check:
        want = schema.load(args.out)
        bad = {leg: schema.differences(got[leg], want.get(leg, []))[:3] for leg in got}
        bad = {leg: b for leg, b in bad.items() if b}
        print(f"{args.out}: {len(want)} legs, {len(bad)} differ {bad}")
        sys.exit(1 if bad or set(want) != set(got) else 0)
    with open(args.out, "w") as fh:
        fh.write("{\n" + ",\n".join(f' {json.dumps(leg)}: [\n' + ",\n".join(f"  {json.dumps(e)}" for e in walk) + "\n ]"
                                    for leg, walk in got.items()) + "\n}\n")
    print(f"{args.out}: " + ", ".join(f"{leg} {len(walk)} entries" for leg, walk in got.items()))


if __name__ == "__main__":
    main()
