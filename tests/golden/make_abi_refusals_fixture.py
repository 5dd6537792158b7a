#!/usr/bin/env python3
"""Recording of what the side modules' C-ABI entries refuse before their first HIP call: ``abi_refusals.json`` for
``tests/test_abi_refusals_host.py``.

    python tests/golden/make_abi_refusals_fixture.py            # run the cases twice, write the file if the two runs agree
    python tests/golden/make_abi_refusals_fixture.py --check    # run them once and compare with the file, character for character

Needs the built library and no device.  The cases are ``tests/support/abi_refusal_cases.py``; they use the ctypes tables of the
package only, so this file runs unchanged on any revision, and the committed file is the recording of the revision BEFORE the
entries' host plumbing was moved into csrc/abi_host.hpp.  Every case must be refused (return code -1) with words of the
entry's own: a text that names ``hipSetDevice`` means the case got past the checks, and nothing is written.  Only data is
written."""
import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from support import abi_refusal_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=cases.FIXTURE)
    args = ap.parse_args()
    lib = cases.library()
    first = cases.run(lib)
    passed = [row for row in first if row[2] != -1 or not row[3] or "hipSetDevice" in row[3]]
    if passed:
        sys.exit(f"{len(passed)} cases were not refused before the device: {passed[:4]}: nothing written")
    if len({(row[0], row[1]) for row in first}) != len(first):
        sys.exit("two cases of one entry share a name: nothing written")
    if args.check:
        want = cases.load(args.out)
        bad = [(a, b) for a, b in zip(first, want) if a != b]
        print(f"{args.out}: {len(want)} cases recorded, {len(first)} run, {len(bad)} differ {bad[:4]}")
        sys.exit(1 if bad or len(first) != len(want) else 0)
    if cases.run(lib) != first:
        sys.exit("two runs of the cases differ: nothing written")
    with open(args.out, "w") as fh:
        fh.write(cases.dumps(first))
    print(f"{args.out}: {len(first)} cases of {len({row[0] for row in first})} entries, "
          f"{len({row[3] for row in first})} different texts, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
