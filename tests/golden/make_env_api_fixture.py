#!/usr/bin/env python3
"""Recording of the batched environments' public API: ``env_api_trace.npz`` for ``tests/test_gpu_env_api_golden.py``.

    python tests/golden/make_env_api_fixture.py            # run the session twice, write the file if the two runs agree
    python tests/golden/make_env_api_fixture.py --check    # run it once and compare with the file, bit for bit

Needs a HIP device and the built library.  The session is ``tests/support/env_api_scenario.py``: both environment classes
through plain calls, auto-reset, spares and the device map stream, on the public API only -- so this file runs unchanged
on any revision, and the committed file is the recording of the revision BEFORE the two classes' host logic was merged.
The kernels use one workgroup per row and no atomics and the map stream is counter-based: two runs give the same bits,
and the script refuses to write if they do not.  The conditions a recording has to meet (every row ends two episodes in
the auto-reset leg, rows 1, 5, 6 load their spares, half of the rows load a streamed map) are asserted by the session
itself.  Only data is written.  If the images push the file past ``MAX_BYTES``, the images of the legs after the first are
kept for every third call only (the test thins its replay in the same way); no other array is ever dropped."""
import argparse
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from support import env_api_scenario as scenario  # noqa: E402

MAX_BYTES = 280_000          # below the largest committed fixture (costgrad_N20.npz, about 290 KB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=scenario.FIXTURE)
    args = ap.parse_args()
    first = scenario.run()
    if args.check:
        want = scenario.load(args.out)
        bad = scenario.differences(scenario.stored(first, want), want)
        print(f"{args.out}: {len(want)} arrays, {len(bad)} differ {bad[:8]}")
        sys.exit(1 if bad else 0)
    bad = scenario.differences(scenario.run(), first)
    if bad:
        sys.exit(f"two runs of the session differ in {bad[:8]}: nothing written")
    for thin in (False, True):
        data = scenario.stored(first, thin=thin)
        np.savez_compressed(args.out, **data)
        size = os.path.getsize(args.out)
        print(f"{args.out}: {len(data)} arrays, {sum(a.nbytes for a in data.values())} bytes raw, {size} in the file"
              + (" (images of legs 2-4: every third call)" if thin else ""))
        if size <= MAX_BYTES:
            return
        with zipfile.ZipFile(args.out) as zf:
            for info in sorted(zf.infolist(), key=lambda i: -i.compress_size)[:10]:
                print(f"    {info.filename}: {info.compress_size} of {info.file_size} bytes")
    os.remove(args.out)
    sys.exit(f"the recording does not fit {MAX_BYTES} bytes even with thinned images: nothing written")


if __name__ == "__main__":
    main()
