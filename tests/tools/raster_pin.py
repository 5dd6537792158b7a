#!/usr/bin/env python3
"""Pin the restated OpenCV rasteriser of the image observation against REAL OpenCV -- on a machine that has cv2.

Why this file exists.  The reference draws its image observation with ``cv2.fillPoly`` (LINE_8, shift 0) and halves it with
``cv2.resize`` (INTER_LINEAR; src/pkg_dqn/environment/components/ext_obsv_image.py:63-74, opencv-python 4.6.0.66 in the
reference's requirements).  OpenCV is not a dependency of this project, so ``tests/support/image_obs_numpy.py`` restates the
rule and the HIP kernel follows the restatement: "parity unpinned" (DESIGN.md section 8.1).  This script is the missing link.
It never runs on the GPU box and imports nothing from the GPU package.

  step 1 (a machine WITH cv2):
      python tests/tools/raster_pin.py record [--out raster_pin.npz] [--n 400] [--seed 0]
    draws seeded random integer polygons -- convex and concave, with horizontal edges, far outside the image, with vertices
    that truncate to negative coordinates (ext_obsv_image.py's np.int32 of values in (-1, 0) gives 0, of (-2, -1) gives -1)
    -- on 2W x 2H uint8 images with fillPoly (boundary 255 first, then the obstacles 0, as the reference does) and resize, and
    writes polygons, image sizes and both the full-size and the resized images.

  step 2 (any machine with this repository; no cv2, no GPU):
      python tests/tools/raster_pin.py compare raster_pin.npz
    runs the restatement on every recorded case and prints the number of cases that match, and for the first mismatch the
    case, the polygon and the first differing pixel (row, column, OpenCV value, restated value) of the full-size image.
    DESIGN.md section 8.1 names the two points where OpenCV releases differ (the rounding of a fill span's left end; a half-pixel
    start of unclipped edges): a mismatch there says which one 4.6 does.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def random_cases(n: int, seed: int):
    """[(width, height, [polygon int32 [k, 2], ...])]: the first polygon is the 'boundary' (255), the others 'obstacles' (0)."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        W, H = int(rng.integers(8, 97)), int(rng.integers(8, 97))
        W2, H2 = 2 * W, 2 * H
        polys = []
        kind = i % 5
        # boundary: a large (possibly concave) ring around the image or partly outside it
        c = rng.uniform([-0.2 * W2, -0.2 * H2], [1.2 * W2, 1.2 * H2])
        k = int(rng.integers(3, 12))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.3, 1.5, k) * max(W2, H2)
        polys.append(np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], 1))
        for _ in range(int(rng.integers(1, 6))):
            k = int(rng.integers(3, 10))
            c = rng.uniform([-10, -10], [W2 + 10, H2 + 10])
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = rng.uniform(0.5, 1.0, k) * rng.uniform(2, 30) * (rng.uniform(0.2, 1.0, k) if kind == 1 else 1.0)  # concave
            p = np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], 1)
            if kind == 2:      # horizontal edges
                p[1::2, 1] = p[0::2, 1][:len(p[1::2])]
            if kind == 3:      # far outside
                p = p + rng.choice([-1, 1], 2) * 1e4
            if kind == 4:      # values in (-2, 1) before truncation
                p = p - p.min(0) - rng.uniform(0.1, 1.9, 2)
            polys.append(p)
        cases.append((W, H, [np.trunc(p).astype(np.int32) for p in polys]))
    return cases


def pack(cases):
    sizes = np.array([(W, H, len(polys)) for W, H, polys in cases], dtype=np.int32)
    lens = np.array([len(p) for _, _, polys in cases for p in polys], dtype=np.int32)
    verts = np.concatenate([p for _, _, polys in cases for p in polys]).astype(np.int32)
    return sizes, lens, verts


def unpack(sizes, lens, verts):
    out, vi, li = [], 0, 0
    for W, H, m in sizes:
        polys = []
        for _ in range(m):
            polys.append(verts[vi:vi + lens[li]])
            vi += lens[li]
            li += 1
        out.append((int(W), int(H), polys))
    return out


def record(args) -> None:
    try:
        import cv2
    except ImportError:
        sys.exit("record needs OpenCV (cv2): run it on a machine that has it; `compare` then runs anywhere")
    cases = random_cases(args.n, args.seed)
    full, small = [], []
    for W, H, polys in cases:
        img = np.zeros((2 * H, 2 * W), dtype=np.uint8)
        cv2.fillPoly(img, [polys[0]], 255)
        for p in polys[1:]:
            cv2.fillPoly(img, [p], 0)
        full.append(img.reshape(-1))
        small.append(cv2.resize(img, (W, H)).reshape(-1))
    sizes, lens, verts = pack(cases)
    np.savez_compressed(args.out, sizes=sizes, lens=lens, verts=verts, full=np.concatenate(full),
                        small=np.concatenate(small), cv2_version=np.array(cv2.__version__))
    print(f"wrote {args.out}: {len(cases)} cases, OpenCV {cv2.__version__}")


def compare(args) -> None:
    from support import image_obs_numpy as im
    d = np.load(args.recording)
    cases = unpack(d["sizes"], d["lens"], d["verts"])
    fo = so = 0
    ok = 0
    first = None
    for i, (W, H, polys) in enumerate(cases):
        nf, ns = 4 * W * H, W * H
        want_full = d["full"][fo:fo + nf].reshape(2 * H, 2 * W)
        want_small = d["small"][so:so + ns].reshape(H, W)
        fo += nf
        so += ns
        img = np.zeros((2 * H, 2 * W), dtype=np.uint8)
        im.fill_poly(img, polys[0], 255)
        for p in polys[1:]:
            im.fill_poly(img, p, 0)
        if np.array_equal(img, want_full) and np.array_equal(im.resize_half(img), want_small):
            ok += 1
        elif first is None:
            r, c = np.argwhere(img != want_full)[0] if not np.array_equal(img, want_full) else (-1, -1)
            first = (i, W, H, polys, r, c, want_full[r, c] if r >= 0 else None, img[r, c] if r >= 0 else None)
    print(f"OpenCV {d['cv2_version']}: {ok} of {len(cases)} cases equal (full-size and resized)")
    if first is not None:
        i, W, H, polys, r, c, cv, me = first
        print(f"first mismatch: case {i} ({2 * W} x {2 * H}), pixel row {r} column {c}: OpenCV {cv}, restatement {me}")
        for j, p in enumerate(polys):
            print(f"  polygon {j} ({'boundary 255' if j == 0 else 'obstacle 0'}): {p.tolist()}")
    sys.exit(0 if ok == len(cases) else 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--out", default="raster_pin.npz")
    r.add_argument("--n", type=int, default=400)
    r.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("compare")
    c.add_argument("recording")
    args = ap.parse_args()
    record(args) if args.cmd == "record" else compare(args)


if __name__ == "__main__":
    main()
