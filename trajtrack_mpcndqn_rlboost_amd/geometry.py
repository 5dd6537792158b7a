"""Half-space (H-) representation of convex polygons: the static-obstacle block of the parameter vector.

Reference: ``src/util/utils_geo.py:33-59`` -- every facet of the convex hull is written as ``a . (x - c) = 1`` with
``c`` the mean of the hull vertices, i.e. the polygon is ``{x : b - a0 x - a1 y > 0}`` with ``b = a . c + 1``
(``src/mpc_traj_tracker/mpc/mpc_generator.py:46-54`` consumes exactly that).  Here the facets come from Qhull's
own facet equations ``n . x + d <= 0`` (same facet order as ``hull.simplices``, which the reference loops over):
with ``s = -(d + n . c)`` the reference's normalisation is ``a = n / s`` and ``b = -d / s``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
from scipy.spatial import ConvexHull


def polygon_halfspace_representation(polygon_points: np.ndarray) -> Tuple[List[float], List[float], List[float]]:
    pts = np.asarray(polygon_points, dtype=float)
    hull = ConvexHull(pts)
    centre = pts[hull.vertices].mean(axis=0)
    normals, offsets = hull.equations[:, :2], hull.equations[:, 2]
    scale = -(offsets + normals @ centre)          # distance-like factor of every facet from the centre (> 0)
    keep = np.abs(scale) > 1e-14                    # a facet through the centre has no such representation
    a = normals[keep] / scale[keep, None]
    b = -offsets[keep] / scale[keep]
    return b.tolist(), a[:, 0].tolist(), a[:, 1].tolist()


NEUTRAL_HALFPLANE = (1.0, 0.0, 0.0)   # (b, a0, a1): max(0, 1 - 0 x - 0 y) = 1 everywhere


def static_obstacle_params(obstacle_list: Sequence[Sequence[Sequence[float]]], n_slots: int,
                           n_per_obstacle: int = 12, pad_edges: bool = False) -> List[float]:
    """Padded static-obstacle block (``src/interface_mpc.py:23,60-63``).  Unlike the reference, an obstacle whose
    hull does not have exactly ``n_per_obstacle / 3`` edges is an error instead of silently changing the length of
    the block.

    ``pad_edges``: a hull with FEWER edges fills its slot with neutral half-planes ``(b, a0, a1) = (1, 0, 0)``.  Such a
    row has the value 1 at every point: it multiplies the product of squared hinges
    (``mpc_generator.py:46-54``) by exactly 1 and adds exactly zero to its gradient, so the padded polygon IS the
    smaller one -- a triangle in a solver built for four edges, quads and hexagons side by side in one built for six.
    A hull with more edges than the slot has is an error in either mode."""
    if len(obstacle_list) > n_slots:
        raise ValueError(f"{len(obstacle_list)} static obstacles but only {n_slots} slots")
    block = [0.0] * (n_slots * n_per_obstacle)
    for i, poly in enumerate(obstacle_list):
        b, a0, a1 = polygon_halfspace_representation(np.array(poly, dtype=float))
        ne = n_per_obstacle // 3
        if len(b) != ne and not (pad_edges and len(b) < ne):
            raise ValueError(f"static obstacle {i} has {len(b)} hull edges; the solver is built for {ne}"
                             + (" or fewer" if pad_edges else ""))
        fill = ne - len(b)
        b, a0, a1 = b + [NEUTRAL_HALFPLANE[0]] * fill, a0 + [NEUTRAL_HALFPLANE[1]] * fill, a1 + [NEUTRAL_HALFPLANE[2]] * fill
        block[i * n_per_obstacle:(i + 1) * n_per_obstacle] = b + a0 + a1
    return block
