"""Fixture of the convex-hull facet rule: Gaussian point sets with the facets and the volume scipy's qhull reports for them.

    python tests/golden/make_hull_facets_golden.py            # rewrites tests/golden/hull_facets_ref.npz

Needs scipy; nothing else. For every (V, n) shape and seed: `<name>/points` float64 [V, n] (standard normal, drawn as float32
- what the device lift is given), `<name>/facets` int64 [F, n] (ConvexHull(points).simplices, every row sorted, the rows in
lexicographic order) and `<name>/volume` float64 (ConvexHull(points).volume). tests/test_hull_lift_cpu.py holds
csmpn.data.complexes.hull_facets against it, and checks on the stored points that no candidate's side value is within 1e-9 of
zero (the sets are in general position, so the facet set does not depend on the implementation)."""
import os

import numpy as np
from scipy.spatial import ConvexHull

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "hull_facets_ref.npz")
SHAPES = [(8, 5), (8, 4), (8, 3), (7, 2), (6, 5), (16, 5), (12, 3), (9, 4)]
SEEDS = [0, 1, 2, 3]


def case_name(V, n, seed):
    return f"v{V}_n{n}_s{seed}"


def main():
    out = {}
    for V, n in SHAPES:
        for seed in SEEDS:
            pts = np.random.default_rng(1000 * V + 100 * n + seed).standard_normal((V, n)).astype(np.float32).astype(np.float64)
            hull = ConvexHull(pts)
            facets = np.array(sorted(map(tuple, np.sort(hull.simplices, axis=1).tolist())), dtype=np.int64)
            name = case_name(V, n, seed)
            out[f"{name}/points"], out[f"{name}/facets"], out[f"{name}/volume"] = pts, facets, np.float64(hull.volume)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {FIXTURE}: {len(SHAPES) * len(SEEDS)} point sets, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
