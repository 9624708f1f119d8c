"""Toy surfaces for the S3F tests: a seeded point cloud around the toy backbones of tests/s2f_cases.py with seeded 42-wide features.
``surface(L, ns)`` returns (points float32 [ns, 3], features float32 [ns, 42]) and asserts, in float64 on the float32 coordinates the
library receives, that both k-NN searches are unambiguous: for every point the relative gap between the 16th and 17th squared
distance to the other points, and between consecutive squared distances among its 4 nearest C-alpha atoms (that list is ordered),
exceeds MARGIN.  fp32 rounding of a squared distance is a few 1e-7 relative, so no list can depend on it."""
import functools

import numpy as np

import s2f_cases
import s3f_ref

MARGIN = 1e-4
FEAT = 42


def draw(pos, ns, rng):
    """ns points 3 .. 7 A from randomly chosen C-alpha atoms, in random directions."""
    pos = np.asarray(pos, dtype=np.float64)
    centre = pos[rng.integers(0, len(pos), ns)]
    u = rng.standard_normal((ns, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (centre + u * rng.uniform(3.0, 7.0, (ns, 1))).astype(np.float32)


def margins(pos, pts):
    return (s3f_ref.knn_margin(pts, pts, s3f_ref.K_SURF, skip_self=True), s3f_ref.knn_margin(pts, pos, s3f_ref.K_RES, ordered=True))


def make(pos, ns, seed):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        pts = draw(pos, ns, rng)
        if min(margins(pos, pts)) > MARGIN:
            break
    feat = rng.standard_normal((ns, FEAT)).astype(np.float32)
    assert min(margins(pos, pts)) > MARGIN, "an ambiguous k-NN list"
    return pts, feat


@functools.lru_cache(maxsize=None)
def surface(L, ns, seed=0):
    pts, feat = make(s2f_cases.toy(L)[0], ns, 100000 * seed + 1000 * L + ns)
    pts.setflags(write=False)
    feat.setflags(write=False)
    return pts, feat
