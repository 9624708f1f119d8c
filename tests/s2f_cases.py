"""Toy structures for the S2F tests: a short perturbed helix next to a perturbed three-strand-wide stack of sheets (a serpentine
lattice at C-alpha spacing), and one residue far from everything.  ``toy(L, seed)`` returns (pos float32 [L, 3], plddt float32 [L])
and asserts its input conditions in float64 on the float32 coordinates the library receives:
  * no pair distance within 1e-3 A of the 10 A radius (the edge set cannot depend on rounding);
  * at least one node without a neighbour;
  * for L >= 37, at least one node with more than 33 candidates (self included), so the cap and its index order are exercised -- a
    9-residue toy cannot have one;
  * pLDDT on both sides of 70.
The seeded weights and inputs of the GPU tests are here too, so the float64 reference of a case is computed once."""
import functools

import numpy as np

RADIUS, CAP = 10.0, 32


def _draw(L, rng):
    nh = min(max(L // 16, 2), 12)
    pts = []
    for k in range(nh):
        a = np.deg2rad(100.0 * k)
        pts.append((-7.5 + 2.3 * np.cos(a), 2.3 * np.sin(a), 1.5 * k))
    for t in range(L - nh - 1):
        z, r = divmod(t, 9)
        y, x = divmod(r, 3)
        if y % 2:
            x = 2 - x
        if z % 2:
            y, x = 2 - y, 2 - x
        pts.append((3.8 * x, 3.8 * y, 3.8 * z))
    pos = np.array(pts, dtype=np.float64) + 0.15 * rng.standard_normal((len(pts), 3))
    return np.concatenate([pos, [[60.0, 60.0, 60.0]]]).astype(np.float32)


def candidates(pos):
    p = np.asarray(pos, dtype=np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    return d, (d * d < RADIUS * RADIUS).sum(1)


def check_conditions(pos, plddt):
    d, cand = candidates(pos)
    assert np.abs(d - RADIUS).min() > 1e-3, "a pair distance within 1e-3 A of the radius"
    assert (cand == 1).any(), "no isolated node"
    if len(pos) >= 37:
        assert (cand > CAP + 1).any(), "no node above the neighbour cap"
    assert (plddt < 70).any() and (plddt >= 70).any(), "pLDDT on one side of 70 only"


@functools.lru_cache(maxsize=None)
def toy(L, seed=0):
    rng = np.random.default_rng(1000 * L + seed)
    for _ in range(100):
        pos = _draw(L, rng)
        if np.abs(candidates(pos)[0] - RADIUS).min() > 1e-3:
            break
    plddt = (40.0 + 55.0 * rng.random(L)).astype(np.float32)
    plddt[0], plddt[1] = 50.0, 90.0
    check_conditions(pos, plddt)
    pos.setflags(write=False)
    plddt.setflags(write=False)
    return pos, plddt


def inputs(L, B, D, seed=0):
    """Seeded node features [B, L, D] (LayerNorm-like rows) and sequence logits [B, L, 20]."""
    rng = np.random.default_rng(77 * L + B + seed)
    return rng.standard_normal((B, L, D)).astype(np.float32), (2.0 * rng.standard_normal((B, L, 20))).astype(np.float32)
