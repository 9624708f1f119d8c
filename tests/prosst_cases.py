"""Toy backbones for the ProSST tests: C-alpha from ``s2f_cases.toy(L)`` (a short helix next to a serpentine lattice at C-alpha spacing
and one residue far from everything), N, C and O at seeded offsets around it, every coordinate rounded to three decimals as a PDB file
holds it.  ``toy(L)`` returns X float32 [L, 4, 3] (N, CA, C, O) and asserts its conditions in float64 on those float32 values:
  * no pair distance within 1e-3 A of the 10 A radius (the edge set cannot depend on rounding);
  * no anchor whose 40th and 41st nearest candidates are closer than 1e-4 A in distance (no tie decides membership);
  * exactly one isolated node;
  * for L = 131: an anchor with more than 40 candidates (the cut to 40), one with 31 .. 40 (more than 30: kept as they are, all below
    the cut) and in-degrees above 32 (more than one 32-row tile of edges at a node).
The lattice already has what can go wrong; for L = 9 several anchors share their node set (2 and 7, 3 and 6, 4 and 5).  The seeded weights, the float64
/ float32 references and the codebooks of the GPU tests are here too, so each is computed once."""
import functools

import numpy as np
import torch

import prosst_ref
import s2f_cases

RADIUS = 10.0
SIZES = (9, 37, 131)
WEIGHT_SEED = 11
TRACE_SUB = {9: 2, 37: 20, 131: 77}          # the subgraph whose node state the tests compare


def _backbone(ca, rng):
    L = len(ca)
    X = np.empty((L, 4, 3), np.float64)
    X[:, 1] = ca
    for atom, length in ((0, 1.46), (2, 1.52)):
        u = rng.standard_normal((L, 3))
        X[:, atom] = ca + length * u / np.linalg.norm(u, axis=1, keepdims=True)
    u = rng.standard_normal((L, 3))
    X[:, 3] = X[:, 2] + 1.23 * u / np.linalg.norm(u, axis=1, keepdims=True)
    return np.round(X, 3).astype(np.float32)


def stats(X):
    d = prosst_ref.distances(X)
    cand = (d < RADIUS).sum(1)                                   # self included
    srt = np.sort(d, axis=1)
    gap = np.array([srt[i, 40] - srt[i, 39] for i in range(len(d)) if cand[i] > 40]) if len(d) > 40 else np.zeros(0)
    edges = prosst_ref.global_edges(d)
    subs = [prosst_ref.subgraph_nodes(d, i) for i in range(len(d))]
    indeg = max((int(np.bincount(prosst_ref.subgraph_edges(d, edges, n)[0][1], minlength=1).max()) if len(n) > 1 else 0) for n in subs)
    return dict(d=d, cand=cand, gap=gap, edges=edges, subs=subs, indeg=indeg, e_sub=sum(len(prosst_ref.subgraph_edges(d, edges, n)[1]) for n in subs))


def check_conditions(X):
    st = stats(X)
    d, cand = st["d"], st["cand"]
    assert np.abs(d - RADIUS).min() > 1e-3, "a pair distance within 1e-3 A of the radius"
    assert not len(st["gap"]) or st["gap"].min() >= 1e-4, "a tie decides the membership of a subgraph"
    assert (cand == 1).sum() == 1, "not exactly one isolated node"
    if len(X) == 131:
        assert (cand > 40).any() and ((cand > 30) & (cand <= 40)).any(), "no anchor above the cut / between the threshold and the cut"
        assert st["indeg"] > 32, "no node copy with more than 32 incoming edges"
    if len(X) == 9:
        sets = [tuple(s) for s in st["subs"]]
        assert len(set(sets)) < len(sets) - 1, "L = 9: no anchors with equal node sets"
    return st


@functools.lru_cache(maxsize=None)
def toy(L):
    for seed in range(50):
        ca = np.asarray(s2f_cases.toy(L, seed)[0], dtype=np.float64)
        X = _backbone(ca, np.random.default_rng(4000 * L + seed))
        d = prosst_ref.distances(X)
        if np.abs(d - RADIUS).min() > 1e-3:
            break
    check_conditions(X)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def state_dict():
    from proteingym_amd import prosst
    sd = prosst.random_state_dict(WEIGHT_SEED)
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def reference(L):
    """(float64 results, float32 results) of prosst_ref.embed_all with the node state of subgraph TRACE_SUB[L]."""
    return tuple(prosst_ref.embed_all(state_dict(), toy(L), dt, trace_sub=TRACE_SUB[L]) for dt in (torch.float64, torch.float32))


def delta(L):
    """The embedding bound of a case as an L2 norm: 10 x the largest row distance of fp32 torch from float64."""
    r64, r32 = reference(L)
    return 10.0 * float(np.linalg.norm(r32["emb"].astype(np.float64) - r64["emb"], axis=1).max())


def exempt(L, centres):
    """Residues whose float64 margin d2(second) - d2(best) is at most 2 |delta| |c_best - c_second|: an fp32 embedding within the bound may
    take the other centre.  Returns (mask [L], float64 tokens)."""
    tok, d2 = prosst_ref.assign(reference(L)[0]["emb"], centres)
    order = np.argsort(d2, axis=1, kind="stable")
    best, second = order[:, 0], order[:, 1]
    rows = np.arange(len(tok))
    margin = d2[rows, second] - d2[rows, best]
    sep = np.linalg.norm(np.asarray(centres, np.float64)[best] - np.asarray(centres, np.float64)[second], axis=1)
    return margin <= 2.0 * delta(L) * sep, tok


@functools.lru_cache(maxsize=None)
def codebook(K):
    """Centres float32 [K, 256] fitted by seeded k-means on the float64 embeddings of the toy structures themselves, so that tokens differ
    between residues (random centres give one token for everything: seeded weights put all embeddings close together).  Asserts what the
    token tests rely on: at most 2 % of a case's residues are exempt, and the tokens of L = 131 are not all equal."""
    pts = np.concatenate([reference(L)[0]["emb"] for L in SIZES])
    c = prosst_ref.kmeans(pts, K, seed=K).astype(np.float32)
    for L in SIZES:
        ex, tok = exempt(L, c)
        assert ex.sum() <= 0.02 * L, f"K {K} L {L}: {int(ex.sum())} residues within the margin"
    assert len(set(exempt(131, c)[1].tolist())) > 1
    c.setflags(write=False)
    return c


def pdb_text(X, seq=None):
    """The backbone as PDB ATOM records (one chain), three decimals: what read_backbone reads back bit for bit."""
    names = ("N", "CA", "C", "O")
    three = ["ALA", "GLY", "SER", "LEU", "LYS", "GLU", "VAL", "THR"]
    lines = []
    n = 1
    for i, res in enumerate(X):
        rn = three[i % len(three)] if seq is None else seq[i]
        for a, p in zip(names, res):
            lines.append("ATOM  %5d  %-3s %3s A%4d    %8.3f%8.3f%8.3f  1.00 80.00           %s" % (n, a, rn, i + 1, p[0], p[1], p[2], a[0]))
            n += 1
    return "\n".join(lines + ["TER", "END", ""])
