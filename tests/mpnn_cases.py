"""TEST INFRASTRUCTURE ONLY -- synthetic backbones for the ProteinMPNN tests: a 3.8 A random walk of CA atoms with N, C and O placed
around each, optional second chain, masked residues (one missing atom: its coordinates 0, mask 0) and an 'X' in the sequence."""
import numpy as np

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"


def backbone(L, seed):
    rng = np.random.default_rng(seed)
    ca = np.zeros((L, 3))
    d = rng.normal(size=3)
    for i in range(1, L):
        d = 0.6 * d / np.linalg.norm(d) + 0.8 * rng.normal(size=3) / np.sqrt(3.0)     # a persistent walk: compact but not collapsed
        ca[i] = ca[i - 1] + 3.8 * d / np.linalg.norm(d)
    X = np.zeros((L, 4, 3))
    X[:, 1] = ca
    for a, r in ((0, 1.46), (2, 1.52), (3, 2.4)):
        v = rng.normal(size=(L, 3))
        X[:, a] = ca + r * v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.round(X, 3)                    # PDB precision


def make_case(L, seed, n_masked=0, two_chains=False, with_x=False):
    rng = np.random.default_rng(seed + 1000)
    X = backbone(L, seed)
    mask = np.ones(L, dtype=np.float32)
    if n_masked:
        for i in rng.choice(np.arange(2, L - 2), size=n_masked, replace=False):
            X[i, rng.integers(0, 4)] = 0.0
            mask[i] = 0.0
    split = L // 2 + 3 if two_chains else L
    chain = np.where(np.arange(L) < split, 1, 2).astype(np.int32)
    ridx = (np.arange(L) + 100 * (chain - 1)).astype(np.int32)
    S = rng.integers(0, 20, size=L).astype(np.int32)
    if with_x:
        S[L // 3] = 20
    return dict(X=X.astype(np.float32), mask=mask, residue_idx=ridx, chain_encoding=chain, S=S, L=L)


def neighbour_gap_ok(case, num_edges=48, gap=1e-3):
    """The GPU tests' input condition, in float64: at every unmasked residue the K-th and (K+1)-th adjusted CA distances differ by
    more than ``gap`` A, and more than K + 1 residues are unmasked whenever L > K."""
    X, mask = case["X"].astype(np.float64), case["mask"].astype(np.float64)
    L = len(mask)
    K = min(num_edges, L)
    if L <= K:
        return True
    if mask.sum() <= K + 1:
        return False
    m2 = mask[:, None] * mask[None, :]
    D = m2 * np.sqrt(((X[None, :, 1] - X[:, None, 1]) ** 2).sum(-1) + 1e-6)
    D = np.sort(D + (1 - m2) * D.max(-1, keepdims=True), axis=-1)
    return bool(((D[:, K] - D[:, K - 1])[mask > 0] > gap).all())


def mutants(case, B, seed):
    """S [B, L] (row 0 the case's sequence, the others one to three substitutions) and randn [B, L]"""
    rng = np.random.default_rng(seed)
    L = case["L"]
    S = np.tile(case["S"], (B, 1))
    for b in range(1, B):
        pos = rng.choice(L, size=1 + b % 3, replace=False)
        S[b, pos] = (S[b, pos] + rng.integers(1, 20, size=len(pos))) % 20
    return S.astype(np.uint8), rng.standard_normal((B, L)).astype(np.float32)


# (L, backbone seed, masked residues, two chains, an X in S): K = L = 24 is no multiple of 16; 70 has two chains; 131 leaves a partial
# tile of nodes (131 = 32 x 4 + 3).  The seeds satisfy neighbour_gap_ok (asserted by the tests that use them).
SHAPES = {24: (24, 1, 2, False, False), 70: (70, 2, 3, True, False), 131: (131, 3, 5, False, True)}
NUM_EDGES = 48


def shape_case(L):
    return make_case(*SHAPES[L])
