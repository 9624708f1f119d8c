"""S3F on the MI355X against the float64 torch restatement (tests/s3f_ref.py over tests/s2f_ref.py) on the toy backbones of
tests/s2f_cases.py with the seeded surfaces of tests/s3f_cases.py and the fixtures of tests/golden/S3F_toy: the two k-NN searches and
surf_W_e, both GNNs alone (pgmi_s3f_gvp_forward), the loader-batch pooling, the whole path over a small seeded ESM2
(pgmi_s3f_set_logprobs), the bits of a copy alone / in a batch / under a row cap, the CLI on the toy assays, and the refusals.

Bounds: the surface node state after the last layer and the per-copy pooled sum within 10 x the deviation of fp32 torch from float64
on the same tensor (S2F's rule; the bound is computed here); log-probabilities and scores within the flat 1e-4 of DESIGN.md section 3.
Surface shapes: 17 points is the minimum (every point neighbours all others); 33 is odd, so the message kernel's last tile holds one
point; 250 points on L = 37 is many tiles and more than three 64-row blocks of the column sum; "cut" is the fixture whose structure is
longer than its window; L = 9 with 40 points is a residue graph below one tile."""
import functools
import os
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

import s2f_cases
import s2f_ref
import s3f_cases
import s3f_ref
from proteingym_amd import _lib, s2f, s3f, synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-4
D_GNN = 128
ESM_CFG = dict(S.ESM2_650M, layers=2, embed_dim=128, heads=2, ffn_dim=256)
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "S3F_toy")
CASES = [(37, 17), (37, 33), (37, 250), "cut", (9, 40)]


@functools.lru_cache(maxsize=None)
def state_dict():
    sd = s3f.random_state_dict(5, ESM_CFG, esm_blob=S.random_weights(ESM_CFG, seed=3))
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def fixture_assay(n):
    """Row n of the fixture's reference file: (row, pos, plddt, structure range, the surface triple)."""
    ref = pd.read_csv(os.path.join(TOY, "reference.csv"))
    row = ref.iloc[n]
    pos, plddt, s_start, s_end = s2f.load_structure(TOY, row["pdb_file"], row["pdb_range"], row["DMS_id"])
    return row, pos, plddt, (s_start, s_end), s3f.load_surface(TOY, row["pdb_file"])


@functools.lru_cache(maxsize=None)
def structure(case):
    """(pos, plddt, surface points, surface features) of a case."""
    if case == "cut":
        row, pos, plddt, (s_start, s_end), surface = fixture_assay(1)
        L = len(row["target_seq"])
        assert s_end - s_start > L                                    # the structure is longer than the window
        pts, feat = s3f.cut_surface(*surface, s_start, s_end, 0, L)
        assert len(pts) < len(surface[0])
        return s2f.cut_structure(pos, plddt, s_start, s_end, 0, L) + (pts, feat)
    L, ns = case
    return s2f_cases.toy(L) + s3f_cases.surface(L, ns)


def inputs(case, B):
    L = len(structure(case)[0])
    return s2f_cases.inputs(L, B, D_GNN, seed=len(structure(case)[2]))


@functools.lru_cache(maxsize=None)
def reference(case, B, batch_size):
    """(float64 lp, surf_s, surf_v, pool_sum) and the fp32-torch deviation of each, computed once per case."""
    pos, plddt, pts, feat = structure(case)
    x, q = inputs(case, B)
    r64 = s3f_ref.gvp_forward(state_dict(), pos, plddt, pts, feat, x, q, batch_size, torch.float64)
    r32 = s3f_ref.gvp_forward(state_dict(), pos, plddt, pts, feat, x, q, batch_size, torch.float32)
    return r64, [float(np.abs(a - b).max()) for a, b in zip(r64, r32)]


@pytest.fixture(scope="module")
def gnn(lib):
    m = s3f.S3F(s3f.pack(state_dict(), ESM_CFG)[1], node_in=D_GNN)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model(lib):
    m = s3f.from_state_dict(state_dict(), ESM_CFG)
    yield m
    m.close()
    m.esm.close()


@pytest.fixture
def row_cap(lib):
    def set_(n):
        _lib.check(lib.pgmi_set_option(b"s2f_max_rows", int(n)))
    yield set_
    lib.pgmi_set_option(b"s2f_max_rows", 0)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_knn_lists_and_edge_features(gnn, case):
    pos, plddt, pts, feat = structure(case)
    assert min(s3f_cases.margins(pos, pts)) > s3f_cases.MARGIN
    gnn.set_structure(pos, plddt, pts, feat)
    g = gnn.graph()
    edges = s2f_ref.radius_edges(pos).numpy()
    assert np.array_equal(g["src"], edges[0]) and np.array_equal(g["dst"], edges[1])
    src, res, res_dist = s3f_ref.surface_lists(pos, pts)
    assert np.array_equal(g["surf_src"], src)
    assert np.array_equal(g["surf_res"], res)
    d32 = np.sqrt(((pts[:, None, :] - np.asarray(pos)[res]) ** 2).sum(-1, dtype=np.float32))
    err, dev = np.abs(g["surf_res_dist"] - res_dist).max(), np.abs(d32 - res_dist).max()
    print(f"{case} res_dist: max|err| {err:.3e}; fp32 numpy vs float64 {dev:.3e} (bound {10 * dev:.1e})")
    assert err <= 10 * dev
    out = {}
    for dtype in (torch.float64, torch.float32):
        W = s2f_ref.tensors(state_dict(), dtype)
        out[dtype] = s3f_ref.surface_edge_features(W, torch.as_tensor(np.array(pts)).to(dtype), s3f_ref.surface_edges(src))
    for name, got, ref, f32 in (("e_s", g["surf_e_s"], out[torch.float64][0], out[torch.float32][0]),
                                ("e_v", g["surf_e_v"], out[torch.float64][1][:, 0], out[torch.float32][1][:, 0])):
        err, dev = np.abs(got - ref.numpy()).max(), np.abs(f32.numpy() - ref.numpy()).max()
        print(f"{case} surface {name}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
        assert err <= 10 * dev, name


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gvp_forward_matches_the_restatement(gnn, case, B):
    pos, plddt, pts, feat = structure(case)
    x, q = inputs(case, B)
    (lp64, s64, v64, p64), dev = reference(case, B, 1)
    gnn.set_structure(pos, plddt, pts, feat)
    lp, ss, sv, ps = gnn.gvp_forward(x, q, want_surface=True)
    for name, got, ref, d in (("surf_s", ss, s64, dev[1]), ("surf_v", sv, v64, dev[2]), ("pool_sum", ps, p64, dev[3])):
        err = np.abs(got - ref).max()
        print(f"{case} B {B} {name}: max|err| {err:.3e}; fp32 torch vs float64 {d:.3e} (bound {10 * d:.1e})")
        assert err <= 10 * d, name
    err = np.abs(lp - lp64).max()
    print(f"{case} B {B} log-probabilities: max|err| {err:.3e} (fp32 torch {dev[0]:.3e})")
    assert err <= TOL


@pytest.mark.parametrize("case", [(37, 33), (37, 250)], ids=str)
def test_a_loader_batch_of_two_shares_one_pooled_row(gnn, row_cap, case):
    """batch_size 2 over three copies: groups (0, 1) and the short last one (2)."""
    pos, plddt, pts, feat = structure(case)
    x, q = inputs(case, 3)
    (lp64, _, _, p64), dev = reference(case, 3, 2)
    gnn.set_structure(pos, plddt, pts, feat)
    lp, _, _, ps = gnn.gvp_forward(x, q, pool_off=s3f.pool_groups(3, 2), want_surface=True)
    ns = len(pts)
    pooled = np.stack([(ps[0] + ps[1]) / (2 * ns)] * 2 + [ps[2] / ns])
    want = np.stack([(p64[0] + p64[1]) / (2 * ns)] * 2 + [p64[2] / ns])
    err = np.abs(pooled - want).max()
    print(f"{case} pooled rows of (0, 1) and (2): max|err| {err:.3e} (bound {10 * dev[3] / ns:.1e})")
    assert err <= 10 * dev[3] / ns
    err = np.abs(lp - lp64).max()
    print(f"{case} batch_size 2 log-probabilities: max|err| {err:.3e}")
    assert err <= TOL
    alone = gnn.gvp_forward(x, q)
    assert not np.array_equal(alone[0], lp[0]) and np.array_equal(alone[2], lp[2])      # the pair pools, the short group is a copy alone
    row_cap(1)                                                                          # one copy per chunk: the pair's head waits
    assert np.array_equal(gnn.gvp_forward(x, q, pool_off=s3f.pool_groups(3, 2)), lp)


@pytest.mark.parametrize("case", [(37, 33), (37, 250)], ids=str)
def test_a_copy_has_the_same_bits_alone_in_a_batch_and_under_a_row_cap(gnn, row_cap, case):
    pos, plddt, pts, feat = structure(case)
    x, q = inputs(case, 3)
    gnn.set_structure(pos, plddt, pts, feat)
    batch = gnn.gvp_forward(x, q, want_surface=True)
    alone = gnn.gvp_forward(x[1:2], q[1:2], want_surface=True)
    for a, b in zip(alone, batch):
        assert np.array_equal(a[0], b[1])
    row_cap(1)
    for a, b in zip(gnn.gvp_forward(x, q, want_surface=True), batch):
        assert np.array_equal(a, b)


def toy_sets(L, seed=2):
    """A sequence and site sets (singles, a double, a repeat) in loader order."""
    rng = np.random.default_rng(seed + L)
    seq = "".join(rng.choice(list(s2f.RESIDUE_ORDER), L))
    sets = [(int(p),) for p in sorted(rng.choice(L - 1, 3, replace=False))]
    sets += [tuple(sorted(int(p) for p in rng.choice(L - 1, 2, replace=False))), sets[0]]
    return seq, sets


@functools.lru_cache(maxsize=None)
def reference_tables(case, batch_size):
    pos, plddt, pts, feat = structure(case)
    seq, sets = toy_sets(len(pos))
    return seq, sets, s3f_ref.sequence_tables(state_dict(), seq, pos, plddt, pts, feat, sets, batch_size, ESM_CFG["heads"], ESM_CFG["layers"])


def csr(sets):
    return np.cumsum([0] + [len(s) for s in sets]).astype(np.int32), np.array([p for s in sets for p in s], dtype=np.int32)


@pytest.mark.parametrize("batch_size", [1, 2])
@pytest.mark.parametrize("case", [(37, 250), "cut", (9, 40)], ids=str)
def test_end_to_end_tables(model, case, batch_size):
    """Five masked sequences: with batch_size 2 the pairs (0, 1), (2, 3) and the short group (4)."""
    pos, plddt, pts, feat = structure(case)
    seq, sets, full64 = reference_tables(case, batch_size)
    model.set_structure(pos, plddt, pts, feat)
    out, full = model.set_logprobs(s2f.tokenize(seq), *csr(sets), s3f.pool_groups(len(sets), batch_size), want_full=True)
    err = np.abs(full - full64).max()
    print(f"{case} batch_size {batch_size}: max|table - float64| = {err:.3e} over {len(sets)} sequences")
    assert err <= TOL
    assert np.array_equal(out, np.concatenate([full[s][list(k)] for s, k in enumerate(sets)]))
    if batch_size == 2:                       # sequence 4 repeats sequence 0's sites with another partner (none): other values
        assert not np.array_equal(full[0], full[4])


def test_a_set_has_the_same_bits_alone_with_others_and_under_a_row_cap(model, row_cap):
    case = (37, 250)
    pos, plddt, pts, feat = structure(case)
    seq, sets = toy_sets(len(pos))
    model.set_structure(pos, plddt, pts, feat)
    tok = s2f.tokenize(seq)
    batch = model.set_logprobs(tok, *csr(sets), want_full=True)[1]
    assert np.array_equal(batch[0], batch[4])                    # batch_size 1: equal sets, equal bits
    for s in (1, 3):
        assert np.array_equal(model.set_logprobs(tok, *csr(sets[s:s + 1]), want_full=True)[1][0], batch[s])
    row_cap(1)
    assert np.array_equal(model.set_logprobs(tok, *csr(sets), want_full=True)[1], batch)
    pairs = model.set_logprobs(tok, *csr(sets), s3f.pool_groups(len(sets), 2), want_full=True)[1]
    row_cap(0)
    assert np.array_equal(model.set_logprobs(tok, *csr(sets), s3f.pool_groups(len(sets), 2), want_full=True)[1], pairs)


def restated_scores(n, batch_size):
    """The fixture assay n scored by the restatement: (rows, float64 scores)."""
    row, pos, plddt, (s_start, s_end), _ = fixture_assay(n)
    with open(os.path.join(TOY, row["pdb_file"].split(".")[0] + ".pkl"), "rb") as f:
        pts, feat, r2s = s3f_ref.read_surfaces([pickle.load(f)])
    seq = row["target_seq"]
    L = len(seq)
    pts, feat, _ = s3f_ref.truncate(pts, feat, r2s, s_start, 0, L)
    assay = pd.read_csv(os.path.join(TOY, row["DMS_filename"]))
    rows = s2f.sort_mutants(assay["mutant"], assay["DMS_score"])
    sets, seq_of = [], []
    for n_, (sites, _, _) in enumerate(rows):
        if n_ == 0 or sites != rows[n_ - 1][0]:
            sets.append(tuple(sorted(set(sites))))
        seq_of.append(len(sets) - 1)
    full = s3f_ref.sequence_tables(state_dict(), seq, pos[:L], plddt[:L], pts, feat, sets, batch_size, ESM_CFG["heads"], ESM_CFG["layers"])
    return row, rows, s2f_ref.scores(rows, full, seq_of)


@pytest.mark.parametrize("n", [0, 1])
def test_cli_reproduces_the_restatement_on_the_toy_assays(lib, tmp_path, n):
    from proteingym_amd import score_s3f_proteingym as cli
    row, rows, want = restated_scores(n, 2)                      # s3f_toy.yaml has batch_size: 2
    ckpt = str(tmp_path / "s3f.pth")
    torch.save({"model": {k: torch.as_tensor(np.array(v)) for k, v in state_dict().items()}}, ckpt)
    dims = f"{ESM_CFG['layers']},{ESM_CFG['embed_dim']},{ESM_CFG['heads']},{ESM_CFG['ffn_dim']}"
    base = ["-c", os.path.join(TOY, "s3f_toy.yaml"), "--datadir", TOY, "--ProteinGym_reference_file", os.path.join(TOY, "reference.csv"),
            "--structdir", TOY, "--surfdir", TOY, "--ckpt", ckpt, "--DMS_index", str(n), "--esm_dims", dims]
    out1 = tmp_path / "plain"
    assert cli.main(base + ["--output_scores_folder", str(out1)]) == 0
    got = pd.read_csv(out1 / row["DMS_filename"])
    assert list(got.columns) == ["Unnamed: 0", "mutant", "mutated_sequence", "DMS_score", "s3f_toy_score"]
    assert list(got["mutant"]) == [":".join(r[1]) for r in rows]
    err = np.abs(got["s3f_toy_score"].to_numpy() - want).max()
    print(f"assay {n}: max|score - float64| = {err:.3e}")
    assert err <= TOL + 0.5e-6                                    # the CSV rounds to 6 decimals
    out2 = tmp_path / "msa"
    assert cli.main(base + ["--output_scores_folder", str(out2), "--MSA_retrieval_location", os.path.join(TOY, "EVE")]) == 0
    got = pd.read_csv(out2 / row["DMS_filename"])
    eve = pd.read_csv(os.path.join(TOY, "EVE", row["DMS_filename"]))
    index = {":".join(r[1]): k for k, r in enumerate(rows)}
    common = [m for m in eve["mutant"] if m in index]
    assert 0 < len(common) < len(rows) and list(got["mutant"]) == common
    p = torch.tensor([want[index[m]] for m in common])
    e = torch.tensor([float(eve["EVE_ensemble"][list(eve["mutant"]).index(m)]) for m in common])
    msa = ((p - p.mean()) / p.std() + (e - e.mean()) / e.std()) / 2.0
    assert list(got.columns)[-1] == "s3f_toy_MSA_score"
    # the bound of test_gpu_s2f.py's MSA column: |dz| <= 2 d (1 + max|z|) sqrt(n / (n - 1)) / std for an error d in every score; the
    # column is z / 2 plus the EVE half, then the CSV's 6 decimals
    z = (p - p.mean()) / p.std()
    msa_tol = TOL * (1.0 + float(z.abs().max())) / float(p.std()) * np.sqrt(len(common) / (len(common) - 1.0)) + 0.5e-6
    err = np.abs(got["s3f_toy_MSA_score"].to_numpy() - msa.numpy()).max()
    print(f"assay {n} MSA column: max error {err:.3e}, bound {msa_tol:.3e}")
    assert err <= msa_tol


def test_bad_inputs_are_refused(lib, gnn):
    pos, plddt, pts, feat = structure((37, 17))
    with pytest.raises(_lib.PgmiError, match="surface points outside"):
        gnn.set_structure(pos, plddt, pts[:16], feat[:16])
    bad = np.array(pts)
    bad[3, 1] = np.nan
    with pytest.raises(_lib.PgmiError, match="not finite"):
        gnn.set_structure(pos, plddt, bad, feat)
    with pytest.raises(_lib.PgmiError, match="no structure set"):
        gnn.gvp_forward(np.zeros((1, 0, D_GNN), np.float32), np.zeros((1, 0, 20), np.float32))
    gnn.set_structure(pos, plddt, pts, feat)
    x, q = inputs((37, 17), 2)
    with pytest.raises(_lib.PgmiError, match="pool groups"):
        gnn.gvp_forward(x, q, pool_off=[0, 1])
    with pytest.raises(_lib.PgmiError, match="without an ESM2 model"):
        gnn.set_logprobs(s2f.tokenize("A" * 37), [0, 1], [0])
