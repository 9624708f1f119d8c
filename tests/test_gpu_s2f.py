"""S2F on the MI355X against the float64 torch restatement (tests/s2f_ref.py) on the toy structures of tests/s2f_cases.py: the graph
and W_e, the GVP-GNN alone (pgmi_s2f_gvp_forward), the whole path over a small seeded ESM2 (pgmi_s2f_set_logprobs), the low-pLDDT
fallback, the bits of a position set alone / in a batch / under a row cap, the CLI on the toy assay, and the refusals.

Bounds: the node state after the last layer (the intermediate the library exposes) within 10 x the deviation of fp32 torch from
float64 on the same tensor, as test_gpu_mpnn.py holds its intermediates; log-probabilities and scores within the flat 1e-4 of DESIGN.md
section 3.  L = 9 is below one tile, 37 is odd and holds a node above the neighbour cap, 131 is past two 64-row tiles with an edge count
that is no multiple of 4, 16, 64 or 128.  The message kernel works on tiles of 32 edges of one node: the default cap of 32 neighbours
keeps every node within one tile, so one case raises the cap to 48."""
import ctypes as C
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import s2f_cases
import s2f_ref
from proteingym_amd import _lib, s2f, synthetic as S
from proteingym_amd import esm as pesm

pytestmark = pytest.mark.gpu
TOL = 1e-4
D_GNN = 128                                             # the GNN alone: any multiple of 32 is a valid input width
ESM_CFG = dict(S.ESM2_650M, layers=2, embed_dim=128, heads=2, ffn_dim=256)
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "S2F_toy")


@functools.lru_cache(maxsize=None)
def state_dict():
    sd = s2f.random_state_dict(5, ESM_CFG, esm_blob=S.random_weights(ESM_CFG, seed=3))
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def reference(L, B):
    """(float64 lp, node_s, node_v) and the fp32-torch deviation of each, computed once per case."""
    pos, plddt = s2f_cases.toy(L)
    x, q = s2f_cases.inputs(L, B, D_GNN)
    r64 = s2f_ref.gvp_forward(state_dict(), pos, plddt, x, q, torch.float64)
    r32 = s2f_ref.gvp_forward(state_dict(), pos, plddt, x, q, torch.float32)
    return r64, [float(np.abs(a - b).max()) for a, b in zip(r64, r32)]


@pytest.fixture(scope="module")
def gnn(lib):
    _, blob = s2f.pack(state_dict(), ESM_CFG)
    m = s2f.S2F(blob, node_in=D_GNN)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model(lib):
    m = s2f.from_state_dict(state_dict(), ESM_CFG)
    yield m
    m.close()
    m.esm.close()


@pytest.fixture
def row_cap(lib):
    def set_(n):
        _lib.check(lib.pgmi_set_option(b"s2f_max_rows", int(n)))
    yield set_
    lib.pgmi_set_option(b"s2f_max_rows", 0)


@pytest.mark.parametrize("L", [9, 37, 131])
def test_graph_and_edge_features(gnn, L):
    pos, plddt = s2f_cases.toy(L)
    gnn.set_structure(pos, plddt)
    src, dst, es, ev = gnn.graph()
    edges = s2f_ref.radius_edges(pos).numpy()
    assert np.array_equal(src, edges[0]) and np.array_equal(dst, edges[1])
    if L == 131:
        assert all(len(src) % t for t in (4, 16, 64, 128))
    W = s2f_ref.tensors(state_dict(), torch.float64)
    rs, rv = s2f_ref.edge_features(W, torch.as_tensor(np.asarray(pos, dtype=np.float64)), torch.as_tensor(edges))
    W32 = s2f_ref.tensors(state_dict(), torch.float32)
    ds, dv = s2f_ref.edge_features(W32, torch.as_tensor(np.array(pos)), torch.as_tensor(edges))
    for name, got, ref, f32 in (("e_s", es, rs, ds), ("e_v", ev, rv[:, 0], dv[:, 0])):
        err, dev = np.abs(got - ref.numpy()).max(), np.abs(f32.numpy() - ref.numpy()).max()
        print(f"L {L} {name}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
        assert err <= 10 * dev, name


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [9, 37, 131])
def test_gvp_forward_matches_the_restatement(gnn, L, B):
    pos, plddt = s2f_cases.toy(L)
    x, q = s2f_cases.inputs(L, B, D_GNN)
    (lp64, s64, v64), dev = reference(L, B)
    gnn.set_structure(pos, plddt)
    lp, ns, nv = gnn.gvp_forward(x, q, want_nodes=True)
    for name, got, ref, d in (("node_s", ns, s64, dev[1]), ("node_v", nv, v64, dev[2])):
        err = np.abs(got - ref).max()
        print(f"L {L} B {B} {name}: max|err| {err:.3e}; fp32 torch vs float64 {d:.3e} (bound {10 * d:.1e})")
        assert err <= 10 * d, name
    err = np.abs(lp - lp64).max()
    print(f"L {L} B {B} log-probabilities: max|err| {err:.3e} (fp32 torch {dev[0]:.3e})")
    assert err <= TOL
    low = np.asarray(plddt) < 70
    assert np.abs(lp[:, low] - torch.log_softmax(torch.as_tensor(q, dtype=torch.float64), -1).numpy()[:, low]).max() <= TOL


def test_gvp_forward_with_more_edges_at_a_node_than_one_message_tile(lib):
    """A neighbour cap of 48 at 12 A: nodes with more than 32 edges go through the message kernel in two tiles."""
    L, r, cap = 131, 12.0, 48
    pos, plddt = s2f_cases.toy(L)
    x, q = s2f_cases.inputs(L, 1, D_GNN)
    edges = s2f_ref.radius_edges(pos, r, cap)
    assert np.bincount(edges[1].numpy(), minlength=L).max() > 32
    out = {}
    for dtype in (torch.float64, torch.float32):
        W = s2f_ref.tensors(state_dict(), dtype)
        g = s2f_ref.gvp_gnn(W, pos, torch.as_tensor(x[0]).to(dtype), 5, r, cap)
        lp = s2f_ref.head_logprobs(W, g["out"], torch.as_tensor(q[0]).to(dtype), plddt)
        out[dtype] = [t.numpy() for t in (lp, g["node_s"], g["node_v"])]
    m = s2f.S2F(s2f.pack(state_dict(), ESM_CFG)[1], node_in=D_GNN, max_neighbors=cap, radius=r)
    try:
        m.set_structure(pos, plddt)
        assert np.array_equal(m.graph()[0], edges[0].numpy())
        got = m.gvp_forward(x, q, want_nodes=True)
    finally:
        m.close()
    for name, a, ref, f32 in zip(("lp", "node_s", "node_v"), got, out[torch.float64], out[torch.float32]):
        err, dev = np.abs(a[0] - ref).max(), np.abs(f32 - ref).max()
        print(f"cap {cap} {name}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e}")
        assert err <= (TOL if name == "lp" else 10 * dev), name


def toy_assay(L, seed=2):
    """A sequence and mutants (singles, doubles, repeats of a site set) in the reference's sorted order."""
    rng = np.random.default_rng(seed + L)
    seq = "".join(rng.choice(list(s2f.RESIDUE_ORDER), L))
    muts = set()
    while len(muts) < 12:
        k = 1 if len(muts) < 7 else 2
        ps = sorted(rng.choice(L - 1, k, replace=False))         # the isolated last residue is left to the table comparison
        muts.add(":".join(seq[p] + str(p + 1) + rng.choice([a for a in s2f.RESIDUE_ORDER if a != seq[p]]) for p in ps))
    muts = sorted(muts)
    return seq, s2f.sort_mutants(muts, np.arange(len(muts), dtype=float))


@functools.lru_cache(maxsize=None)
def reference_tables(L):
    seq, rows = toy_assay(L)
    pos, plddt = s2f_cases.toy(L)
    sets, set_of = [], []
    for sites, _, _ in rows:
        key = tuple(sorted(set(sites)))
        if key not in sets:
            sets.append(key)
        set_of.append(sets.index(key))
    full, esm_only = s2f_ref.set_tables(state_dict(), seq, pos, plddt, sets, ESM_CFG["heads"], ESM_CFG["layers"])
    return seq, rows, sets, set_of, full, esm_only


@pytest.mark.parametrize("L", [9, 37, 131])
def test_end_to_end_table_scores_and_fallback(model, L):
    seq, rows, sets, set_of, full64, esm64 = reference_tables(L)
    pos, plddt = s2f_cases.toy(L)
    windows, csr, where = s2f.position_sets(rows, "toy", L)
    assert windows == [(0, L)] and [w for w, _ in where] == [0] * len(rows) and [s for _, s in where] == set_of
    model.set_structure(pos, plddt)
    out, full = model.set_logprobs(s2f.tokenize(seq), *csr[0], want_full=True)
    err = np.abs(full - full64).max()
    print(f"L {L}: max|table - float64| = {err:.3e} over {len(sets)} sets")
    assert err <= TOL
    assert np.array_equal(out, np.concatenate([full[s][list(k)] for s, k in enumerate(sets)]))
    low = np.asarray(plddt) < 70
    err = np.abs(full[:, low] - esm64[:, low]).max()
    print(f"L {L}: low-pLDDT rows against the ESM-only log-softmax: {err:.3e}")
    assert err <= TOL
    got = s2f.score_rows(rows, where, [full], windows)
    ref = s2f_ref.scores(rows, full64, set_of)
    err = np.abs(got - ref).max()
    print(f"L {L}: max|score - float64| = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("L", [37, 131])
def test_a_set_has_the_same_bits_alone_in_a_batch_and_under_a_row_cap(model, row_cap, L):
    seq, rows, sets, _, _, _ = reference_tables(L)
    pos, plddt = s2f_cases.toy(L)
    _, csr, _ = s2f.position_sets(rows, "toy", L)
    set_off, set_pos = csr[0]
    model.set_structure(pos, plddt)
    tok = s2f.tokenize(seq)
    batch = model.set_logprobs(tok, set_off, set_pos, want_full=True)[1]
    for s in (0, len(sets) - 1):
        alone = model.set_logprobs(tok, [0, set_off[s + 1] - set_off[s]], set_pos[set_off[s]:set_off[s + 1]], want_full=True)[1]
        assert np.array_equal(alone[0], batch[s])
    row_cap(2 * max(len(model.graph()[0]), L + 2))                 # two sets per chunk
    assert np.array_equal(model.set_logprobs(tok, set_off, set_pos, want_full=True)[1], batch)


def test_gvp_forward_bits_do_not_depend_on_the_batch(gnn, row_cap):
    L = 37
    pos, plddt = s2f_cases.toy(L)
    x, q = s2f_cases.inputs(L, 3, D_GNN)
    gnn.set_structure(pos, plddt)
    batch = gnn.gvp_forward(x, q)
    assert np.array_equal(gnn.gvp_forward(x[1:2], q[1:2])[0], batch[1])
    row_cap(1)
    assert np.array_equal(gnn.gvp_forward(x, q), batch)


def test_cli_reproduces_the_restatement_on_the_toy_assay(lib, tmp_path):
    from proteingym_amd import score_s2f_proteingym as cli
    ref = pd.read_csv(os.path.join(TOY, "reference.csv"))
    seq = ref["target_seq"][0]
    L = len(seq)
    pos, plddt = s2f.read_ca(os.path.join(TOY, ref["pdb_file"][0]))
    assay = pd.read_csv(os.path.join(TOY, ref["DMS_filename"][0]))
    rows = s2f.sort_mutants(assay["mutant"], assay["DMS_score"])
    sets, set_of = [], []
    for sites, _, _ in rows:
        if tuple(sorted(set(sites))) not in sets:
            sets.append(tuple(sorted(set(sites))))
        set_of.append(sets.index(tuple(sorted(set(sites)))))
    full64, _ = s2f_ref.set_tables(state_dict(), seq, pos, plddt, sets, ESM_CFG["heads"], ESM_CFG["layers"])
    want = s2f_ref.scores(rows, full64, set_of)
    ckpt = str(tmp_path / "s2f.pth")
    torch.save({"model": {k: torch.as_tensor(np.array(v)) for k, v in state_dict().items()}}, ckpt)
    dims = f"{ESM_CFG['layers']},{ESM_CFG['embed_dim']},{ESM_CFG['heads']},{ESM_CFG['ffn_dim']}"
    base = ["-c", os.path.join(TOY, "s2f_toy.yaml"), "--datadir", TOY, "--ProteinGym_reference_file", os.path.join(TOY, "reference.csv"),
            "--structdir", TOY, "--ckpt", ckpt, "--DMS_index", "0", "--esm_dims", dims]
    out1 = tmp_path / "plain"
    assert cli.main(base + ["--output_scores_folder", str(out1)]) == 0
    got = pd.read_csv(out1 / ref["DMS_filename"][0])
    assert list(got.columns) == ["Unnamed: 0", "mutant", "mutated_sequence", "DMS_score", "s2f_toy_score"]
    assert list(got["mutant"]) == [":".join(r[1]) for r in rows]
    assert got["Unnamed: 0"].isna().all() and got["mutated_sequence"].isna().all()
    assert np.abs(got["s2f_toy_score"].to_numpy() - want).max() <= TOL + 0.5e-6               # the CSV rounds to 6 decimals
    out2 = tmp_path / "msa"
    assert cli.main(base + ["--output_scores_folder", str(out2), "--MSA_retrieval_location", os.path.join(TOY, "EVE")]) == 0
    got = pd.read_csv(out2 / ref["DMS_filename"][0])
    eve = pd.read_csv(os.path.join(TOY, "EVE", ref["DMS_filename"][0]))
    index = {":".join(r[1]): n for n, r in enumerate(rows)}
    common = [m for m in eve["mutant"] if m in index]
    assert 0 < len(common) < len(rows) and list(got["mutant"]) == common
    p = torch.tensor([want[index[m]] for m in common])
    e = torch.tensor([float(eve["EVE_ensemble"][list(eve["mutant"]).index(m)]) for m in common])
    msa = ((p - p.mean()) / p.std() + (e - e.mean()) / e.std()) / 2.0
    assert list(got.columns)[-1] == "s2f_toy_MSA_score"
    # z = (p - mean) / std.  An error of at most d = TOL in every p moves each p - mean by at most 2 d, and the centred vector by at most
    # 2 d sqrt(n) in length; std is that length over sqrt(n - 1), so it moves by at most 2 d sqrt(n / (n - 1)).  To first order
    # |dz| <= 2 d (1 + max|z|) sqrt(n / (n - 1)) / std.  The column is z / 2 plus the EVE half, which does not move; then the CSV's
    # 6 decimals.
    p64 = p.double()
    z = (p64 - p64.mean()) / p64.std()
    msa_tol = TOL * (1.0 + float(z.abs().max())) / float(p64.std()) * np.sqrt(len(common) / (len(common) - 1.0)) + 0.5e-6
    err = np.abs(got["s2f_toy_MSA_score"].to_numpy() - msa.numpy()).max()
    print(f"MSA column: max error {err:.3e}, bound {msa_tol:.3e}")
    assert err <= msa_tol
    assert np.abs(got["s2f_toy_score"].to_numpy() - p.numpy()).max() <= TOL + 0.5e-6


def test_bad_inputs_are_refused(lib, gnn, model):
    pos, plddt = s2f_cases.toy(9)
    bad = np.array(pos)
    bad[3, 1] = np.nan
    with pytest.raises(_lib.PgmiError, match="not finite"):
        gnn.set_structure(bad, plddt)
    gnn.set_structure(pos, plddt)
    with pytest.raises(ValueError):
        gnn.gvp_forward(np.zeros((1, 8, D_GNN), np.float32), np.zeros((1, 8, 20), np.float32))
    with pytest.raises(_lib.PgmiError, match="without an ESM2 model"):
        gnn.set_logprobs(s2f.tokenize("A" * 9), [0, 1], [0])
    model.set_structure(pos, plddt)
    tok = s2f.tokenize("ACDEFGHIK")
    with pytest.raises(_lib.PgmiError, match="tokens"):
        model.set_logprobs(tok[:-1], [0, 1], [0])
    with pytest.raises(_lib.PgmiError, match="out of range or not ascending"):
        model.set_logprobs(tok, [0, 2], [3, 3])
    with pytest.raises(_lib.PgmiError, match="out of range or not ascending"):
        model.set_logprobs(tok, [0, 1], [9])
    with pytest.raises(_lib.PgmiError, match="empty"):
        model.set_logprobs(tok, [0, 0, 1], [1])
    wide = dict(S.ESM2_650M, layers=1, embed_dim=64, heads=1, ffn_dim=128)
    esm = pesm.EsmModel(wide, S.random_weights(wide, seed=1))
    with pytest.raises(_lib.PgmiError, match="differs from the ESM2 model's width"):
        h = C.c_void_p()
        cfg = s2f.make_config(D_GNN)
        blob = s2f.pack(state_dict(), ESM_CFG)[1]
        _lib.check(lib.pgmi_s2f_create(C.byref(cfg), _lib.ptr(blob, _lib._f32p), blob.size, esm._h, 0, C.byref(h)))
    esm.close()
