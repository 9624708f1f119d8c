"""The ProSST structure quantizer on the MI355X against the float64 torch restatement (tests/prosst_ref.py) on the toy backbones of
tests/prosst_cases.py: the subgraph view, W_e, the node state of one subgraph after the last layer, the pooled row and the normalised
embedding, the tokens of two codebooks, the bits (equal node sets, chunking, codebooks per pass, the assign op), the isolated node, the
CLI and the refusals.

Bounds: every compared tensor within 10 x the deviation of fp32 torch from float64 on the same tensor, as test_gpu_s2f.py and
test_gpu_mpnn.py hold theirs; both numbers are printed.  A token may differ from the float64 one only where the float64 margin
d2(second) - d2(best) is at most 2 |delta| |c_best - c_second| with |delta| the embedding bound as an L2 norm, and at most 2 % of a case's
residues may be such (prosst_cases.codebook asserts that; with the committed seeds none is).  The message kernel cuts 32-row tiles from
the edge list: L = 9 has 44 global and 262 subgraph edges (a partial last tile each, more than one block) and anchors with equal node
sets; 37 has subgraphs between the threshold and the cut and in-degree 33; 131 has subgraphs cut to 40 nodes, in-degree 39, 100 178
subgraph edges (no multiple of 32) over 4 128 global edges, and one isolated node (every case has one).

Measured on the MI355X (profiles/prosst_tokens/README.md): errors at about 1 x fp32 torch's own deviation, e.g. L = 131 normalised
embedding 8.6e-8 against 1.0e-7 (bound 1.0e-6), node state 1.5e-6 against 1.8e-6; no token differs and none is exempt."""
import os

import numpy as np
import pytest
import torch

import prosst_cases
import prosst_ref
from proteingym_amd import _lib, prosst, prosst_structure_tokens as cli

pytestmark = pytest.mark.gpu
SIZES = [9, 37, 131]


@pytest.fixture(scope="module")
def model(lib):
    m = prosst.Quantizer(prosst.pack(prosst_cases.state_dict()))
    yield m
    m.close()


@pytest.fixture
def option(lib):
    def set_(name, n):
        _lib.check(lib.pgmi_set_option(name.encode(), int(n)))
    yield set_
    lib.pgmi_set_option(b"prosst_max_rows", 0)
    lib.pgmi_set_option(b"prosst_share_layer0", 1)


def run(model, L, **kw):
    model.set_structure(prosst_cases.toy(L))
    return model.embed(**kw)


@pytest.mark.parametrize("L", SIZES)
def test_subgraph_view_equals_the_restatement(model, L):
    X = prosst_cases.toy(L)
    st = prosst_cases.stats(X)
    model.set_structure(X)
    g = model.subgraphs()
    assert np.array_equal(g["edges"], st["edges"])
    assert np.array_equal(g["node_off"], np.concatenate([[0], np.cumsum([len(n) for n in st["subs"]])]))
    assert np.array_equal(g["nodes"], np.concatenate(st["subs"]))
    gids = [prosst_ref.subgraph_edges(st["d"], st["edges"], n)[1] for n in st["subs"]]
    assert np.array_equal(g["edge_off"], np.concatenate([[0], np.cumsum([len(x) for x in gids])]))
    assert np.array_equal(g["edge_gid"], np.concatenate(gids))
    if L == 131:
        assert len(g["edge_gid"]) == 100178 and len(g["edge_gid"]) % 32


@pytest.mark.parametrize("L", SIZES)
def test_edge_embedding_matches_the_restatement(model, L):
    X = prosst_cases.toy(L)
    model.set_structure(X)
    g = model.subgraphs()
    r64, r32 = (prosst_ref.edge_embed_np(prosst_cases.state_dict(), X, dt) for dt in (torch.float64, torch.float32))
    for name, got, ref, f32 in (("e_s", g["e_s"], r64[0], r32[0]), ("e_v", g["e_v"], r64[1], r32[1])):
        err, dev = np.abs(got - ref).max(), np.abs(f32 - ref).max()
        print(f"L {L} W_e {name}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
        assert err <= 10 * dev, name


def compare(L, got, share=""):
    r64, r32 = prosst_cases.reference(L)
    for name in ("node_s", "node_v", "pooled", "emb"):
        err, dev = np.abs(got[name] - r64[name]).max(), np.abs(r32[name].astype(np.float64) - r64[name]).max()
        print(f"L {L}{share} {name}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
        assert err <= 10 * dev, name


def outputs(model, L):
    sub = prosst_cases.TRACE_SUB[L]
    n = len(prosst_cases.stats(prosst_cases.toy(L))["subs"][sub])
    emb, pooled, ns, nv = run(model, L, want_pooled=True, sub=sub, n_nodes=n)
    return dict(emb=emb, pooled=pooled, node_s=ns, node_v=nv)


@pytest.mark.parametrize("L", SIZES)
def test_encoder_matches_the_restatement(model, L):
    compare(L, outputs(model, L))


def test_encoder_without_the_layer0_sharing_matches_too(model, option):
    option("prosst_share_layer0", 0)
    compare(37, outputs(model, 37), " (layer 0 per node copy)")


@pytest.mark.parametrize("K", [20, 128])
@pytest.mark.parametrize("L", SIZES)
def test_tokens(model, L, K):
    c = prosst_cases.codebook(K)
    ex, want = prosst_cases.exempt(L, c)
    run(model, L)
    tok = model.assign(c)
    assert tok.dtype == np.int32 and tok.min() >= 0 and tok.max() < K
    bad = np.flatnonzero((tok != want) & ~ex)
    print(f"L {L} K {K}: {int((tok != want).sum())} tokens differ, {int(ex.sum())} exempt, {len(set(want.tolist()))} distinct tokens")
    assert ex.sum() <= 0.02 * L and not len(bad), bad


def test_isolated_node_and_equal_node_sets(model):
    for L in SIZES:
        st = prosst_cases.stats(prosst_cases.toy(L))
        emb = run(model, L)
        iso = int(np.flatnonzero(st["cand"] == 1)[0])
        assert list(st["subs"][iso]) == [iso]                            # one node, no edges: every message sum is zero
        r64, r32 = prosst_cases.reference(L)
        dev = np.abs(r32["emb"][iso].astype(np.float64) - r64["emb"][iso]).max()
        assert np.abs(emb[iso] - r64["emb"][iso]).max() <= 10 * dev
        groups = {}
        for i, n in enumerate(st["subs"]):
            groups.setdefault(tuple(n), []).append(i)
        same = [g for g in groups.values() if len(g) > 1]
        if L == 9:
            assert same
        for g in same:                                                  # the anchor is not marked: equal node sets, equal bits
            for i in g[1:]:
                assert np.array_equal(emb[g[0]], emb[i]), (L, g)


def test_bits_do_not_depend_on_the_chunking(model, option):
    L = 131
    st = prosst_cases.stats(prosst_cases.toy(L))
    sub = prosst_cases.TRACE_SUB[L]
    n = len(st["subs"][sub])
    whole = run(model, L, want_pooled=True, sub=sub, n_nodes=n)
    rows = sum(len(s) for s in st["subs"])
    option("prosst_max_rows", rows // 4)                                # at least four chunks
    assert rows // (rows // 4) >= 3
    parts = run(model, L, want_pooled=True, sub=sub, n_nodes=n)
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)
    option("prosst_max_rows", 1)                                        # one subgraph per chunk
    for a, b in zip(whole, run(model, L, want_pooled=True, sub=sub, n_nodes=n)):
        assert np.array_equal(a, b)


def test_codebooks_of_one_pass_equal_separate_passes_and_the_assign_op(model):
    c20, c128 = prosst_cases.codebook(20), prosst_cases.codebook(128)
    emb = run(model, 37)
    both = (model.assign(c20), model.assign(c128))
    run(model, 37)
    t20 = model.assign(c20)
    run(model, 37)
    t128 = model.assign(c128)
    assert np.array_equal(both[0], t20) and np.array_equal(both[1], t128)
    assert np.array_equal(prosst.op_assign(emb, c20), t20) and np.array_equal(prosst.op_assign(emb, c128), t128)
    # the lowest index wins a tie: a duplicated centre is never chosen at its higher index
    dup = np.concatenate([c20, c20])
    assert np.array_equal(prosst.op_assign(emb, dup), t20)


def test_cli_writes_the_structure_sequence_tree(lib, tmp_path):
    pdb_dir, out, clusters = tmp_path / "pdb", tmp_path / "structure_sequence", tmp_path / "static"
    pdb_dir.mkdir(); clusters.mkdir()
    for name, L in (("TOY_A", 9), ("TOY_B", 37)):
        (pdb_dir / f"{name}.pdb").write_text(prosst_cases.pdb_text(prosst_cases.toy(L)))
    (pdb_dir / "BROKEN.pdb").write_text("\n".join(l for l in prosst_cases.pdb_text(prosst_cases.toy(9)).splitlines() if " CA " not in l))
    for K in (20, 128):
        np.save(clusters / f"{K}.npy", prosst_cases.codebook(K))
    ckpt = tmp_path / "AE.pt"
    torch.save({k: torch.as_tensor(np.array(v)) for k, v in prosst_cases.state_dict().items()}, ckpt)
    rc = cli.main(["--pdb_dir", str(pdb_dir), "--out_dir", str(out), "--vocab_size", "20", "128", "--model_path", str(ckpt),
                   "--cluster_dir", str(clusters)])
    assert rc == 1                                                      # BROKEN is reported and skipped; the run went on
    assert sorted(os.listdir(out)) == ["128", "20"]
    for K in (20, 128):
        assert sorted(os.listdir(out / str(K))) == ["TOY_A.fasta", "TOY_B.fasta"]
        for name, L in (("TOY_A", 9), ("TOY_B", 37)):
            head, body = (out / str(K) / f"{name}.fasta").read_bytes().split(b"\n")
            toks = [int(t) for t in body.split(b",")]
            assert head == b">" + name.encode() and len(toks) == L
            ex, want = prosst_cases.exempt(L, prosst_cases.codebook(K))
            assert all(t == w or e for t, w, e in zip(toks, want, ex))
    q = prosst.PdbQuantizer(20, model_path=str(ckpt), cluster_dir=str(clusters))
    try:
        seq, toks = q(str(pdb_dir / "TOY_A.pdb"), return_residue_seq=True)
        assert seq == "AGSLKEVTA" and isinstance(toks, list) and toks == q(str(pdb_dir / "TOY_A.pdb"))
        assert ",".join(map(str, toks)).encode() == (out / "20" / "TOY_A.fasta").read_bytes().split(b"\n")[1]
    finally:
        q.close()


def test_refusals(model):
    blob = prosst.pack(prosst_cases.state_dict())
    with pytest.raises(_lib.PgmiError, match=r"node \(256, 16\)"):
        prosst.Quantizer(blob, node_h=(256, 16))
    with pytest.raises(_lib.PgmiError, match="weight blob"):
        prosst.Quantizer(blob[:-1])
    run(model, 9)
    with pytest.raises(_lib.PgmiError, match="K = 0"):
        model.assign(np.zeros((0, 256), np.float32))
    with pytest.raises(_lib.PgmiError, match="outside 1 .. 8192"):
        model.set_structure(np.zeros((8193, 4, 3), np.float32))
    with pytest.raises(_lib.PgmiError, match="no structure set"):
        model.embed()
    with pytest.raises(_lib.PgmiError, match="L = 3"):
        model.set_structure(prosst_cases.toy(9)[:3])
    model.set_structure(prosst_cases.toy(9))
    with pytest.raises(_lib.PgmiError, match="no embedding"):
        model.assign(prosst_cases.codebook(20))
    bad = np.array(prosst_cases.toy(9))
    bad[2, 1, 0] = np.nan
    with pytest.raises(_lib.PgmiError, match="residue 2 is not finite"):
        model.set_structure(bad)
