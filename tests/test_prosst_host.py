"""ProSST structure tokens, host side (no GPU): the PDB reader and its refusals, the restatement's graph rules on the toy backbones (the
global edges, "more than 30 keeps 40", "at most 30 keeps all", the edge-feature indices), the checkpoint packing, the ignored and the
refused keys, the codebook reader, the fasta bytes and the CLI's flags; and the library's own graph pass (pgmi_op_prosst_subgraphs, host
only) against the restatement: the global edges, the node and edge CSR, and the per-copy edge lists the kernels read."""
import os

import numpy as np
import pytest
import torch

import prosst_cases
import prosst_ref
from proteingym_amd import _lib, prosst, prosst_structure_tokens as cli


def test_reader_reads_back_the_toy_backbone_and_names_the_sequence(tmp_path):
    X = prosst_cases.toy(37)
    p = tmp_path / "toy.pdb"
    p.write_text(prosst_cases.pdb_text(X))
    seq, got = prosst.read_backbone(str(p))
    assert got.dtype == np.float32 and np.array_equal(got, X)
    assert seq == "".join("AGSLKEVT"[i % 8] for i in range(37))
    lines = prosst_cases.pdb_text(X[:5], ["ALA", "MSE", "GLY", "XYZ", "TRP"]).splitlines()
    assert prosst.read_backbone(lines)[0] == "AXGXW"                       # seq1: an unknown name is X


def test_reader_takes_the_first_model_atom_records_and_first_altloc():
    X = prosst_cases.toy(9)
    lines = prosst_cases.pdb_text(X).splitlines()[:-2]
    het = "HETATM 9000  CA  HOH A 900      10.000  10.000  10.000  1.00 80.00           C"
    alt = lines[1][:30] + "   9.999   9.999   9.999" + lines[1][54:]       # a second CA of residue 1
    second_model = ["ENDMDL", "MODEL        2"] + lines
    seq, got = prosst.read_backbone(["MODEL        1"] + lines[:2] + [alt] + lines[2:] + [het] + second_model)
    assert len(seq) == 9 and np.array_equal(got, X)


def test_reader_refuses_a_missing_backbone_atom_and_three_residues():
    X = prosst_cases.toy(9)
    lines = prosst_cases.pdb_text(X).splitlines()
    no_o = [l for l in lines if not (l.startswith("ATOM") and l[12:16].strip() == "O" and int(l[22:26]) == 4)]
    with pytest.raises(ValueError, match=r"residue LEU A4 has no O atom"):
        prosst.read_backbone(no_o)
    with pytest.raises(ValueError, match="torch.cross"):
        prosst.read_backbone(prosst_cases.pdb_text(X[:3]).splitlines())
    with pytest.raises(ValueError, match="no residues"):
        prosst.read_backbone(["HETATM    1  CA  HOH A   1       0.000   0.000   0.000"])


@pytest.mark.parametrize("L", [9, 37, 131])
def test_graph_rules_of_the_restatement(L):
    X = prosst_cases.toy(L)
    st = prosst_cases.stats(X)
    d, edges = st["d"], st["edges"]
    assert d.dtype == np.float64
    # row-major (a, b), no loops, symmetric
    key = edges[0] * L + edges[1]
    assert (np.diff(key) > 0).all() and (edges[0] != edges[1]).all()
    assert set(map(tuple, edges.T)) == set(map(tuple, edges[::-1].T))
    for i, nodes in enumerate(st["subs"]):
        cand = int((d[i] < 10.0).sum())
        assert i in nodes and (np.diff(nodes) > 0).all()
        if cand > 30:
            assert len(nodes) == min(cand, 40)                               # more than 30: the first 40
            assert d[i][nodes].max() <= np.sort(d[i])[len(nodes) - 1]        # and they are the nearest ones
        else:
            assert len(nodes) == cand                                        # at most 30: all of them
        se, gid = prosst_ref.subgraph_edges(d, edges, nodes)
        assert (np.diff(gid) > 0).all()                                      # the subgraph's order is the global edges' order
        assert np.array_equal(edges[:, gid], nodes[se])
    if L == 131:
        assert max(len(n) for n in st["subs"]) == 40 and st["e_sub"] == 100178 and edges.shape[1] == 4128


@pytest.mark.parametrize("L", [9, 37, 131])
def test_library_graph_pass_equals_the_restatement(lib, L):
    """pgmi_op_prosst_subgraphs: the C++ graph pass of pgmi_prosst_set_structure, without a device."""
    X = prosst_cases.toy(L)
    st = prosst_cases.stats(X)
    d, edges = st["d"], st["edges"]
    g = prosst.host_subgraphs(X)
    assert np.array_equal(g["edges"], edges)
    node_off = np.concatenate([[0], np.cumsum([len(n) for n in st["subs"]])])
    assert np.array_equal(g["node_off"], node_off) and np.array_equal(g["nodes"], np.concatenate(st["subs"]))
    sub = [prosst_ref.subgraph_edges(d, edges, n) for n in st["subs"]]
    assert np.array_equal(g["edge_off"], np.concatenate([[0], np.cumsum([len(x) for _, x in sub])]))
    assert np.array_equal(g["edge_gid"], np.concatenate([x for _, x in sub]))
    # what the kernels read: per node copy its incoming edges, ascending source, as (global edge, copy of the source)
    in_off, in_gid, in_src = [0], [], []
    for i, (nodes, (se, gid)) in enumerate(zip(st["subs"], sub)):
        for q in range(len(nodes)):
            pick = np.flatnonzero(se[1] == q)                                # row-major (p, q): already ascending p
            in_gid.extend(gid[pick])
            in_src.extend(node_off[i] + se[0][pick])
            in_off.append(len(in_gid))
    assert np.array_equal(g["in_off"], in_off) and np.array_equal(g["in_gid"], in_gid) and np.array_equal(g["in_src"], in_src)
    assert np.array_equal(edges[1][g["in_gid"]], g["nodes"][np.repeat(np.arange(len(g["nodes"])), np.diff(g["in_off"]))])


def test_library_graph_pass_cut_and_refusals(lib):
    X = prosst_cases.toy(131)
    small = prosst.host_subgraphs(X, prosst.make_config(max_nodes=12, threshold=5))
    assert np.diff(small["node_off"]).max() == 12
    with pytest.raises(_lib.PgmiError, match="L = 3"):
        prosst.host_subgraphs(X[:3])
    with pytest.raises(_lib.PgmiError, match="max_nodes"):
        prosst.host_subgraphs(X, prosst.make_config(max_nodes=41))
    with pytest.raises(ValueError, match="max_distance"):
        prosst.PdbQuantizer(20, max_distance=8.0, state_dict={}, codebooks={})
    # the assign op refuses a product table it could not allocate before it touches a device
    with pytest.raises(_lib.PgmiError, match="products"):
        prosst.op_assign(np.zeros((40000, 256), np.float32), np.zeros((8192, 256), np.float32))


def test_edge_features_use_source_minus_target_and_the_global_index_difference():
    X = prosst_cases.toy(37)
    edges = prosst_cases.stats(X)["edges"]
    node_v, edge_s, edge_v = prosst_ref.features(X, edges, torch.float64)
    ca = np.asarray(X, np.float64)[:, 1]
    a, b = edges
    vec = ca[a] - ca[b]
    assert np.allclose(edge_v[:, 0].numpy(), vec / np.linalg.norm(vec, axis=1, keepdims=True), atol=1e-12)
    f = np.exp(-2 * np.arange(8) * np.log(1e4) / 16)
    assert np.allclose(edge_s[:, 16:24].numpy(), np.cos((a - b)[:, None] * f), atol=1e-5)
    assert np.allclose(edge_s[:, 24:].numpy(), np.sin((a - b)[:, None] * f), atol=1e-5)
    mu = np.linspace(0, 20, 16)
    assert np.allclose(edge_s[:, :16].numpy(), np.exp(-((np.linalg.norm(vec, axis=1)[:, None] - mu) / 1.25) ** 2), atol=1e-5)
    assert np.array_equal(node_v[-1, 0].numpy(), np.zeros(3)) and np.array_equal(node_v[0, 1].numpy(), np.zeros(3))
    assert np.allclose(np.linalg.norm(node_v[5].numpy(), axis=1), 1.0)


def test_pack_round_trip_ignored_and_refused_keys():
    sd = prosst.random_state_dict(3)
    shapes = prosst.key_shapes()
    blob = prosst.pack(sd)
    assert blob.dtype == np.float32 and blob.size == sum(int(np.prod(s)) for _, s in shapes)
    o = 0
    for k, s in shapes:
        n = int(np.prod(s))
        assert np.array_equal(blob[o:o + n].reshape(s), sd[k]), k
        o += n
    assert dict(shapes)["layers.5.conv.message_func.0.ws.weight"] == (256, 642)
    assert dict(shapes)["layers.0.ff_func.1.wh.weight"] == (64, 64) and dict(shapes)["W_e.1.wv.weight"] == (2, 2)
    assert not any("wsv" in k for k, _ in shapes)                            # vector_gate = False
    assert any(k.startswith("dense.") for k in sd) and any(k.endswith("dummy_param") for k in sd)     # carried and ignored
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    assert np.array_equal(prosst.pack(tsd), blob)
    with pytest.raises(ValueError, match="unexpected.*W_extra.weight"):
        prosst.pack(dict(sd, **{"W_extra.weight": np.zeros(3, np.float32)}))
    with pytest.raises(ValueError, match="missing.*W_out.1.ws.bias"):
        prosst.pack({k: v for k, v in sd.items() if k != "W_out.1.ws.bias"})
    with pytest.raises(ValueError, match="shape"):
        prosst.pack(dict(sd, **{"W_v.1.wh.weight": np.zeros((32, 4), np.float32)}))


def test_codebook_reader_npy(tmp_path):
    c = np.random.default_rng(0).standard_normal((20, 256))
    np.save(tmp_path / "20.npy", c)
    got = prosst.read_codebook(str(tmp_path / "20.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, c.astype(np.float32))
    assert prosst.find_codebook(str(tmp_path), 20).endswith("20.npy")
    np.save(tmp_path / "64.npy", c[:, :100])
    with pytest.raises(ValueError, match="expected"):
        prosst.read_codebook(str(tmp_path / "64.npy"))
    with pytest.raises(FileNotFoundError, match="never downloads"):
        prosst.find_codebook(str(tmp_path), 128)


def test_codebook_reader_joblib(tmp_path):
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    from sklearn.cluster import KMeans
    x = np.random.default_rng(1).standard_normal((60, 256))
    km = KMeans(n_clusters=20, n_init=1, random_state=0).fit(x)
    joblib.dump(km, tmp_path / "20.joblib")
    got = prosst.read_codebook(prosst.find_codebook(str(tmp_path), 20))
    assert np.array_equal(got, km.cluster_centers_.astype(np.float32))


def test_fasta_bytes_and_cli_flags():
    assert prosst.fasta_text("P1_x", [3, 0, 2047]) == ">P1_x\n3,0,2047"     # no trailing newline, as the reference writes it
    a = cli.parser().parse_args(["--pdb_dir", "d", "--vocab_size", "2048", "20", "--overwrite", "--out_dir", "o", "--model_path", "AE.pt",
                                 "--cluster_dir", "c"])
    assert (a.pdb_dir, a.pdb_file, a.vocab_size, a.overwrite, a.out_dir, a.model_path, a.cluster_dir) == ("d", None, [2048, 20], True, "o",
                                                                                                           "AE.pt", "c")
    assert cli.parser().parse_args(["--pdb_file", "x.pdb", "--out_dir", "o"]).vocab_size == [2048]
    with pytest.raises(SystemExit):
        cli.run(cli.parser().parse_args(["--pdb_file", "x.pdb", "--out_dir", "o", "--vocab_size", "33"]))
    with pytest.raises(SystemExit):
        cli.run(cli.parser().parse_args(["--pdb_file", "x.pdb"]))


def test_launcher_names_the_cli_and_its_flags():
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    text = open(os.path.join(root, "scripts", "scoring_DMS_zero_shot", "tokenize_ProSST_structures.sh")).read()
    assert "proteingym_amd.prosst_structure_tokens" in text
    known = {a.option_strings[0] for a in cli.parser()._actions}
    for flag in ("--pdb_dir", "--out_dir", "--vocab_size", "--model_path", "--cluster_dir"):
        assert flag in text and flag in known
