"""S2F without a GPU: the torch restatement (tests/s2f_ref.py) against the arrays recorded from the reference's own GVP modules
(tests/golden/S2F_toy/reference_modules.npz, written by tests/golden/make_golden_s2f.py), the radius graph on the cap and the
isolated node, the window and position-set rules with the named assays, the packing and yaml refusals, the CSV layout and the `_MSA`
average, the PDB reader, and the refusals of the C ABI that need no device."""
import ctypes as C
import io
import os

import numpy as np
import pandas as pd
import pytest
import torch

import s2f_cases
import s2f_ref
from proteingym_amd import _lib, s2f, synthetic as S
from proteingym_amd import score_s2f_proteingym as cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "S2F_toy")
ESM_CFG = dict(S.ESM2_650M, layers=2, embed_dim=128, heads=2, ffn_dim=256)
ROUND_OFF = 1e-11                     # float64 against float64 on values of order 1 - 10, a few thousand additions per element


@pytest.fixture(scope="module")
def sd():
    return s2f.random_state_dict(5, ESM_CFG)


@pytest.fixture(scope="module")
def rec():
    return np.load(os.path.join(TOY, "reference_modules.npz"))


def close(a, b):
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    assert err <= ROUND_OFF, err


def test_restatement_matches_the_reference_modules(sd, rec):
    W = s2f_ref.tensors(sd, torch.float64)
    p0 = s2f_ref.SM + "layers.0."
    t = lambda k: torch.as_tensor(rec[k])
    gs, gv = s2f_ref.gvp(W, p0 + "conv.message_func.0.", t("msg_in_s"), t("msg_in_v"), True, 16)          # GVP
    close(gs, rec["gvp_s"]); close(gv, rec["gvp_v"])
    ls, lv = s2f_ref.tuple_ln(W, p0 + "norm.0.", t("tuple_s"), t("tuple_v"))                               # GVPLayerNorm, a zero vector row
    close(ls, rec["ln_s"]); close(lv, rec["ln_v"])
    fs, fv = s2f_ref.gvp(W, p0 + "ff_func.0.", t("tuple_s"), t("tuple_v"), True, 32)
    fs, fv = s2f_ref.gvp(W, p0 + "ff_func.1.", fs, fv, False, 16)
    close(fs, rec["ff_s"]); close(fv, rec["ff_v"])
    pos, _ = s2f_cases.toy(37)
    edges = s2f_ref.radius_edges(pos)
    assert np.array_equal(edges.numpy(), rec["edges"])
    x = torch.as_tensor(s2f_cases.inputs(37, 1, 128)[0][0]).double()
    es, ev = s2f_ref.edge_features(W, torch.as_tensor(np.array(pos)).double(), edges)
    close(es[:160], rec["edge_s"]); close(ev, rec["edge_v"])
    s, _ = s2f_ref.tuple_ln(W, s2f_ref.SM + "W_v.0.", x @ W[s2f_ref.SM + "residue_embdding.weight"].T, None)
    s, v = s2f_ref.gvp(W, s2f_ref.SM + "W_v.1.", s, None, False, 16)
    s, v = s2f_ref.conv_layer(W, p0, s, v, edges, es, ev)                                                 # GVPConvLayer
    close(s, rec["layer0_s"]); close(v, rec["layer0_v"])
    close(s2f_ref.gvp_gnn(W, pos, x)["out"], rec["gnn_out"])                                             # GVPGNN.forward


def test_esm2_restatement_matches_the_oracle():
    from oracle import esm_oracle as eo
    blob = S.random_weights(ESM_CFG, seed=3)
    sd = s2f.random_state_dict(5, ESM_CFG, esm_blob=blob)
    ocfg, W = eo.from_arrays(arrays=S.blob_to_arrays(ESM_CFG, blob), dtype=torch.float64, **ESM_CFG)
    tok = s2f.tokenize("ACDEFGHIKLMNPQRSTVWY")
    tok[4] = tok[9] = 32
    _, logits = s2f_ref.esm2(s2f_ref.tensors(sd, torch.float64), tok, 2, 2)
    ref = eo.forward_logits(ocfg, W, tok[None].astype(np.int64))[0]
    assert float((logits - ref).abs().max()) <= 1e-10


def test_radius_graph_cap_order_and_isolated_node():
    for L in (9, 37, 131):
        pos, _ = s2f_cases.toy(L)
        src, dst = s2f.radius_graph(pos)
        e = s2f_ref.radius_edges(pos).numpy()
        assert np.array_equal(src, e[0]) and np.array_equal(dst, e[1])
        assert L - 1 not in src and L - 1 not in dst                                   # the isolated node
    line = np.zeros((40, 3))
    line[:, 0] = 0.2 * np.arange(40)                                                    # everything within 10 A of everything
    src, dst = s2f.radius_graph(line)
    assert list(src[dst == 0]) == list(range(1, 33))                                    # self among the first 33: 32 edges
    assert list(src[dst == 39]) == list(range(0, 33))                                   # self not among them: 33 edges, lowest indices
    assert list(src[dst == 10]) == [j for j in range(33) if j != 10]
    two = np.array([[0, 0, 0], [10.0, 0, 0], [9.999, 0, 0]])
    src, dst = s2f.radius_graph(two)                                                    # strictly inside the radius
    assert sorted(zip(src, dst)) == [(0, 2), (1, 2), (2, 0), (2, 1)]


def test_windows_and_position_sets():
    assert s2f.window_for("X", (5,), 300) == (0, 300)
    assert s2f.window_for("X", (100, 1900), 2000) == (0, 1022)
    assert s2f.window_for("X", (1900, 100), 2000) == (2000 - 1022, 2000)
    assert s2f.window_for("X", (1000,), 2500) == (489, 1511)
    assert s2f.window_for("POLG_HCVJF_Qi_2014", (2000,), 3033) == (1981, 2225)
    assert s2f.window_for("A0A140D2T1_ZIKV_Sourisseau_2019", (300,), 3423) == (290, 794)
    assert s2f.window_for("B2L11_HUMAN_Dutta_2010_binding-Mcl-1", (150,), 198) == (119, 197)
    assert s2f.window_for(s2f.BRCA2_ID, (2900,), 3418) == (1820, 2832)                 # a window ending past 2832 is replaced
    assert s2f.window_for(s2f.BRCA2_ID, (100,), 3418) == (0, 1022)
    rows = s2f.sort_mutants(["A3C:D1E", "D1E", "A3C", "A3G", "D1E:A3C", "K2R"], [1, 2, 3, 4, 5, 6])
    assert [r[0] for r in rows] == [(0,), (0, 2), (1,), (2,), (2,), (2, 0)]            # sites are 0-based, in sub-mutation order
    assert [":".join(r[1]) for r in rows] == ["D1E", "D1E:A3C", "K2R", "A3C", "A3G", "A3C:D1E"]
    windows, csr, where = s2f.position_sets(rows, "X", 3)
    assert windows == [(0, 3)]
    assert list(csr[0][0]) == [0, 1, 3, 4, 5] and list(csr[0][1]) == [0, 0, 2, 1, 2]   # (2, 0) shares (0, 2)'s forward
    assert where == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 3), (0, 1)]
    long_rows = s2f.sort_mutants(["A101C", "A1901C"], [0, 0])
    lw, lcsr, lwhere = s2f.position_sets(long_rows, "X", 2000)
    assert lw == [(0, 1022), (978, 2000)] and list(lcsr[1][1]) == [1900 - 978] and lwhere == [(0, 0), (1, 0)]
    pos, pl = np.zeros((50, 3)), np.zeros(50)
    assert len(s2f.cut_structure(pos, pl, 10, 60, 20, 40)[0]) == 20
    with pytest.raises(ValueError, match="doesn't match the sequence range"):
        s2f.cut_structure(pos, pl, 10, 60, 5, 40)
    with pytest.raises(AssertionError):
        s2f.cut_structure(pos[:40], pl[:40], 10, 60, 10, 60)
    table = np.log(np.random.default_rng(0).random((2, 3, 20)))
    got = s2f.score_rows(rows[:2], where[:2], [table], [(0, 3)])
    o = s2f.RESIDUE_ORDER.index
    assert np.allclose(got, [table[0, 0, o("E")] - table[0, 0, o("D")],
                             table[1, 0, o("E")] - table[1, 0, o("D")] + table[1, 2, o("C")] - table[1, 2, o("A")]], atol=1e-6)


def test_packing_refusals(sd):
    full = s2f.random_state_dict(5, ESM_CFG, esm_blob=S.random_weights(ESM_CFG, seed=3))
    esm_blob, gvp_blob = s2f.pack(full, ESM_CFG)
    assert esm_blob.size == S.random_weights(ESM_CFG, seed=3).size
    assert gvp_blob.size == sum(int(np.prod(s)) for _, s in s2f.gvp_key_shapes(128))
    assert "model.sequence_model.mapping" in full and "mlp.layers.0.weight" in full          # ignored, not refused
    extra = dict(full)
    extra["model.structure_model.layers.0.dropout.0.vdropout.dummy_param"] = np.zeros(0, np.float32)
    s2f.pack(extra, ESM_CFG)
    with pytest.raises(ValueError, match="missing"):
        s2f.pack({k: v for k, v in full.items() if k != "linear.bias"}, ESM_CFG)
    with pytest.raises(ValueError, match="unexpected"):
        s2f.pack(dict(full, **{"model.structure_model.surf_W_v.1.ws.weight": np.zeros((2, 2), np.float32)}), ESM_CFG)
    with pytest.raises(ValueError, match="shape"):
        s2f.pack(dict(full, **{"linear.weight": np.zeros((21, 256), np.float32)}), ESM_CFG)


def test_yaml_refusals(tmp_path):
    ctx = dict(datadir="d", structdir="s", ckpt="c")
    cfg = s2f.load_yaml(os.path.join(TOY, "s2f_toy.yaml"), ctx)
    assert cfg["structure_path"] == "s" and cfg["surface_path"] is None and cfg["model_checkpoint"] == "c"
    assert s2f.check_yaml(cfg, 128, None) == dict(layers=5, radius=10.0, max_neighbors=32, plddt_threshold=70.0)
    with pytest.raises(ValueError, match="node_in_dim"):
        s2f.check_yaml(cfg, 1280, None)                                                # the released model's width is 1280
    with pytest.raises(ValueError, match="ESM-2-650M"):
        s2f.check_yaml(cfg, 128)
    with pytest.raises(ValueError, match="surface"):
        s2f.check_yaml(s2f.load_yaml(os.path.join(TOY, "s2f_toy.yaml"), dict(ctx, surfdir="/surf")), 128, None)

    def edited(path, value):
        c = s2f.load_yaml(os.path.join(TOY, "s2f_toy.yaml"), ctx)
        node = c
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = value
        return c
    sm = ("task", "model", "structure_model")
    for path, value, msg in ((sm + ("class",), "SurfGVP", "surface"), (sm + ("node_h_dim",), [128, 16], "node_h_dim"),
                             (sm + ("edge_h_dim",), [32, 1], "edge_h_dim"), (sm + ("vector_gate",), False, "vector_gate"),
                             (("task", "graph_construction_model", "edge_layers"), [dict({"class": "KNNEdge"})], "SpatialEdge"),
                             (("task", "class"), "PropertyPrediction", "ResidueTypePrediction")):
        with pytest.raises(ValueError, match=msg):
            s2f.check_yaml(edited(path, value), 128, None)


def test_csv_layout_and_msa_average(tmp_path):
    rows = s2f.sort_mutants(["A3C", "D1E:A3C", "K2R", "A3G"], [0.5, -1.25, 2.0, 0.0])
    pred = np.array([0.1, -2.0, 0.3, 1.5], dtype=np.float32)
    path = str(tmp_path / "out" / "X.csv")
    cli.write_scores(path, "s2f", rows, pred)
    text = open(path).read().splitlines()
    assert text[0] == ",mutant,mutated_sequence,DMS_score,s2f_score"
    assert text[1] == ",D1E:A3C,,-1.250000,0.100000" and text[4] == ",A3G,,0.000000,1.500000"
    eve = pd.read_csv(io.StringIO("mutant,EVE_ensemble\nA3G,1.0\nQ9Q,5.0\nD1E:A3C,-1.0\nK2R,0.5\n"))
    keep, msa = cli.msa_average(pred, [":".join(r[1]) for r in rows], eve)
    assert keep == [3, 0, 1]                                                            # the EVE file's order, common mutants only
    p, e = torch.tensor(pred[keep]), torch.tensor([1.0, -1.0, 0.5])
    want = ((p - p.mean()) / p.std() + (e - e.mean()) / e.std()) / 2.0                   # torch's std is the unbiased one
    assert np.abs(msa - want.numpy()).max() <= 1e-6
    cli.write_scores(path, "s2f", [rows[i] for i in keep], pred[keep], msa)
    got = pd.read_csv(path)
    assert list(got.columns) == ["Unnamed: 0", "mutant", "mutated_sequence", "DMS_score", "s2f_score", "s2f_MSA_score"]
    assert list(got["mutant"]) == ["A3G", "D1E:A3C", "K2R"]
    args = cli.parser().parse_args(["-c", "s2f.yaml", "--datadir", "d", "--ProteinGym_reference_file", "r.csv", "--structdir", "s", "--ckpt", "c",
                                    "--output_scores_folder", "o", "--DMS_index", "0", "--MSA_retrieval_location", "e", "--seed", "3"])
    assert args.DMS_index == 0 and args.seed == 3


def test_pdb_reader_takes_c_alpha_and_its_b_factor():
    pos, bf = s2f.read_ca(os.path.join(TOY, "toy.pdb"))
    want_pos, want_bf = s2f_cases.toy(37)
    assert pos.shape == (37, 3) and np.abs(pos - want_pos).max() <= 5e-4 and np.abs(bf - want_bf).max() <= 5e-3
    p2, b2, start, end = s2f.load_structure(TOY, "toy.pdb|toy.pdb", "5-78")
    assert len(p2) == 74 and (start, end) == (4, 78) and np.array_equal(p2[37:], pos)
    assert s2f.load_structure(TOY, "toy.pdb", "1-37", "POLG_HCVJF_Qi_2014")[2:] == (1981, 2225)
    assert list(s2f.tokenize("GAW")) == [0, 6, 5, 22, 2] and list(s2f.AA_COLS[:3]) == [6, 5, 8]
    with pytest.raises(ValueError):
        s2f.tokenize("AXA")


def test_abi_refusals_without_a_device(lib):
    good = s2f.make_config(128)
    n = lib.pgmi_s2f_weight_count(C.byref(good))
    assert n == sum(int(np.prod(s)) for _, s in s2f.gvp_key_shapes(128))
    assert lib.pgmi_s2f_weight_count(C.byref(s2f.make_config(1280))) == sum(int(np.prod(s)) for _, s in s2f.gvp_key_shapes(1280))
    for field, value, msg in (("abi_version", 5, "ABI version"), ("node_in", 100, "multiple of 32"), ("node_s", 128, "dimensions"),
                              ("edge_v", 2, "dimensions"), ("layers", 0, "layers"), ("layers", 9, "layers"), ("max_neighbors", 0, "max_neighbors"),
                              ("radius", 0.0, "radius"), ("radius", float("nan"), "radius"), ("plddt_threshold", float("inf"), "plddt")):
        bad = s2f.make_config(128)
        setattr(bad, field, value)
        assert lib.pgmi_s2f_weight_count(C.byref(bad)) == -1
        assert msg in lib.pgmi_last_error().decode()
    h = C.c_void_p()
    blob = np.zeros(8, np.float32)
    assert lib.pgmi_s2f_create(C.byref(good), _lib.ptr(blob, _lib._f32p), blob.size, None, 0, C.byref(h)) == _lib.EINVAL
    assert "weight blob" in lib.pgmi_last_error().decode() and not h.value
    assert lib.pgmi_s2f_create(C.byref(good), None, n, None, 0, C.byref(h)) == _lib.EINVAL
    for call in (lambda: lib.pgmi_s2f_set_structure(None, None, None, 3), lambda: lib.pgmi_s2f_graph(None, None, None, None, None, None),
                 lambda: lib.pgmi_s2f_gvp_forward(None, None, None, 1, None, None, None),
                 lambda: lib.pgmi_s2f_set_logprobs(None, None, 5, None, None, None, 1, None, None)):
        assert call() == _lib.EINVAL
    assert lib.pgmi_s2f_profile_model(None) is None
    lib.pgmi_s2f_destroy(None)
    assert lib.pgmi_set_option(b"s2f_max_rows", 4096) == 0 and lib.pgmi_set_option(b"s2f_max_rows", 0) == 0
    assert lib.pgmi_set_option(b"s2f_rows", 1) == _lib.EINVAL
