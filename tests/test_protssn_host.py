"""ProtSSN host code (proteingym_amd/protssn.py, score_protssn_proteingym.py) on the CPU: the PDB reader, the graph builder and the
edge attributes against slow loop restatements (tests/protssn_ref.py -- torch_geometric, Bio and rdkit are not installed here, so the
live reference produced no value in this file), the normalisation, the packing and its counts, the split of the first edge Linear,
the scoring rules, the ensemble column, the CLI's refusals, the HF key map and the launcher."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

import protssn_ref as R
from proteingym_amd import _lib, protssn, synthetic
from proteingym_amd import esm as pesm
from proteingym_amd import score_protssn_proteingym as cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ProtSSN_toy")
TOY_PDB = os.path.join(TOY, "DATASET", R.TOY_NAME, R.TOY_NAME + ".pdb")


def three_branch_coordinates():
    """19 residues, interleaved in index: 14 within 12 A of each other (more than k = 10 within 30 A), 4 in a second cluster 200 A
    away (fewer than k: all taken, in index order), and one 500 A from everything (none within 30 A: the nearest is taken).
    Coordinates are multiples of 1 / 64, so the float32 C-alpha difference the reference takes is exact at 500 A too and the bound
    below stays the float32 rounding of the attributes themselves."""
    rng = np.random.default_rng(21)
    ca = np.zeros((19, 3))
    big, small, alone = [0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 17, 18], [2, 5, 9, 16], 13
    ca[big] = 6.0 * rng.standard_normal((len(big), 3))
    ca[small] = np.array([200.0, 0.0, 0.0]) + 4.0 * rng.standard_normal((len(small), 3))
    ca[alone] = np.array([0.0, 500.0, 0.0])
    return np.round(ca * 64) / 64, big, small, alone


def test_pdb_reader_on_the_toy_structure():
    n, ca, c, seq = protssn.read_pdb(TOY_PDB)
    assert len(seq) == 40 and n.shape == ca.shape == c.shape == (40, 3) and n.dtype == np.float64
    assert seq == "MKVLAAGIVRHDESTNQCGPAVIFY" + "WLMKRHDESTNQCGP"          # two chains; the water and the residue without C are gone
    lines = open(TOY_PDB).read().splitlines()
    assert any(ln.startswith("HETATM") and ln[17:20] == "HOH" for ln in lines)
    assert sum(ln[12:16].strip() == "CA" for ln in lines if ln.startswith("ATOM")) == 41
    assert np.array_equal(ca, ca.astype(np.float32).astype(np.float64))      # Bio.PDB keeps float32 coordinates
    assert ca[0].tolist() == [float(np.float32(lines[2][30 + 8 * i:38 + 8 * i])) for i in range(3)]
    bad = [ln.replace("LYS A   2", "MSE A   2") for ln in lines]
    with pytest.raises(ValueError, match="MSE A2"):
        protssn.read_pdb(bad)
    with pytest.raises(ValueError, match="no residue"):
        protssn.read_pdb([ln for ln in lines if ln[12:16].strip() != "C"])
    second_model = lines[:-1] + ["ENDMDL", "MODEL        2"] + lines[1:4] + ["ENDMDL"]
    assert protssn.read_pdb(second_model)[3] == seq


@pytest.mark.parametrize("case", ["toy_k10", "toy_k20", "toy_k30", "branches"])
def test_graph_and_attributes_against_the_loop_restatement(case):
    if case == "branches":
        ca, big, small, alone = three_branch_coordinates()
        n, ca, c = R.toy_backbone(ca, seed=2)
        k = 10
    else:
        n, ca, c, _ = protssn.read_pdb(TOY_PDB)
        k = int(case[5:])
    centre, nb, dist = protssn.calpha_graph(ca, k)
    src, dst, dl = R.slow_graph(ca, k)
    assert centre.tolist() == src and nb.tolist() == dst
    assert np.array_equal(dist, np.array(dl))
    if case == "branches":
        deg = np.bincount(centre, minlength=len(ca))
        assert all(deg[i] == 10 for i in big) and all(deg[i] == 3 for i in small) and deg[alone] == 1
        for i in small:                                     # fewer than k: everything within 30 A, in ascending index
            assert nb[centre == i].tolist() == [j for j in small if j != i]
        order = np.argsort(((ca - ca[alone]) ** 2).sum(1))
        assert nb[centre == alone].tolist() == [order[1]] and dist[centre == alone][0] > 30
        i = big[0]                                          # more than k: the k nearest, nearest first
        assert nb[centre == i].tolist() == [int(j) for j in np.argsort(((ca - ca[i]) ** 2).sum(1))[1:11]]
    ea = protssn.edge_attributes(centre, nb, dist, n, ca, c)
    assert ea.shape == (len(src), 93) and ea.dtype == np.float32
    want = R.slow_edge_attr(src, dst, dl, n, ca, c)
    assert np.array_equal(ea[:, :65], want[:, :65]) and np.array_equal(ea[:, 80], want[:, 80])
    np.testing.assert_allclose(ea, want, rtol=1e-6, atol=1e-6)              # float32 rounding of values up to 30


def test_normalisation_includes_column_64():
    norm = protssn.load_norm(10, norm_dir=TOY)
    assert norm["pos_std"].shape == (3,) and norm["edge_attr_mean"].shape == norm["edge_attr_std"].shape == (93,)
    n, ca, c, _ = protssn.read_pdb(TOY_PDB)
    centre, nb, dist = protssn.calpha_graph(ca, 10)
    raw = protssn.edge_attributes(centre, nb, dist, n, ca, c)
    pos, ea = protssn.normalize(ca, raw, norm)
    assert pos.dtype == ea.dtype == np.float32
    np.testing.assert_allclose(pos, (ca - ca.mean(0)) / (norm["pos_std"].astype(np.float64).mean() + 1e-10), rtol=1e-6, atol=1e-6)
    assert np.array_equal(ea[:, :64], raw[:, :64])                           # the first 64 one-hot columns pass through
    want = (raw[:, 64:].astype(np.float64) - norm["edge_attr_mean"][64:]) / (norm["edge_attr_std"][64:].astype(np.float64) + 1e-10)
    np.testing.assert_allclose(ea[:, 64:], want, rtol=1e-6, atol=1e-6)
    assert np.all(ea[:, 64] != raw[:, 64])                                   # column 64, the last one-hot column, IS normalised
    for k in (20, 30):
        assert protssn.load_norm(k, norm_dir=TOY)["edge_attr_mean"].shape == (93,)
    with pytest.raises(FileNotFoundError, match="cath_k10_mean_attr.pt"):
        protssn.load_norm(10, norm_dir=os.path.dirname(TOY))


@pytest.mark.parametrize("D,h,layers", [(128, 64, 2), (128, 40, 1), (1280, 512, 1)])
def test_pack_then_unpack_reproduces_the_blocks_and_zero_pads(lib, D, h, layers):
    sd = protssn.random_state_dict(3, D, h, gain=0.5, layers=layers, bias_std=0.1)
    blob = protssn.pack(sd, D, h, layers)
    d = protssn.dims(D, h)
    assert d["Hh"] == 4 * D + 188 and d["Hp"] % 32 == 0 and 0 <= d["Hp"] - d["Hh"] < 32
    if D == 1280:
        assert (d["Hh"], d["Hp"]) == (5308, 5312)
    cfg = protssn.ProtssnConfig(abi_version=_lib.ABI_VERSION, node_in=D, hidden=h, layers=layers, edge_attr_dim=93, precision=_lib.PREC_F16X3)
    assert lib.pgmi_protssn_weight_count(C.byref(cfg)) == blob.size
    parts = protssn.unpack(blob, D, h, layers)
    Hh, Hp, hp = d["Hh"], d["Hp"], d["hp"]
    for n in range(layers):
        p, t = f"GNN_model.mpnn_layes.{n}.", parts[n]
        w1 = sd[p + "edge_mlp.0.weight"]
        assert np.array_equal(t["Wi"][:Hh], w1[:, :D]) and np.array_equal(t["Wj"][:Hh], w1[:, D:2 * D])
        assert np.array_equal(t["We"][:Hh, :94], w1[:, 2 * D:]) and w1.shape[1] == 2 * D + 94
        assert not t["Wi"][Hh:].any() and not t["Wj"][Hh:].any() and not t["We"][Hh:].any() and not t["We"][:, 94:].any()
        assert np.array_equal(t["b1"][:Hh], sd[p + "edge_mlp.0.bias"]) and not t["b1"][Hh:].any()
        assert np.array_equal(t["W2"][:h, :Hh], sd[p + "edge_mlp.3.weight"]) and not t["W2"][h:].any() and not t["W2"][:, Hh:].any()
        assert np.array_equal(t["b2"][:h], sd[p + "edge_mlp.3.bias"]) and not t["b2"][h:].any()
        w3 = sd[p + "node_mlp.0.weight"]
        assert np.array_equal(t["W3"][:, :D], w3[:, :D]) and np.array_equal(t["W3"][:, D:D + h], w3[:, D:]) and not t["W3"][:, D + h:].any()
        assert np.array_equal(t["b3"], sd[p + "node_mlp.0.bias"]) and np.array_equal(t["W4"], sd[p + "node_mlp.3.weight"])
        assert np.array_equal(t["b4"], sd[p + "node_mlp.3.bias"])
    assert np.array_equal(parts[-1]["lin_w"], sd["GNN_model.lin.weight"]) and np.array_equal(parts[-1]["lin_b"], sd["GNN_model.lin.bias"])
    with pytest.raises(ValueError, match="missing"):
        protssn.pack({k: v for k, v in sd.items() if "lin.bias" not in k}, D, h, layers)
    with pytest.raises(ValueError, match="unexpected"):
        protssn.pack(dict(sd, extra=np.zeros(1)), D, h, layers)
    with pytest.raises(ValueError, match="shape"):
        protssn.pack(sd, D, h + 32, layers)


def test_parameter_counts_are_the_readme_figures(lib):
    # protssn README.md: 148 M, 160 M and 184 M parameters for h = 512, 768 and 1280
    assert [round(protssn.param_count(1280, h) / 1e6) for h in (512, 768, 1280)] == [148, 160, 184]
    assert protssn.param_count(1280, 512) == 6 * (5308 * 2654 + 5308 + 512 * 5308 + 512 + 2560 * 1792 + 2560 + 1280 * 2560 + 1280) + 20 * 1280 + 20
    for field, value, msg in (("abi_version", 5, "ABI version"), ("node_in", 100, "multiple of 32"), ("hidden", 0, "hidden"),
                              ("hidden", 5000, "hidden"), ("layers", 0, "layers"), ("precision", _lib.PREC_BF16, "f16x3 or fp32"),
                              ("edge_chunk", -1, "edge_chunk")):
        ok = dict(abi_version=_lib.ABI_VERSION, node_in=128, hidden=64, layers=6, edge_attr_dim=93, precision=_lib.PREC_F16X3, edge_chunk=0)
        ok[field] = value
        cfg = protssn.ProtssnConfig(**ok)
        assert lib.pgmi_protssn_weight_count(C.byref(cfg)) == -1 and msg in lib.pgmi_last_error().decode()


def test_split_first_linear_equals_the_unsplit_product_in_float64():
    D, h = 128, 64
    sd = protssn.random_state_dict(4, D, h, gain=0.5, layers=1, bias_std=0.1)
    t = {k: v.astype(np.float64) for k, v in protssn.unpack(protssn.pack(sd, D, h, 1), D, h, 1)[0].items()}
    rng = np.random.default_rng(5)
    L, E = 23, 160
    x = rng.standard_normal((L, D))
    centre, nb = rng.integers(0, L, E), rng.integers(0, L, E)
    ea = rng.standard_normal((E, 94))
    w1, b1 = sd["GNN_model.mpnn_layes.0.edge_mlp.0.weight"].astype(np.float64), sd["GNN_model.mpnn_layes.0.edge_mlp.0.bias"].astype(np.float64)
    unsplit = np.concatenate([x[nb], x[centre], ea], axis=1) @ w1.T + b1
    Pi, Pj = x @ t["Wi"].T, x @ t["Wj"].T                                   # the per-node tables
    share = np.concatenate([ea, np.zeros((E, 2))], axis=1) @ t["We"].T + t["b1"]
    split = Pi[nb] + Pj[centre] + share
    assert np.abs(split[:, :700] - unsplit).max() < 1e-12
    assert not split[:, 700:].any()                                          # the pads stay exactly zero


def test_label_row_semantics_offset_and_mismatch():
    rng = np.random.default_rng(6)
    seq = "MKVLAAGIVR"
    lp = np.log(rng.dirichlet(np.ones(20), size=len(seq))).astype(np.float32)
    col = protssn.AA_ORDER.index
    assert protssn.AA_ORDER == "ARNDCQEGHILKMFPSTWYV" == R.AA
    one = lp[1, col("R")] - lp[1, col("K")]
    assert protssn.label_row("K2R", seq, lp) == one.item()
    two = (lp[4, col("G")] - lp[4, col("A")]).item()
    assert protssn.label_row("K2R:A5G", seq, lp) == sum([one.item(), two]) == protssn.label_row("K2R;A5G", seq, lp)
    assert protssn.label_row("wt", seq, lp) == 0 and protssn.label_row("WT", seq, lp) == 0 and protssn.label_row("K2R:wt", seq, lp) == one.item()
    for m in ("K2R", "K2R:A5G", "M1A;R10W", "wt"):
        assert protssn.label_row(m, seq, lp) == pytest.approx(R.label_row(m, seq, lp), abs=1e-12)
    # ':' wins when both separators appear: the ';' stays inside a row, which then does not parse
    with pytest.raises(ValueError, match="row"):
        protssn.label_row("K2R;A5G:V3I", seq, lp)
    # the ZIKV assay counts from 291
    assert protssn.OFFSETS == {"A0A140D2T1_ZIKV_Sourisseau_2019": 291}
    assert protssn.label_row("K292R", seq, lp, 291) == one.item()
    with pytest.raises(ValueError, match="A2R"):
        protssn.label_row("M1K:A2R", seq, lp)                                # the wild type at 2 is K: the error names the failing row
    with pytest.raises(ValueError, match="K2000R"):
        protssn.label_row("K2000R", seq, lp)


def test_ensemble_is_excluded_from_its_own_mean_on_a_rerun(tmp_path):
    df = pd.DataFrame({"mutant": ["A1C", "wt"], "DMS_score": [0.5, 1.0]})
    path = str(tmp_path / "X.csv")
    cols = {"ProtSSN_k10_h512": pd.Series([1.0, 0.0]), "ProtSSN_k20_h512": pd.Series([3.0, 0.0])}
    first = cli.write_columns(path, df, cols, True)
    assert first["ProtSSN_ensemble"].tolist() == [2.0, 0.0]
    second = cli.write_columns(path, df, cols, True)                        # the reference would give (1 + 3 + 2) / 3 here
    assert second["ProtSSN_ensemble"].tolist() == [2.0, 0.0]
    assert list(pd.read_csv(path).columns) == ["mutant", "DMS_score", "ProtSSN_k10_h512", "ProtSSN_k20_h512", "ProtSSN_ensemble"]
    third = cli.write_columns(path, df, {"ProtSSN_k30_h512": pd.Series([5.0, 0.0])}, True)      # a later call extends the file
    assert third["ProtSSN_ensemble"].tolist() == [3.0, 0.0]
    assert protssn.ensemble_mean({"ProtSSN_a": [1.0], "ProtSSN_ensemble": [9.0], "other": [7.0]}).tolist() == [1.0]
    with pytest.raises(ValueError, match="no ProtSSN column"):
        protssn.ensemble_mean({"ProtSSN_ensemble": [1.0]})


def test_cli_refusals(tmp_path):
    good = "egnn:\n  edge_attr_dim: 93\n  output_dim: 20\n  dropout: 0\n  n_layers: 6\n  residual: False\n  embedding: False\n  embedding_dim: 64\n  mlp_num: 2\n"
    yml = tmp_path / "egnn.yaml"
    yml.write_text(good + "gat:\n  n_layers: 2\n")
    base = ["--gnn_config", str(yml), "--mutant_dataset_dir", str(tmp_path), "--output_scores_folder", str(tmp_path / "out"), "--plm", "/nowhere"]
    args = cli.parser().parse_args(base + ["--gnn_model_name", "k10_h512", "k30_h1280"])
    assert cli.check_args(args) == [("ProtSSN_k10_h512", 10, 512), ("ProtSSN_k30_h1280", 30, 1280)] and args.layers == 6
    for extra, msg in ((["--gnn", "gat", "--gnn_model_name", "k10_h512"], "egnn"), (["--gnn", "gcn", "--gnn_model_name", "k10_h512"], "egnn"),
                       (["--gnn_model_name", "k15_h512"], "Invalid k: 15"), (["--gnn_model_name", "k10_h256"], "Invalid h: 256"),
                       (["--gnn_model_name", "k10_h512", "k20_h1024"], "Invalid h: 1024"), (["--gnn_model_name", "k10"], "expected k<k>_h<h>"),
                       ([], "gnn_model_name"), (["--gnn_model_name", "k15_h64", "--test_widths"], "Invalid k: 15")):
        with pytest.raises(ValueError, match=msg):
            cli.main(base + extra)
    for line, new in (("embedding: False", "embedding: True"), ("residual: False", "residual: True"), ("mlp_num: 2", "mlp_num: 3"),
                      ("dropout: 0", "dropout: 0.1"), ("edge_attr_dim: 93", "edge_attr_dim: 17")):
        yml.write_text(good.replace(line, new))
        with pytest.raises(ValueError, match=new.split(":")[0]):
            cli.main(base + ["--gnn_model_name", "k10_h512"])
    yml.write_text(good)
    with pytest.raises(FileNotFoundError, match="cath_k10_mean_attr.pt"):   # past the refusals: the first file it needs
        cli.main(base + ["--gnn_model_name", "k10_h512", "--repo_path", str(tmp_path)])


def test_hf_key_map_round_trip():
    from transformers import EsmConfig, EsmModel
    torch.manual_seed(0)
    hc = EsmConfig(vocab_size=33, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                   position_embedding_type="rotary", token_dropout=True, pad_token_id=1, mask_token_id=32, layer_norm_eps=1e-5)
    hf = EsmModel(hc)
    sd = hf.state_dict()
    cfg, fair = protssn.hf_to_fair(sd, hc.to_dict())
    assert cfg == dict(arch=_lib.ARCH_ESM2, layers=2, embed_dim=64, heads=2, ffn_dim=128, max_positions=0, token_dropout=1, emb_layer_norm_before=0)
    back = synthetic.blob_to_arrays(cfg, pesm.pack_state_dict(cfg, fair))   # the packed blob, and back, key by key
    pairs = {"embed_tokens.weight": "embeddings.word_embeddings.weight", "emb_layer_norm_after.weight": "encoder.emb_layer_norm_after.weight",
             "emb_layer_norm_after.bias": "encoder.emb_layer_norm_after.bias"}
    for i in range(2):
        for a, b in (("self_attn_layer_norm", "attention.LayerNorm"), ("self_attn.q_proj", "attention.self.query"),
                     ("self_attn.k_proj", "attention.self.key"), ("self_attn.v_proj", "attention.self.value"),
                     ("self_attn.out_proj", "attention.output.dense"), ("final_layer_norm", "LayerNorm"), ("fc1", "intermediate.dense"),
                     ("fc2", "output.dense")):
            for leaf in ("weight", "bias"):
                pairs[f"layers.{i}.{a}.{leaf}"] = f"encoder.layer.{i}.{b}.{leaf}"
    mapped = set()
    for k in pesm.expected_keys(cfg):
        if k.startswith("lm_head."):
            assert not back[k].any()                                         # EsmModel has no LM head; the residue rows never read it
            continue
        assert np.array_equal(back[k], sd[pairs[k]].numpy()), k
        mapped.add(pairs[k])
    left = set(sd) - mapped
    assert left and all(protssn._hf_ignored(k) for k in left), left          # the pooler, the contact head, rotary buffers
    for field, value, msg in (("position_embedding_type", "absolute", "rotary"), ("emb_layer_norm_before", True, "emb_layer_norm_before"),
                              ("layer_norm_eps", 1e-12, "layer_norm_eps"), ("vocab_size", 64, "vocab_size")):
        with pytest.raises(ValueError, match=msg):
            protssn.hf_to_fair(sd, dict(hc.to_dict(), **{field: value}))
    with pytest.raises(ValueError, match="missing"):
        protssn.hf_to_fair({k: v for k, v in sd.items() if "layer.1.output.dense.bias" not in k}, hc.to_dict())
    with pytest.raises(ValueError, match="unexpected"):
        protssn.hf_to_fair(dict(sd, **{"lm_head.decoder.weight": torch.zeros(1)}), hc.to_dict())
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        protssn.load_plm("facebook/esm2_t33_650M_UR50D")


def test_random_state_dict_is_xavier_normal_times_gain():
    sd = protssn.random_state_dict(1, 128, 64, gain=0.5, layers=1)
    w = sd["GNN_model.mpnn_layes.0.edge_mlp.0.weight"]
    assert w.shape == (700, 350) and abs(w.std() / (0.5 * np.sqrt(2.0 / 1050)) - 1) < 0.02
    assert not sd["GNN_model.mpnn_layes.0.edge_mlp.0.bias"].any()            # init_ zeroes the biases
    assert sd["GNN_model.lin.weight"].shape == (20, 128)
    again = protssn.random_state_dict(1, 128, 64, gain=0.5, layers=1)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert [k for k, _ in protssn.key_shapes(128, 64, 1)] == [f"GNN_model.mpnn_layes.0.{m}.{i}.{leaf}" for m in ("edge_mlp", "node_mlp")
                                                               for i in (0, 3) for leaf in ("weight", "bias")] + ["GNN_model.lin.weight", "GNN_model.lin.bias"]


def test_launcher_builds_a_command_line_the_cli_parses(tmp_path):
    """The launcher of the reference's name reads zero_shot_config.sh and passes the reference's flags."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text('export DMS_output_score_folder_subs="/data/pg/out_subs"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7", model_checkpoint="/w/protssn",
               model_name="k10_h512 k20_h768", DMS_and_structure_folder="/data/pdb-csv", ProtSSN_plm="/w/esm2_t33_650M_UR50D.pt")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", "scoring_ProtSSN_substitutions.sh")], env=env,
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_protssn_proteingym"
    a = cli.parser().parse_args(argv[1:])
    assert a.gnn_model_name == ["k10_h512", "k20_h768"] and a.gnn_model_dir == "/w/protssn" and a.use_ensemble and a.DMS_index == 7
    assert a.mutant_dataset_dir == "/data/pdb-csv" and a.output_scores_folder == "/data/pg/out_subs/ProtSSN" and a.plm.endswith(".pt")
    assert a.gnn == "egnn" and a.gnn_config.endswith("egnn.yaml") and a.score_info.endswith("protssn_scores.csv")
