"""ProteinMPNN host side, no GPU: tests/mpnn_ref.py (our float64 restatement, the GPU tests' yardstick) and proteingym_amd/mpnn.py
pinned to the unmodified reference (proteingym/baselines/protein_mpnn, driven by tests/mpnn_reference.py; those tests skip where the
reference tree is absent), and the hoisted / factorised decoder arithmetic of the HIP path as a numpy model against mpnn_ref.

Bound of the restatement pin: 10 x the reference's own fp32-vs-float64 deviation on the same inputs, computed here (about 2e-6)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mpnn_cases as mc
import mpnn_ref
import mpnn_reference as mr
from proteingym_amd import _lib, mpnn, score_proteinmpnn_proteingym as cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ProteinMPNN_toy")
needs_reference = pytest.mark.skipif(not mr.reference_available(), reason="reference ProteinMPNN code not on this machine")


@pytest.fixture(scope="module")
def sd():
    return mpnn.random_state_dict(7)


@pytest.fixture(scope="module")
def ref_model(sd):
    return mr.build_model(sd, mc.NUM_EDGES)


@needs_reference
@pytest.mark.parametrize("L,B", [(24, 1), (24, 5), (70, 5), (131, 1), (131, 5)])
def test_restatement_matches_the_reference_forward(sd, ref_model, L, B):
    c = mc.shape_case(L)
    assert mc.neighbour_gap_ok(c, mc.NUM_EDGES)
    S, randn = mc.mutants(c, B, seed=L)
    rep = lambda a: np.tile(a, (B,) + (1,) * np.ndim(a))
    args = (rep(c["X"]), S.astype(np.int64), rep(c["mask"]), np.ones((B, L)), rep(c["residue_idx"]), rep(c["chain_encoding"]), randn)
    ref32 = mr.forward(ref_model, *args)
    ref64 = mr.forward(ref_model, *args, dtype=torch.float64)
    rank = mpnn.rank_from_randn(randn, c["mask"])
    ours = mpnn_ref.forward(sd, mc.NUM_EDGES, c["X"], c["mask"], c["residue_idx"], c["chain_encoding"], S, rank)["log_probs"]
    own = float(np.abs(ref32 - ref64).max())
    err = float(np.abs(ours - ref32).max())
    print(f"L {L} B {B}: reference fp32 vs float64 {own:.2e}; restatement (float64) vs reference fp32 {err:.2e}, vs float64 "
          f"{np.abs(ours - ref64).max():.2e}")
    assert err <= 10 * own


@needs_reference
def test_parser_and_featurise_inputs_equal_the_reference_on_the_toy_pdb():
    u = mr.utils()
    pdb = os.path.join(TOY, "toy.pdb")
    d = u.parse_PDB(pdb, ca_only=False)
    ds = u.StructureDatasetPDB(d, truncate=None, max_length=200000)
    chains = [k[-1:] for k in d[0] if k[:9] == "seq_chain"]
    want = u.tied_featurize([ds[0]], torch.device("cpu"), {d[0]["name"]: (chains, [])}, None, None, None, None, None, ca_only=False)
    X, S, mask, chain_M, chain_enc, chain_M_pos, ridx = want[0], want[1], want[2], want[4], want[5], want[10], want[12]
    got = mpnn.featurize(mpnn.parse_pdb(pdb))
    assert [c for c, _, _ in mpnn.parse_pdb(pdb)] == ["A", "B"]
    assert np.array_equal(got["X"], X[0].numpy()) and got["X"].dtype == np.float32
    assert np.array_equal(got["mask"], mask[0].numpy()) and got["mask"].sum() == 68
    assert np.array_equal(got["residue_idx"], ridx[0].numpy())
    assert np.array_equal(got["chain_encoding"], chain_enc[0].numpy())
    assert np.array_equal(got["S"], S[0].numpy())
    assert np.array_equal(got["chain_M"], chain_M[0].numpy()) and np.array_equal(got["chain_M_pos"], chain_M_pos[0].numpy())
    assert got["seq"][16] == "X" and got["seq"][8] == "M"            # the absent residue number; HETATM MSE


@needs_reference
def test_designed_chains_and_fixed_positions_follow_the_reference():
    u = mr.utils()
    pdb = os.path.join(TOY, "toy.pdb")
    d = u.parse_PDB(pdb, ca_only=False)
    fixed = {d[0]["name"]: {"B": [1, 2, 7], "A": []}}
    want = u.tied_featurize([d[0]], torch.device("cpu"), {d[0]["name"]: (["B"], ["A"])}, fixed, None, None, None, None, ca_only=False)
    got = mpnn.featurize(mpnn.parse_pdb(pdb), ["B"], fixed[d[0]["name"]])
    for key, i in (("X", 0), ("S", 1), ("mask", 2), ("chain_M", 4), ("chain_encoding", 5), ("chain_M_pos", 10), ("residue_idx", 12)):
        assert np.array_equal(got[key], want[i][0].numpy()), key


@needs_reference
def test_blob_order_is_the_reference_state_dict_order(sd, ref_model):
    want = [(k, tuple(v.shape)) for k, v in ref_model.state_dict().items()]
    assert want == [(k, tuple(s)) for k, s in mpnn.key_shapes()]
    blob = mpnn.blob_from_state_dict(ref_model.state_dict())
    assert np.array_equal(blob, np.concatenate([v.numpy().ravel() for v in ref_model.state_dict().values()]))


def test_blob_size_is_the_library_count(lib, sd):
    c = mpnn.MpnnConfig(abi_version=_lib.ABI_VERSION, hidden=128, num_edges=48, enc_layers=3, dec_layers=3, precision=_lib.PREC_FP32)
    assert lib.pgmi_mpnn_weight_count(C.byref(c)) == mpnn.blob_from_state_dict(sd).size
    c.hidden = 64
    assert lib.pgmi_mpnn_weight_count(C.byref(c)) == -1
    with pytest.raises(_lib.PgmiError, match="shape"):
        mpnn.blob_from_state_dict(dict(sd, **{"W_e.weight": np.zeros((128, 64), np.float32)}))


def test_num_edges_is_limited_to_the_three_row_tiles_of_the_edge_kernel(lib):
    c = mpnn.MpnnConfig(abi_version=_lib.ABI_VERSION, hidden=128, num_edges=1, enc_layers=3, dec_layers=3, precision=_lib.PREC_FP32)
    assert lib.pgmi_mpnn_weight_count(C.byref(c)) > 0
    for bad in (0, 49, 64):
        c.num_edges = bad
        assert lib.pgmi_mpnn_weight_count(C.byref(c)) == -1
        assert "num_edges" in lib.pgmi_last_error().decode()


def test_rank_is_the_reference_argsort_line():
    rng = np.random.default_rng(3)
    L = 97
    randn = rng.standard_normal((6, L)).astype(np.float32)
    mask = (rng.random(L) > 0.1).astype(np.float32)
    chain_M = (np.arange(L) < 60).astype(np.float32)
    chain_M_pos = (rng.random(L) > 0.2).astype(np.float32)
    # protein_mpnn_utils.py:1080-1082 as written, on the product the script passes in
    cm = torch.from_numpy(chain_M * chain_M_pos)[None] * torch.from_numpy(mask)[None]
    order = torch.argsort((cm + 0.0001) * (torch.abs(torch.from_numpy(randn))))
    got = mpnn.rank_from_randn(randn, mask, chain_M, chain_M_pos)
    assert got.dtype == np.int32
    for b in range(6):
        assert np.array_equal(order[b].numpy()[got[b]], np.arange(L)) and np.array_equal(np.argsort(got[b]), order[b].numpy())
    assert np.array_equal(got, mpnn_ref.rank_from_randn(randn, mask, chain_M, chain_M_pos))


@needs_reference
def test_cli_option_names_are_the_reference_parser_s():
    ours = {a.option_strings[0]: a for a in cli.parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    assert set(mr.option_names()) <= set(ours)
    assert set(ours) - set(mr.option_names()) == {"--device", "--max_batch"}
    text = cli.parser().format_help()
    assert "no effect on the score" in text


@pytest.mark.parametrize("L", [24, 70, 131])
def test_hoisted_and_factorised_decoder_is_the_model(sd, L):
    """What the HIP decoder computes (W1 split by input block and hoisted, W3 after the sum over the edges), in float64."""
    c = mc.shape_case(L)
    S, randn = mc.mutants(c, 3, seed=L + 1)
    rank = mpnn.rank_from_randn(randn, c["mask"])
    o = mpnn_ref.forward(sd, mc.NUM_EDGES, c["X"], c["mask"], c["residue_idx"], c["chain_encoding"], S, rank)
    f = mpnn_ref.factorised_log_probs(sd, o["h_V"], o["h_E"], o["E_idx"], c["mask"], S, rank)
    assert np.abs(f - o["log_probs"]).max() < 1e-12


def test_cli_refuses_a_sequence_of_another_length(tmp_path):
    import pandas as pd
    df = pd.read_csv(os.path.join(TOY, "TOY_PMPNN_DMS.csv"))
    df.loc[3, "mutated_sequence"] = df.loc[3, "mutated_sequence"][:-1]
    df.to_csv(tmp_path / "TOY_PMPNN_DMS.csv", index=False)
    with pytest.raises(SystemExit, match="69 residues"):
        cli.main(["--DMS_reference_file_path", os.path.join(TOY, "TOY_PMPNN_MAPPING.csv"), "--DMS_data_folder", str(tmp_path),
                  "--structure_folder", TOY, "--DMS_index", "0", "--checkpoint", "unused.pt", "--output_scores_folder", str(tmp_path)])


def test_row_normals_depend_on_seed_and_row_only():
    a = cli.row_randn(5, 3, 70)
    torch.manual_seed(123)
    torch.randn(1000)
    assert np.array_equal(a, cli.row_randn(5, 3, 70)) and not np.array_equal(a, cli.row_randn(5, 4, 70))
    assert not np.array_equal(a, cli.row_randn(6, 3, 70)) and a.dtype == np.float32


def test_golden_fixtures_are_consistent():
    import pandas as pd
    ref = pd.read_csv(os.path.join(TOY, "TOY_PMPNN_REFERENCE.csv"))
    dms = pd.read_csv(os.path.join(TOY, "TOY_PMPNN_DMS.csv"))
    assert list(ref.columns) == ["mutant", "mutated_sequence", "pmpnn_ll"] and list(ref["mutant"]) == list(dms["mutant"])
    assert np.load(os.path.join(TOY, "TOY_PMPNN_RANDN.npy")).shape == (len(dms), 70)
    # the recorded scores are the restatement's, from the recorded normals
    feat = mpnn.featurize(mpnn.parse_pdb(os.path.join(TOY, "toy.pdb")))
    S = mpnn.encode_sequences(list(dms["mutated_sequence"]), 70)
    rank = mpnn.rank_from_randn(np.load(os.path.join(TOY, "TOY_PMPNN_RANDN.npy")), feat["mask"], feat["chain_M"], feat["chain_M_pos"])
    o = mpnn_ref.forward(mpnn.random_state_dict(7), 48, feat["X"], feat["mask"], feat["residue_idx"], feat["chain_encoding"], S, rank)
    assert np.abs(o["scores"] - ref["pmpnn_ll"].to_numpy()).max() < 2e-5
