"""S3F without a GPU: the torch restatement (tests/s3f_ref.py) against the arrays recorded from the reference's own SurfGVP
(tests/golden/S3F_toy/reference_modules.npz, written by tests/golden/make_golden_s3f.py), the host-side fold of the surface MLP in
float64 numpy against the unfolded restatement, packing and yaml acceptance and refusals, the surface reader with several files and
the truncation's re-indexing, the loader's pool groups, the CLI's flags, the fixtures' k-NN margins, and the ABI's refusals."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import s2f_cases
import s2f_ref
import s3f_cases
import s3f_ref
from proteingym_amd import _lib, s2f, s3f, synthetic as S
from proteingym_amd import score_s3f_proteingym as cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "S3F_toy")
ESM_CFG = dict(S.ESM2_650M, layers=2, embed_dim=128, heads=2, ffn_dim=256)
TOL = 1e-11                                            # S2F's bound on its restatement against the recorded modules
SM = s2f_ref.SM


@pytest.fixture(scope="module")
def sd():
    return s3f.random_state_dict(5, ESM_CFG)


@pytest.fixture(scope="module")
def rec():
    return np.load(os.path.join(TOY, "reference_modules.npz"))


@pytest.fixture(scope="module")
def toy():
    """(C-alpha positions, the unpickled surface dict, its (points, features, res2surf))."""
    pos, _ = s2f.read_ca(os.path.join(TOY, "toy.pdb"))
    with open(os.path.join(TOY, "toy.pkl"), "rb") as f:
        d = pickle.load(f)
    return pos, d, s3f_ref.read_surfaces([d])


def test_restatement_matches_the_reference_surfgvp(sd, rec, toy):
    pos, _, (pts, feat, _) = toy
    assert bool(rec["residue2surface_is_none"])                  # the live module: the readout pools over every surface point
    W = s2f_ref.tensors(sd, torch.float64)
    x = torch.as_tensor(s2f_cases.inputs(37, 2, 128)[0]).double()
    trace = {}
    one = s3f_ref.surf_gvp(W, pos, pts, feat, [x[0]], trace=trace)
    two = s3f_ref.surf_gvp(W, pos, pts, feat, [x[0], x[1]])
    st = s3f_ref.surface_structure(W, pos, pts, x)
    # the recorded edges come nearest first per centre; the restatement's by ascending source
    ei = rec["init_edge_index"]
    order = np.lexsort((ei[0], ei[1]))
    assert np.array_equal(ei[:, order], st["edges"].numpy())
    vec = (torch.as_tensor(np.array(pts)).double()[st["edges"][0]] - torch.as_tensor(np.array(pts)).double()[st["edges"][1]]).numpy()
    pairs = [("node_feature (batch of one)", one["node_feature"][0], rec["node_feature_1"]),
             ("node_feature (batch of two)", two["node_feature"].reshape(-1, 256), rec["node_feature_2"]),
             ("surface_feature_init node", trace["init"][:96], rec["init_node"]), ("surface_feature_init vec", vec, rec["init_vec"][order]),
             ("surface layer 0 s", trace["layer0_s"][:96], rec["layer0_s"]), ("surface layer 0 v", trace["layer0_v"], rec["layer0_v"]),
             ("pooled row", one["pooled"], rec["pooled"])]
    keep = order < 320                                            # the rbf rows that were recorded
    rbf = s2f_ref.rbf(torch.as_tensor(np.linalg.norm(vec, axis=1)))
    pairs.append(("surface_feature_init rbf", rbf[keep], rec["init_rbf"][order[keep]]))
    for name, got, want in pairs:
        err = np.abs(np.asarray(got) - want).max()
        print(f"{name}: max|err| {err:.3e}")
        assert err <= TOL, name
    assert not np.allclose(two["node_feature"][0].numpy(), one["node_feature"][0].numpy(), atol=1e-6)       # the partner changes the row


def test_fold_matches_the_unfolded_restatement(sd, toy):
    """The pre-LayerNorm row of the surface MLP from s3f.fold's float64 arrays, in plain numpy, against surf_in_linear on the 3 x 1281
    rows, the mean, and the 1322-wide Linear."""
    pos, _, (pts, feat, _) = toy
    D = 128
    x = s2f_cases.inputs(37, 1, D)[0][0].astype(np.float64)
    _, res, dist = s3f_ref.surface_lists(pos, pts)
    f = s3f.fold(sd, D)
    Z = x @ f["Wz"].T
    folded = Z[res].mean(1) + np.concatenate([feat.astype(np.float64), dist.mean(1, keepdims=True)], 1) @ f["Wsf"].T + f["b1"]
    W = s2f_ref.tensors(sd, torch.float64)
    h = torch.cat([torch.as_tensor(x)[torch.as_tensor(res.reshape(-1))], torch.as_tensor(dist.reshape(-1, 1))], -1).view(len(pts), 3, -1)
    h = (h @ W[SM + "surf_in_linear.weight"].T).mean(1)
    want = torch.cat([h, torch.as_tensor(feat).double()], -1) @ W[SM + "surf_in_mlp.0.weight"].T + W[SM + "surf_in_mlp.0.bias"]
    err = np.abs(folded - want.numpy()).max()
    print(f"folded pre-LayerNorm row: max|err| {err:.3e}")
    assert err <= TOL
    # and through the LayerNorm, the ReLU and the second Linear, against the restatement's surface_input
    ln = (folded - folded.mean(1, keepdims=True)) / np.sqrt(folded.var(1, keepdims=True) + 1e-5)
    ln = np.maximum(ln * sd[SM + "surf_in_mlp.2.weight"] + sd[SM + "surf_in_mlp.2.bias"], 0.0)
    out = ln @ sd[SM + "surf_in_mlp.4.weight"].astype(np.float64).T + sd[SM + "surf_in_mlp.4.bias"]
    ref = s3f_ref.surface_input(W, torch.as_tensor(x), res, dist, torch.as_tensor(feat).double()).numpy()
    assert np.abs(out - ref).max() <= TOL


def test_packing_and_its_refusals(sd, lib):
    full = dict(sd)
    for k, a in S.blob_to_arrays(ESM_CFG, S.random_weights(ESM_CFG, seed=3)).items():
        full[s2f.SEQ_PREFIX + k] = a
    esm_blob, blob = s3f.pack(full, ESM_CFG)
    cfg = s3f.S3fConfig(s2f=s2f.make_config(128), surf_feat=42, surf_res_neighbors=3, surf_neighbors=16)
    assert blob.size == lib.pgmi_s3f_weight_count(C.byref(cfg)) and blob.dtype == np.float32
    n_res = lib.pgmi_s2f_weight_count(C.byref(cfg.s2f))
    assert np.array_equal(blob[:n_res], s2f.pack({k: v for k, v in full.items() if "surf_" not in k}, ESM_CFG)[1])
    f = s3f.fold(full, 128)
    assert np.array_equal(blob[n_res:n_res + 256 * 128], f["Wz"].astype(np.float32).ravel())
    mlp, gnn = s3f.surf_key_shapes(128)
    assert blob.size == n_res + 256 * 128 + 256 * 43 + 256 * 3 + 128 * 256 + 128 + sum(int(np.prod(s)) for _, s in gnn)
    assert not any("residue_embdding" in k or k.startswith("linear") for k, _ in gnn) and len(mlp) == 7
    with pytest.raises(ValueError, match="missing"):
        s3f.pack({k: v for k, v in full.items() if k != SM + "surf_in_linear.weight"}, ESM_CFG)
    with pytest.raises(ValueError, match="missing"):
        s3f.pack({k: v for k, v in full.items() if "surf_layers.4.norm.1" not in k}, ESM_CFG)
    with pytest.raises(ValueError, match="unexpected"):
        s3f.pack(dict(full, **{SM + "surf_extra.weight": np.zeros(3, np.float32)}), ESM_CFG)
    with pytest.raises(ValueError, match="shape"):
        s3f.pack(dict(full, **{SM + "surf_in_mlp.0.weight": np.zeros((256, 128 + 41), np.float32)}), ESM_CFG)
    with pytest.raises(ValueError, match="unexpected"):           # an S3F state dict is not an S2F one
        s2f.pack(full, ESM_CFG)


def test_yaml_acceptance_and_refusals():
    ctx = dict(datadir="d", structdir="s", surfdir="/surf", ckpt="c")
    path = os.path.join(TOY, "s3f_toy.yaml")
    cfg = s2f.load_yaml(path, ctx)
    assert cfg["surface_path"] == "/surf"
    assert s3f.check_yaml(cfg, 128, None) == dict(layers=5, radius=10.0, max_neighbors=32, plddt_threshold=70.0, batch_size=2)
    with pytest.raises(ValueError, match="surface"):              # the S2F path still refuses this configuration
        s2f.check_yaml(cfg, 128, None)
    with pytest.raises(ValueError, match="surface_path"):
        s3f.check_yaml(s2f.load_yaml(path, dict(ctx, surfdir="")), 128, None)
    with pytest.raises(ValueError, match="ESM-2-650M"):
        s3f.check_yaml(cfg, 128)

    def edited(keys, value):
        c = s2f.load_yaml(path, ctx)
        node = c
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = value
        return c
    sm = ("task", "model", "structure_model")
    for keys, value, msg in ((sm + ("class",), "GVPGNN", "SurfGVP"), (sm + ("surf_in_dim",), [40, 0], "surf_in_dim"),
                             (sm + ("surf_edge_in_dim",), [32, 1], "surf_edge_in_dim"), (sm + ("num_surf_res_neighbor",), 4, "num_surf_res_neighbor"),
                             (sm + ("num_surf_graph_neighbor",), 8, "num_surf_graph_neighbor"), (sm + ("node_h_dim",), [128, 16], "node_h_dim"),
                             (sm + ("vector_gate",), False, "vector_gate"), (("batch_size",), 0, "batch_size"),
                             (("task", "class"), "PropertyPrediction", "ResidueTypePrediction")):
        with pytest.raises(ValueError, match=msg):
            s3f.check_yaml(edited(keys, value), 128, None)
    assert s3f.check_yaml(edited(("batch_size",), 1), 128, None)["batch_size"] == 1


def surface_dict(rng, n, L):
    return dict(surf_points=rng.standard_normal((n, 3)).astype(np.float32), surf_normals=rng.standard_normal((n, 3)).astype(np.float32),
                surf_hks=rng.standard_normal((n, 32)).astype(np.float32), surf_curvatures=rng.standard_normal((n, 10)).astype(np.float32),
                res2surf=rng.integers(0, n, (L, 3, 21)))


def test_surface_reader_concatenation_and_truncation(tmp_path, toy):
    _, d, (pts, feat, r2s) = toy
    got = s3f.load_surface(TOY, "toy.pdb")
    assert got[0].dtype == np.float32 and got[1].shape == (len(pts), 42)
    for a, b in zip(got, (pts, feat, r2s)):
        assert np.array_equal(a, b)
    assert np.array_equal(got[1][:, :32], d["surf_hks"]) and np.array_equal(got[1][:, 32:], d["surf_curvatures"])
    # two files: points and features concatenated, the res2surf rows concatenated as they are (the reference adds no offset)
    rng = np.random.default_rng(3)
    a, b = surface_dict(rng, 40, 6), surface_dict(rng, 55, 5)
    for name, dd in (("a", a), ("b", b)):
        with open(tmp_path / f"{name}.pkl", "wb") as f:
            pickle.dump(dd, f)
    got = s3f.load_surface(str(tmp_path), "a.pdb|b.pdb")
    want = s3f_ref.read_surfaces([a, b])
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert len(got[0]) == 95 and got[2].shape == (11, 3, 21) and got[2][6:].max() < 55
    with pytest.raises(FileNotFoundError, match="c.pkl"):
        s3f.load_surface(str(tmp_path), "a.pdb|c.pdb")
    # truncation: residues [2, 9) of a structure that starts at residue 1 of the sequence
    cut = s3f.cut_surface(*got, 1, 12, 3, 10)
    wp, wf, inverse = s3f_ref.truncate(*want, 1, 3, 10)
    assert np.array_equal(cut[0], wp) and np.array_equal(cut[1], wf) and len(wp) < 95
    assert np.array_equal(wp[inverse], got[0][got[2][2:9]])       # the re-indexed rows name the same points
    whole = s3f.cut_surface(*got, 1, 12, 1, 12)                   # equal ranges still drop the points no residue names
    assert np.array_equal(whole[0], s3f_ref.truncate(*want, 1, 1, 12)[0])
    with pytest.raises(ValueError, match="doesn't match"):
        s3f.cut_surface(*got, 3, 12, 1, 12)
    with pytest.raises(ValueError, match="at least 17"):
        s3f.cut_surface(got[0], got[1], np.zeros((11, 3, 21), np.int64), 1, 12, 1, 12)
    # the fixture whose structure is longer than its window
    kept = s3f.cut_surface(pts, feat, r2s, 0, 37, 0, 30)
    assert 17 <= len(kept[0]) < len(s3f.cut_surface(pts, feat, r2s, 0, 37, 0, 37)[0]) <= len(pts)
    assert np.array_equal(kept[0], s3f_ref.truncate(pts, feat, r2s, 0, 0, 30)[0])


def test_masked_sequences_and_pool_groups():
    assert s3f.pool_groups(5, 1).tolist() == [0, 1, 2, 3, 4, 5]
    assert s3f.pool_groups(4, 2).tolist() == [0, 2, 4]
    assert s3f.pool_groups(5, 2).tolist() == [0, 2, 4, 5]         # an odd count: the last group is short
    assert s3f.pool_groups(2, 4).tolist() == [0, 2]
    for n, b in ((5, 1), (4, 2), (5, 2), (7, 3)):
        off = s3f.pool_groups(n, b)
        assert [list(range(off[g], off[g + 1])) for g in range(len(off) - 1)] == s3f_ref.groups(n, b)
    with pytest.raises(ValueError):
        s3f.pool_groups(3, 0)
    # load_dataset: sorted mutants, one masked sequence per run of equal site tuples; (3, 5) and (5, 3) are two sequences with one set
    rows = s2f.sort_mutants(["A4C", "A4D", "D6E:A4C", "A4C:D6E", "K2R", "A4C:D6F"], [0.0] * 6)
    seqs, seq_of = s3f.masked_sequences(rows, "toy", 20)
    assert [r[0] for r in rows] == [(1,), (3,), (3,), (3, 5), (3, 5), (5, 3)]
    assert seqs == [((0, 20), (1,)), ((0, 20), (3,)), ((0, 20), (3, 5)), ((0, 20), (3, 5))] and seq_of == [0, 1, 1, 2, 2, 3]
    # s2f.position_sets merges the two; its first appearances are in the same order as the reference's list
    _, csr, where = s2f.position_sets(rows, "toy", 20)
    assert len(csr[0][0]) - 1 == 3 and [s for _, s in where] == [0, 1, 1, 2, 2, 2]
    # a long protein: the window follows the first site
    rows = s2f.sort_mutants(["A10C", "A1200C", "A1500C"], [0.0, 0.0, 0.0])
    seqs, _ = s3f.masked_sequences(rows, "toy", 2000)
    assert [w for w, _ in seqs] == [(0, 1022), (1199 - 511, 1199 + 511), (2000 - 1022, 2000)] and seqs[1][1] == (511,)


def test_cli_flags_are_the_references():
    # util.parse_args: -c/--config, -s/--seed and the four named flags; one flag per {{ variable }} of the yaml (s3f.yaml: datadir,
    # structdir, surfdir, ckpt)
    args = cli.parser().parse_args(["-c", "s3f.yaml", "-s", "3", "--datadir", "d", "--ProteinGym_reference_file", "r.csv", "--structdir", "s",
                                    "--surfdir", "u", "--ckpt", "c", "--output_scores_folder", "o", "--DMS_index", "0",
                                    "--MSA_retrieval_location", "e"])
    assert (args.config, args.seed, args.datadir, args.ProteinGym_reference_file, args.structdir, args.surfdir, args.ckpt) == \
        ("s3f.yaml", 3, "d", "r.csv", "s", "u", "c")
    assert (args.output_scores_folder, args.DMS_index, args.MSA_retrieval_location) == ("o", 0, "e")
    assert cli.parser().parse_args(["--config", "x", "--seed", "1", "--datadir", "d", "--ProteinGym_reference_file", "r", "--structdir", "s",
                                    "--surfdir", "u", "--ckpt", "c", "--output_scores_folder", "o"]).DMS_index is None
    with pytest.raises(SystemExit):                               # S3F without surfaces is S2F
        cli.parser().parse_args(["-c", "x", "--datadir", "d", "--ProteinGym_reference_file", "r", "--structdir", "s", "--ckpt", "c",
                                 "--output_scores_folder", "o"])


def test_the_fixtures_knn_lists_are_unambiguous(toy):
    pos, _, (pts, feat, r2s) = toy
    clouds = [(pos, s3f_ref.truncate(pts, feat, r2s, 0, 0, 37)[0]), (pos[:30], s3f_ref.truncate(pts, feat, r2s, 0, 0, 30)[0])]
    clouds += [(s2f_cases.toy(L)[0], s3f_cases.surface(L, ns)[0]) for L, ns in ((37, 17), (37, 33), (37, 250), (9, 40))]
    for ca, cloud in clouds:
        surf, res = s3f_cases.margins(ca, cloud)
        print(f"L {len(ca)} Ns {len(cloud)}: smallest relative gap {surf:.2e} (16th / 17th), {res:.2e} (C-alpha lists)")
        assert surf > 1e-4 and res > 1e-4
    assert len(clouds[1][1]) < len(clouds[0][1])                  # the shorter window keeps fewer points


def test_abi_refusals_without_a_device(lib):
    def config(**kw):
        c = s3f.S3fConfig(s2f=s2f.make_config(128), surf_feat=42, surf_res_neighbors=3, surf_neighbors=16)
        for k, v in kw.items():
            setattr(c.s2f if hasattr(c.s2f, k) else c, k, v)
        return c
    assert lib.pgmi_s3f_weight_count(C.byref(config())) > 2 * lib.pgmi_s2f_weight_count(C.byref(s2f.make_config(128))) - 128 * 128
    for kw, msg in ((dict(surf_feat=40), "surf_feat"), (dict(surf_res_neighbors=4), "surf_res_neighbors"), (dict(surf_neighbors=8), "surf_neighbors"),
                    (dict(node_in=8192), "4096"), (dict(node_in=100), "multiple of 32"), (dict(layers=0), "layers")):
        assert lib.pgmi_s3f_weight_count(C.byref(config(**kw))) == -1
        assert msg in lib.pgmi_last_error().decode()
    h = C.c_void_p()
    blob = np.zeros(8, np.float32)
    assert lib.pgmi_s3f_create(C.byref(config()), _lib.ptr(blob, _lib._f32p), blob.size, None, 0, C.byref(h)) == _lib.EINVAL
    assert "weight blob" in lib.pgmi_last_error().decode() and not h.value
    for call in (lambda: lib.pgmi_s3f_set_structure(None, None, None, 3, None, None, 20),
                 lambda: lib.pgmi_s3f_graph(None, None, None, None, None, None, None, None, None, None, None),
                 lambda: lib.pgmi_s3f_gvp_forward(None, None, None, 1, None, 1, None, None, None, None),
                 lambda: lib.pgmi_s3f_set_logprobs(None, None, 5, None, None, None, 1, None, 1, None, None)):
        assert call() == _lib.EINVAL
    assert lib.pgmi_s3f_profile_model(None, 0) is None
    lib.pgmi_s3f_destroy(None)
